"""rtp_render_guides*: the path camera's first hit per pixel centre, on a
64x48 canvas with the default camera.  Variant 1 has the glass sphere inside
the box, in view; variant 3 is C3 (1000 spheres behind the sphere BVH).

The primitive and the bits of t are checked against the exact scan of
rtp_debug_closest_hit on the same rays, built here in numpy float32 from the
oracle's camera constants (rtp_launch_eval_closest runs closest_hit<kBvh> with
spheres, so its columns cover the spheres and the BVH walk too); the colour
against the scene's texture table, exactly; the normals against a float64
computation from the scene description."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NX, NY = 64, 48
F = np.float32
_cache = {}


def pixel_centre_rays(oracle):
    """camera_ray with both jitter draws 0.5f, in float32 (rtp_kernels.hip camera_ray_at)."""
    cam = oracle.camera_setup(NX, NY)
    eye, nlook, dx, dy = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    pix = np.arange(NX * NY)
    pi, pj = (pix % NX).astype(F), (pix // NX).astype(F)
    a = (F(2) * (pi + (F(1) - F(0.5))) - F(NX)) / F(2)
    b = (F(2) * (pj + F(0.5)) - F(NY)) / F(2)
    rd = (nlook[None, :] + dx[None, :] * a[:, None]) + dy[None, :] * b[:, None]
    rd = np.where(rd == 0, rd + F(0.0000001), rd).astype(F)
    mag = np.sqrt((rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1]) + rd[:, 2] * rd[:, 2])
    d = (rd / mag[:, None]).astype(F)
    assert d.dtype == F
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(eye, d.shape), d], axis=1), dtype=F)


def guides_of(device, oracle, variant):
    if variant not in _cache:
        import raytracingtherestofyourlife_amd as rtp

        device.set_cornell_box(variant)
        cam = rtp.default_camera()
        g0, g1, prim, _ = device.render_guides(cam, NX, NY)
        rays = pixel_centre_rays(oracle)
        exact = device.debug_closest_hit(rays)
        cb = rtp.CornellBox(variant)
        cb.buildDataSet()
        _cache[variant] = dict(g0=g0, g1=g1, prim=prim, rays=rays, exact=exact, cb=cb, cam=cam)
    else:
        device.set_cornell_box(variant)
    return _cache[variant]


def quad_hits_f64(cb, o, d):
    """Per ray: (index of the closest quad in scene order or -1, its t), float64,
    by the Lagae-Dutre test the renderer uses (v00 = p0, v10 = p1, v11 = p2,
    v01 = p3): t and (alpha, beta) in the plane of (v00, v10, v01), and where
    alpha + beta > 1 the corner at v11 decides.  One box top is not planar, so
    the definition matters: its t is the first triangle's plane's."""
    P = cb.coord.astype(np.float64)
    Q = np.asarray(cb.ds.cellset.quad_points).reshape(-1, 4)
    best_t = np.full(len(o), np.inf)
    best_q = np.full(len(o), -1)

    def moller_trumbore(a, b, c):
        e1, e2 = b - a, c - a
        pv = np.cross(d, e2)
        det = pv @ e1
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            tv = o - a
            u = (tv * pv).sum(1) * inv
            qv = np.cross(tv, e1)
            return np.abs(det) > 1e-14, u, (d * qv).sum(1) * inv, (qv @ e2) * inv

    for q, (i0, i1, i2, i3) in enumerate(Q):
        ok, al, be, t = moller_trumbore(P[i0], P[i1], P[i3])
        ok2, ap, bp, _ = moller_trumbore(P[i2], P[i3], P[i1])
        with np.errstate(all="ignore"):
            hit = ok & (al >= 0) & (be >= 0) & (t > 0.001) & (t < best_t)
            hit &= (al + be <= 1) | (ok2 & (ap >= 0) & (bp >= 0))
        best_t = np.where(hit, t, best_t)
        best_q = np.where(hit, q, best_q)
    return best_q, best_t


@pytest.mark.parametrize("variant", [1, 3])
def test_gpu_guides_primitive_and_t(device, oracle, variant):
    g = guides_of(device, oracle, variant)
    prim, g0, exact = g["prim"], g["g0"], g["exact"]
    kind, idx = exact[:, 4].view(np.int32), exact[:, 5].view(np.int32)
    want = np.where(kind < 0, -1, kind * (1 << 24) + idx)
    assert np.array_equal(prim, want), np.flatnonzero(prim != want)[:8]
    hit = prim >= 0
    assert np.array_equal(g0[hit, 3].view(np.uint32), exact[hit, 3])
    # (the path kernel's prefiltered scan agrees with the exact one on these rays)
    assert np.array_equal(exact[:, 0:3], exact[:, 3:6])
    assert hit.sum() > 0.9 * hit.size
    spheres = (prim >> 24) == 1
    if variant == 1:
        assert spheres.sum() > 20, "the glass sphere is in view"
        assert set(prim[spheres] & 0xFFFFFF) == {0}
    else:
        assert device.sphere_walk() != "scan"
        assert len(set(prim[spheres] & 0xFFFFFF)) > 20, "C3's spheres are in view"


@pytest.mark.parametrize("variant", [1, 3])
def test_gpu_guides_miss_values(device, oracle, variant):
    import raytracingtherestofyourlife_amd as rtp

    g = guides_of(device, oracle, variant)
    # the scene's own camera sees a surface almost everywhere: look away for misses
    cam = rtp.Camera()
    cam.SetPosition([278 / 555.0, 278 / 555.0, -800 / 555.0])
    cam.SetLookAt([3.0, 278 / 555.0, -800 / 555.0])
    cam.SetViewUp([0, 1, 0])
    cam.SetFieldOfView(40.0)
    g0, g1, prim, _ = device.render_guides(cam, NX, NY)
    miss = prim == -1
    assert miss.sum() > 0
    for a, m in ((g["g0"], g["prim"] == -1), (g0, miss)):
        assert np.array_equal(a[m, :3], np.zeros((int(m.sum()), 3), F)) and np.isposinf(a[m, 3]).all()
    assert not g1[miss].any() and not g["g1"][g["prim"] == -1].any()
    assert (g1[~miss, 3] == 1).all() and (g["g1"][g["prim"] >= 0, 3] == 1).all()


@pytest.mark.parametrize("variant", [1, 3])
def test_gpu_guides_colour_and_normals(device, oracle, variant):
    g = guides_of(device, oracle, variant)
    cb, prim, g0, g1, rays = g["cb"], g["prim"], g["g0"], g["g1"], g["rays"]
    o, d = rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64)
    kind, idx = prim >> 24, prim & 0xFFFFFF
    hit = prim >= 0
    # the normal faces the ray
    assert ((g0[hit, :3].astype(np.float64) * d[hit]).sum(1) <= 0).all()
    tex = cb.tex[cb.texType]  # float32 [n_tex_type, 3]: tex_rgb[tex_type[.]]

    # spheres: prim's index is the scene's sphere index
    sp = np.flatnonzero(hit & (kind == 1))
    k = idx[sp]
    assert np.array_equal(g1[sp, :3], tex[cb.texIdx[1][k]])
    c = cb.coord[np.asarray(cb.ds.cellset.sphere_points)[k]].astype(np.float64)
    r = cb.SphereRadii[k].astype(np.float64)
    oc = o[sp] - c
    bq = (oc * d[sp]).sum(1)
    aq = (d[sp] * d[sp]).sum(1)  # (the float32 direction is a unit vector only to 1e-7)
    disc = bq * bq - aq * ((oc * oc).sum(1) - r * r)
    root = np.sqrt(np.maximum(disc, 0.0))
    t1, t2 = (-bq - root) / aq, (-bq + root) / aq
    t64 = np.where(t1 > 0.001, t1, t2)

    def sphere_normal(t):
        n = (o[sp] + t[:, None] * d[sp] - c) / r[:, None]
        return np.where(((n * d[sp]).sum(1) > 0)[:, None], -n, n)

    # The guide's normal is (hp - c) / r at the hit point of the guide's own t
    # (whose bits are checked against the exact scan above): the float64
    # evaluation of that expression is the reference.  An independent float64
    # intersection differs from it by the path kernel's sphere_hit rounding of
    # t, which at grazing incidence (a small discriminant under the root) is
    # amplified by 1 / r: measured 3.2e-5 on variant 1's glass sphere
    # (r = 90 / 555); it is printed, not asserted.
    err_s = np.abs(g0[sp, :3] - sphere_normal(g0[sp, 3].astype(np.float64))).max() if sp.size else 0.0
    err_i = np.abs(g0[sp, :3] - sphere_normal(t64)).max() if sp.size else 0.0
    print(f"variant {variant}: {sp.size} sphere pixels, smallest radius {r.min() if sp.size else 0:.5g}, "
          f"max normal error {err_s:.3g} (against an independent float64 intersection {err_i:.3g})")
    assert err_s <= 1e-5

    # quads: prim's index is the scan position; the scene quad behind each
    # position is the one a float64 intersection finds for most of its pixels
    qd = np.flatnonzero(hit & (kind == 0))
    q64, t64q = quad_hits_f64(cb, o[qd], d[qd])
    pos_to_quad = {}
    for p in np.unique(idx[qd]):
        votes = q64[idx[qd] == p]
        votes = votes[votes >= 0]
        lost = qd[idx[qd] == p][:6]
        assert votes.size, (f"scan position {p}: no float64 quad hit on its pixels {lost.tolist()}, t "
                            f"{g0[lost, 3].tolist()}, hit points {(o[lost] + g0[lost, 3:4] * d[lost]).tolist()}")
        pos_to_quad[int(p)] = int(np.bincount(votes).argmax())
    quad = np.array([pos_to_quad[int(p)] for p in idx[qd]])
    # (float64 and float32 may disagree on the quad only along shared edges)
    assert (quad == q64).mean() > 0.97
    assert np.array_equal(g1[qd, :3], tex[cb.texIdx[0][quad]])
    P = cb.coord.astype(np.float64)
    Q = np.asarray(cb.ds.cellset.quad_points).reshape(-1, 4)
    nq = np.cross(P[Q[:, 1]] - P[Q[:, 0]], P[Q[:, 2]] - P[Q[:, 0]])
    nq /= np.linalg.norm(nq, axis=1, keepdims=True)
    n64 = nq[quad]
    n64 = np.where(((n64 * d[qd]).sum(1) > 0)[:, None], -n64, n64)
    err_q = np.abs(g0[qd, :3] - n64).max()
    print(f"variant {variant}: {qd.size} quad pixels, max normal error {err_q:.3g}")
    assert err_q <= 1e-5
    same = quad == q64
    assert np.abs(g0[qd, 3][same] - t64q[same]).max() <= 1e-4 * t64q[same].max()


def test_gpu_guides_repeatable_and_device_variant(device, oracle):
    import torch

    g = guides_of(device, oracle, 1)
    td = torch.device("cuda", device.device)
    n = NX * NY
    bufs = []
    for _ in range(2):
        g0 = torch.full((n, 4), 7.0, dtype=torch.float32, device=td)
        g1 = torch.full((n, 4), 7.0, dtype=torch.float32, device=td)
        prim = torch.full((n,), 7, dtype=torch.int32, device=td)
        device.render_guides_device(g["cam"], NX, NY, g0.data_ptr(), g1.data_ptr(), prim.data_ptr(),
                                    stream=torch.cuda.current_stream(td).cuda_stream)
        bufs.append((g0.cpu().numpy(), g1.cpu().numpy(), prim.cpu().numpy()))
    for a, b, h in zip(bufs[0], bufs[1], (g["g0"], g["g1"], g["prim"])):
        assert a.tobytes() == b.tobytes() == h.tobytes()
    # each output alone
    only = torch.full((n,), 7, dtype=torch.int32, device=td)
    st = device.render_guides_device(g["cam"], NX, NY, prim_ptr=only.data_ptr(), timed=True)
    assert st.kernel_ms > 0 and np.array_equal(only.cpu().numpy(), g["prim"])


def test_gpu_guides_argument_checks(device):
    import torch

    import raytracingtherestofyourlife_amd as rtp

    device.set_cornell_box(1)
    td = torch.device("cuda", device.device)
    buf = torch.full((16, 4), 7.0, dtype=torch.float32, device=td)
    cam = rtp.default_camera()
    for call in (lambda: device.render_guides_device(None, 4, 4, buf.data_ptr()),
                 lambda: device.render_guides_device(cam, 0, 4, buf.data_ptr()),
                 lambda: device.render_guides_device(cam, 4, -2, buf.data_ptr()),
                 lambda: device.render_guides_device(cam, 4, 4)):
        with pytest.raises(rtp.RtpError) as e:
            call()
        assert e.value.status == rtp._lib.RTP_ERR_INVALID_ARGUMENT
    fresh = rtp.Device(device.device)
    try:
        with pytest.raises(rtp.RtpError) as e:
            fresh.render_guides_device(cam, 4, 4, buf.data_ptr())
        assert e.value.status == rtp._lib.RTP_ERR_NO_SCENE
    finally:
        fresh.close()
    torch.cuda.synchronize(td)
    assert bool((buf == 7.0).all())
