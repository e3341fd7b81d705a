"""CPU guards of the generated sphere sets (tests/_spheres.py): what
tests/test_gpu_sphere_zoo.py relies on holds by the references alone -- the
float32 restatement of the sphere root against the float64 rows, the scenes
in the oracle, and that each set holds the cases it is there for (exact ties,
near ties, grazing rays that float32 accepts outside the sphere's own box as
it was padded before the soundness bound, infinite box faces, fair shares of
sphere and quad hits).  Each assert's message carries the counts found."""
from __future__ import annotations

import numpy as np
import pytest

import _scenes as S
import _spheres as Z

F = np.float32
_sets = {}


def _rays(name):
    if name not in _sets:
        _sets[name] = Z.ray_sets(Z.variant(name))
    return _sets[name]


def _union(name):
    return np.concatenate(list(_rays(name).values()))


def test_variants_hold_what_they_are_named_for():
    for n in (8, 9, 10, 300, 2000):
        assert len(Z.variant(f"count{n}").spheres) == n
    z = Z.variant("duplicates")
    c, r = Z.centres(z), Z.radii(z)
    assert len(z.spheres) == 40 and len(z.groups) == 10
    for g in z.groups:
        assert all(c[i].tobytes() == c[g[0]].tobytes() and r[i] == r[g[0]] for i in g)
        assert g[1] - g[0] > 1 and g[2] - g[1] > 1
    for lo, hi, m, _, _ in z.mirror:
        assert lo < hi and c[lo][0] > c[hi][0] and c[lo][0] - F(m) == F(m) - c[hi][0] and r[lo] == r[hi]
    for name in ("all_equal", "concentric"):
        c = Z.centres(Z.variant(name))
        assert len(c) == 16 and (c == c[0]).all()
    assert np.unique(Z.radii(Z.variant("all_equal"))).size == 1
    assert np.unique(Z.radii(Z.variant("concentric"))).size == 16
    c = Z.centres(Z.variant("line"))
    assert np.unique(c[:, 0]).size == len(c) and (c[:, 1:] == c[0, 1:]).all()
    c = Z.centres(Z.variant("plane"))
    assert (c[:, 1] == c[0, 1]).all() and np.unique(c[:, 0]).size == len(c)
    z = Z.variant("cluster")
    c = Z.centres(z)[2:]
    assert len(z.spheres) == 500 and (c.max(0) - c.min(0)).max() <= 2.0 ** -11
    # the device builder's 30-bit codes, from their definition: 10 bits per axis over the centres' bounds
    call = Z.centres(z)
    q = np.clip(((call - call.min(0)) / (call.max(0) - call.min(0)) * F(1024)).astype(np.int64), 0, 1023)
    codes = np.unique(q, axis=0).shape[0]
    assert codes <= 12, f"{codes} distinct Morton codes among 500 spheres"
    z = Z.variant("near_ties")
    c, r = Z.centres(z), Z.radii(z)
    dc = (c[32:] - c[:32]).astype(np.float64)
    assert (r[32:] == r[:32]).all() and ((dc != 0).sum(1) == 1).all()
    assert (np.abs(dc).max(1) > 0.9e-5).all() and (np.abs(dc).max(1) < 1.1e-4).all()
    assert (dc.sum(1) < 0).sum() == 16, "the higher index is the nearer one for half of the pairs"
    z = Z.variant("nested")
    c, r = Z.centres(z).astype(np.float64), Z.radii(z).astype(np.float64)
    big = int(r.argmax())
    assert r[big] == F(0.6)
    assert all(np.linalg.norm(c[k] - c[big]) + r[k] < r[big] for k in range(len(r) - 1) if k != big)
    assert np.linalg.norm(c[-1] - z.cam["position"]) < r[-1], "the last sphere contains the camera"
    assert all(np.linalg.norm(c[k + 1] - c[k]) < r[k] + r[k + 1] for k in range(1, 12)), "a chain of overlaps"


def test_extreme_spheres_define_the_cloud_and_sit_on_the_half_grid():
    for name, pad in (("extreme", None), ("extreme_new_pad", "new")):
        z = Z.variant(name)
        c, r = Z.centres(z).astype(np.float64), Z.radii(z).astype(np.float64)
        lo, hi = Z.boxes(z, Z.pad_new(z) if pad else Z.pad_old(Z.centres(z), Z.radii(z)))
        rest = np.setdiff1d(np.arange(len(r)), [e[0] for e in z.extreme])
        assert set(np.unique(Z.radii(z))) == {F(1 / 555), F(0.25 / 555)}
        for k, a, up in z.extreme:
            face = (hi if up else lo)[k, a]
            gap = abs(float(Z.half_outward(face, up)) - float(face))
            assert 0 < gap <= 2e-6, (name, k, a, up, gap)
            if up:
                assert (c[rest, a] + r[rest] < c[k, a] - r[k]).all() and hi[k, a] == hi[:, a].max()
            else:
                assert (c[rest, a] - r[rest] > c[k, a] + r[k]).all() and lo[k, a] == lo[:, a].min()


def test_half_outward_restatement():
    x = np.array([0.1, -0.1, 65504.0, 65505.0, 70000.0, -70000.0, 0.0, 1e-9, -1e-9, 0.333], dtype=F)
    up, dn = Z.half_outward(x, True), Z.half_outward(x, False)
    assert (up >= x).all() and (dn <= x).all()
    assert up[3] == np.inf and up[4] == np.inf and dn[4] == F(65504) and dn[5] == -np.inf and up[5] == F(-65504)
    assert (up[[2, 6]] == x[[2, 6]]).all() and up[7] == F(2.0 ** -24) and dn[8] == F(-(2.0 ** -24))
    fin = np.isfinite(up) & np.isfinite(dn)
    assert (up[fin].astype(np.float16).astype(F) == up[fin]).all()
    assert (np.nextafter(up[fin].astype(np.float16), np.float16(-np.inf)).astype(F) < x[fin]).all(), "the nearest such"


@pytest.mark.parametrize("name", sorted(Z.VARIANTS))
def test_float32_restatement_agrees_with_float64_away_from_silhouettes(name):
    """Away from silhouettes (|disc| above 1e-3 of b b for every sphere, in
    float64) sphere_hits_f32's t is the float64 rows' within a relative 1e-4,
    and it picks the same sphere wherever the float64 runner-up (other than
    an exact tie, which both give to the lower index) is farther than that.
    Rays with a root of some sphere within 1e-5 (scene units) of tmin are
    left out: which root counts there is a rounding away."""
    z = Z.variant(name)
    nq, ns = len(z.quads), len(z.spheres)
    r = _union(name)
    r = r[np.isfinite(r).all(1)]
    r = r[:: max(1, (ns * len(r)) >> 23)]
    o, d = r[:, :3].astype(np.float64), r[:, 3:].astype(np.float64)
    T = S.hits_f64(z, o, d)[nq:]
    c, rad = Z.centres(z).astype(np.float64), Z.radii(z).astype(np.float64)
    away = np.ones(len(r), dtype=bool)
    for k in range(ns):
        oc = o - c[k]
        b, a = (oc * d).sum(1), (d * d).sum(1)
        disc = b * b - a * ((oc * oc).sum(1) - rad[k] ** 2)
        root = np.sqrt(np.maximum(disc, 0))
        near_tmin = (disc > 0) & ((np.abs((-b - root) / a - 0.001) < 1e-5 * z.scale) |
                                  (np.abs((-b + root) / a - 0.001) < 1e-5 * z.scale))
        away &= (np.abs(disc) > 1e-3 * b * b) & ~near_tmin
    t32, i32 = Z.sphere_hits_f32(z, r[:, :3], r[:, 3:])
    cols = np.arange(len(r))
    first = T.argmin(0)
    t64 = T[first, cols]
    hit64 = np.isfinite(t64)
    assert np.array_equal(np.isfinite(t32[away]), hit64[away]), "the same rays hit some sphere"
    sel = away & hit64
    rel = np.abs(t32[sel].astype(np.float64) - t64[sel]) / t64[sel]
    rest = np.where(T == t64[None, :], np.inf, T).min(0)
    clear = sel & (rest > t64 * (1 + 1e-4))
    wrong = int((i32[clear] != first[clear]).sum())
    print(f"{name}: {int(away.sum())} of {len(r)} rays away from silhouettes, {int(sel.sum())} hit a sphere, "
          f"max relative t error {rel.max() if rel.size else 0:.3g}, {int(clear.sum())} clear, {wrong} other sphere")
    # (in a crowded scene most rays pass some sphere's silhouette band, which is 1e-3 D^2 / 2r wide;
    # a restatement wrong in any operation is wrong on every ray)
    assert sel.sum() >= 100, f"{name}: only {int(sel.sum())} rays to compare"
    assert rel.max() <= 1e-4, f"{name}: t differs by a relative {rel.max():.3g} ({int((rel > 1e-4).sum())} rays)"
    assert wrong == 0, f"{name}: {wrong} of {int(clear.sum())} clear rays pick another sphere"
    # exact float64 ties go to the lower index in both
    tie = sel & (rest > t64 * (1 + 1e-4)) & ((T == t64[None, :]).sum(0) > 1)
    assert (i32[tie] == first[tie]).all()


@pytest.mark.parametrize("name", ["count9", "duplicates"])
def test_oracle_renders_the_scene(oracle, name):
    z = Z.variant(name)
    nx = ny = 32
    pix = np.sort(np.random.default_rng(2).choice(nx * ny, 64, replace=False)).astype(np.int64)
    rgba, _, live = oracle.render_pixels(z.scene(oracle), z.oracle_camera(oracle, nx, ny), nx, ny, 2, 5, pix)
    fin = np.isfinite(rgba[:, :3]).all(1)
    assert fin.mean() >= 0.9, f"{name}: {int(fin.sum())} of 64 pixels finite"
    assert live.sum() > 64, f"{name}: {int(live.sum())} live bounces"


def test_duplicates_rays_meet_exact_ties():
    z = Z.variant("duplicates")
    r = _union("duplicates")
    T = Z.sphere_roots_f32(z, r[:, :3], r[:, 3:])
    t, i = Z.sphere_hits_f32(z, r[:, :3], r[:, 3:])
    assert np.array_equal(i, np.where(np.isfinite(T.min(0)), T.argmin(0), -1))
    tied = np.isfinite(t) & ((T == t[None, :]).sum(0) >= 2)
    # the sphere first in ascending-x centre order (stable: equal centres in index order) among the tied ones
    order = np.argsort(Z.centres(z)[:, 0], kind="stable")
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    first_x = np.where(T == t[None, :], rank[:, None], len(order)).argmin(0)
    other = tied & (first_x != i)
    oct_neg = tied & (r[:, 3:] < 0).any(1)
    print(f"duplicates: {int(tied.sum())} rays end in an exact tie, in {int(other.sum())} the lower index is not the "
          f"first in x order, {int(oct_neg.sum())} have a negative direction component")
    assert tied.sum() >= 200, f"{int(tied.sum())} tied rays"
    assert other.sum() >= 50, f"{int(other.sum())} tied rays whose lower index is not first in x order"
    assert oct_neg.sum() >= 100 and (tied & ~oct_neg).sum() >= 20, "ties are met in both walk orders"
    for name in ("all_equal", "concentric"):
        zz, rr = Z.variant(name), _union(name)
        tt, ii = Z.sphere_hits_f32(zz, rr[:, :3], rr[:, 3:])
        assert np.isfinite(tt).sum() >= 1000, f"{name}: {int(np.isfinite(tt).sum())} rays hit"
        if name == "all_equal":
            assert (ii[np.isfinite(tt)] == 0).all()
        else:
            assert np.unique(ii[np.isfinite(tt)]).size >= 8, "origins lie between the shells"


def test_near_ties_rays_meet_near_ties():
    z = Z.variant("near_ties")
    r = _union("near_ties")
    T = np.sort(Z.sphere_roots_f32(z, r[:, :3], r[:, 3:]), axis=0)
    _, i = Z.sphere_hits_f32(z, r[:, :3], r[:, 3:])
    with np.errstate(invalid="ignore"):
        near = np.isfinite(T[1]) & (T[1] - T[0] < 1e-4 * T[0])
    hi, lo = int((near & (i >= 32)).sum()), int((near & (i < 32)).sum())
    print(f"near_ties: {int(near.sum())} rays with two roots within a relative 1e-4; the higher index wins {hi}, "
          f"the lower {lo}")
    assert near.sum() >= 200 and hi >= 50 and lo >= 50, f"{int(near.sum())} near ties, higher wins {hi}, lower {lo}"


def test_graze_rays_leave_the_old_boxes():
    """What makes the GPU test of the extreme set meaningful: float32 accepts
    rays on a sphere that miss that sphere's own box, padded as before the
    soundness bound and rounded outward to half precision, on the side the
    sphere defines for the whole cloud -- no box above it can be wider there."""
    z = Z.variant("extreme")
    g = _rays("extreme")["graze"]
    t, i = Z.sphere_hits_f32(z, g[:, :3], g[:, 3:])
    ext = np.array([e[0] for e in z.extreme])
    lo, hi = Z.boxes(z, Z.pad_old(Z.centres(z), Z.radii(z)))
    lo, hi = Z.half_outward(lo, False), Z.half_outward(hi, True)
    on = np.isin(i, ext)
    k = np.where(on, i, ext[0])
    out = on & Z.slab_misses(lo[k], hi[k], g[:, :3], g[:, 3:])
    lo2, hi2 = Z.boxes(z, Z.pad_new(z))
    out2 = on & Z.slab_misses(lo2[k], hi2[k], g[:, :3], g[:, 3:])
    print(f"extreme: of {len(g)} grazing rays float32 accepts {int(on.sum())} on an extreme sphere; {int(out.sum())} "
          f"miss its box with the old pad, {int(out2.sum())} with the soundness bound")
    assert out.sum() >= 200, f"{int(out.sum())} accepted rays miss the old box ({int(on.sum())} accepted)"
    assert out2.sum() == 0, f"{int(out2.sum())} accepted rays miss the box with the soundness bound"


@pytest.mark.parametrize("name", sorted(Z.VARIANTS))
def test_soundness_bound_holds_for_every_accepted_ray(name):
    """The bound itself, on every ray of the sets within the reach: a ray
    that float32 accepts on a sphere crosses that sphere's box (pad_new,
    exact slab test), and the point at the accepted t lies inside it."""
    z = Z.variant(name)
    r = _union(name)
    r = r[np.isfinite(r).all(1)]
    r = r[:: max(1, (len(z.spheres) * len(r)) >> 22)]
    lo, hi = Z.boxes(z, Z.pad_new(z))
    c = Z.centres(z).astype(np.float64)
    o, d = r[:, :3].astype(np.float64), r[:, 3:].astype(np.float64)
    bad = total = 0
    for s0 in range(0, len(z.spheres), 32):
        T = Z.sphere_roots_f32(z, r[:, :3], r[:, 3:], s0, s0 + 32)
        for j in range(T.shape[0]):
            k = s0 + j
            acc = np.isfinite(T[j]) & (np.linalg.norm(o - c[k], axis=1) <= float(Z.reach(z)))
            if not acc.any():
                continue
            p = o[acc] + d[acc] * T[j][acc].astype(np.float64)[:, None]
            inside = ((p >= lo[k]) & (p <= hi[k])).all(1)
            bad += int((~inside).sum()) + int(Z.slab_misses(lo[k], hi[k], o[acc], d[acc]).sum())
            total += int(acc.sum())
    print(f"{name}: {total} accepted (ray, sphere) pairs within the reach, {bad} outside the box")
    assert total >= 1000 and bad == 0, f"{name}: {bad} of {total} accepted pairs leave the padded box"


@pytest.mark.parametrize("name", sorted(Z.VARIANTS))
def test_camera_rays_see_spheres_and_quads(name):
    z = Z.variant(name)
    r = _rays(name)["camera"]
    nq = len(z.quads)
    if len(z.spheres) * len(r) > 1 << 22:
        r = r[:: (len(z.spheres) * len(r)) >> 22]
    T = S.hits_f64(z, r[:, :3].astype(np.float64), r[:, 3:].astype(np.float64))
    first = T.argmin(0)
    hit = np.isfinite(T.min(0))
    sph, quad = (hit & (first >= nq)).mean(), (hit & (first < nq)).mean()
    print(f"{name}: of {len(r)} camera rays {sph:.3f} hit a sphere first, {quad:.3f} a quad")
    assert sph >= 0.1 and quad >= 0.1, f"{name}: sphere share {sph:.3f}, quad share {quad:.3f}"


def test_far_boxes_reach_past_half_precision():
    z = Z.variant("far_beyond_half")
    for pad in (Z.pad_old(Z.centres(z), Z.radii(z)), Z.pad_new(z)):
        lo, hi = Z.boxes(z, pad)
        n = int((hi > 65504).any(1).sum() + (lo < -65504).any(1).sum())
        assert n == 3, f"{n} sphere boxes with a face beyond 65504"
        assert np.isinf(Z.half_outward(hi.max(0), True)).any() and np.isinf(Z.half_outward(lo.min(0), False)).any()
    assert np.abs(Z.centres(Z.variant("far"))).max() > 400 and Z.variant("far").scale == 555.0
