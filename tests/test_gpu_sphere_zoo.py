"""GPU parity of the sphere BVH on generated sphere sets (tests/_spheres.py),
ray by ray: both builders (the host's binned SAH, the device LBVH), the
half-precision compact nodes, the walks (spheres_bvh behind
rtp_debug_closest_hit and the guides, the pool kernel's resumable loop and
the LDS walk behind the renders) and RTP_BVH_DROP -- on counts next to the
BVH threshold and past the inline array, the cloud's extreme spheres on the
half-precision grid with rays grazing them, bit-identical and concentric
spheres, near ties, degenerate extents, nested spheres, the reference's
units and boxes that round to an infinity.  tests/test_sphere_zoo.py guards
these inputs on the CPU.

The contract is bit equality with the brute-force scan: the lexicographic
minimum of (t, quads before spheres, sphere index), every sphere tested by
the float32 sphere root.  The spheres' part is _spheres.sphere_hits_f32, a
numpy restatement with no tree in it; the quads' part is read from the
device on a scene with the same quads and one sphere out of every ray's way
(the scan path, which the quad tests hold to the oracle).  Renders are
compared with the C oracle bit for bit."""
from __future__ import annotations

import numpy as np
import pytest

import _scenes as S
import _spheres as Z
from _util import assert_render_equal, set_scene_from_oracle

pytestmark = pytest.mark.gpu

F = np.float32
BVH_MIN = 9  # spheres from which a scene gets the BVH
_refs = {}
_wants = {}


@pytest.fixture(scope="module")
def rtp():
    import raytracingtherestofyourlife_amd as m

    return m


def _walk(z):
    return "scan" if len(z.spheres) < BVH_MIN else "global"


def _expected(device, oracle, z, rays):
    """The expected combined hit of each ray (three uint32 words)."""
    set_scene_from_oracle(device, Z.parked(z).scene(oracle))
    assert device.sphere_walk() == "scan"
    q = device.debug_closest_hit(rays)
    assert (q[:, 4] != 1).all() and (q[:, 1] != 1).all(), "a ray reached the parked sphere"
    assert Z.same_hits(q[:, 0:3], q[:, 3:6]).all()
    t, i = Z.sphere_hits_f32(z, rays[:, :3], rays[:, 3:])
    return Z.expected_hits(q[:, 3:6], t, i)


def _reference(device, oracle, name):
    """(rays, expected hits, kind of each ray) of a variant, computed once."""
    if name not in _refs:
        z = Z.variant(name)
        sets = Z.ray_sets(z)
        rays = np.concatenate(list(sets.values()))
        assert len(rays) <= 1 << 16
        kind = np.concatenate([[k] * len(v) for k, v in sets.items()])
        _refs[name] = (rays, _expected(device, oracle, z, rays), kind)
    return _refs[name]


def _mismatch(what, rays, got, want, kind=None):
    bad = np.flatnonzero(~Z.same_hits(got, want))
    if bad.size == 0:
        return None
    def triple(w):
        return f"(t {float(w[0:1].copy().view(F)[0])!r}, kind {int(w[1].astype(np.int32))}, index {int(w[2])})"

    rows = [f"ray {int(j)}{'' if kind is None else ' (' + str(kind[j]) + ')'} o {rays[j, :3].tolist()} d "
            f"{rays[j, 3:].tolist()}: got {triple(got[j])}, want {triple(want[j])}" for j in bad[:4]]
    by = "" if kind is None else " " + str({str(k): int(n) for k, n in zip(*np.unique(kind[bad], return_counts=True))})
    return f"{what}: {bad.size} of {len(rays)} rays differ{by}; " + "; ".join(rows)


# -------------------------------------------------------------- ray level --
CASES = [("count8", "host", None)] + [(n, b, d) for n in sorted(Z.VARIANTS) if n != "count8"
                                      for b in ("host", "gpu") for d in (None, "0")]


@pytest.mark.parametrize("name,builder,drop", CASES)
def test_closest_hit_equals_brute_force(device, oracle, monkeypatch, name, builder, drop):
    """Columns 3..5 of rtp_debug_closest_hit (the exact quad scan, then the
    sphere walk) are the expected combined hit bit for bit, and columns 0..2
    (prefiltered) equal them.  For count8 this runs on the scan path: a check
    of this file's restatement against code the oracle renders vouch for."""
    z = Z.variant(name)
    try:
        rays, want, kind = _reference(device, oracle, name)
        monkeypatch.setenv("RTP_BVH_BUILD", builder)
        if drop is not None:
            monkeypatch.setenv("RTP_BVH_DROP", drop)
        set_scene_from_oracle(device, z.scene(oracle))
        assert device.sphere_walk() == _walk(z)
        got = device.debug_closest_hit(rays)
    finally:
        device.set_cornell_box(0)
    what = f"{name}, {builder} builder, RTP_BVH_DROP {drop}"
    msg = _mismatch(what, rays, got[:, 3:6], want, kind)
    assert msg is None, msg
    msg = _mismatch(what + ", prefiltered against exact", rays, got[:, 0:3], got[:, 3:6], kind)
    assert msg is None, msg
    sph = want[:, 1] == 1
    assert sph.mean() > 0.05 and (want[:, 1] == 0).mean() > 0.05, "the rays meet spheres and quads"


# ----------------------------------------------------------------- guides --
@pytest.mark.parametrize("name", ["count9", "nested", "extreme"])
def test_guides_equal_brute_force(device, oracle, rtp, name):
    """The second caller of spheres_bvh: the guides' primitive and t of the
    default camera's pixel centres at 64 x 64."""
    z = Z.variant(name)
    nx = ny = 64
    o, d = S.pixel_centre_rays(z.oracle_camera(oracle, nx, ny), nx, ny)
    rays = np.concatenate([o, d], axis=1).astype(F)
    try:
        want = _expected(device, oracle, z, rays)
        set_scene_from_oracle(device, z.scene(oracle))
        assert device.sphere_walk() == "global"
        g0, _, prim, _ = device.render_guides(z.camera(rtp), nx, ny)
    finally:
        device.set_cornell_box(0)
    miss = want[:, 1] == 0xFFFFFFFF
    wprim = np.where(miss, -1, (want[:, 1].astype(np.int64) << 24) + want[:, 2]).astype(np.int32)
    wt = np.where(miss, F(np.inf), want[:, 0].copy().view(F))
    got = np.stack([g0[:, 3].copy().view(np.uint32), (prim >> 24).astype(np.uint32),
                    np.where(prim < 0, 0, prim & 0xFFFFFF).astype(np.uint32)], axis=1)
    wanted = np.stack([wt.view(np.uint32), (wprim >> 24).astype(np.uint32),
                       np.where(wprim < 0, 0, wprim & 0xFFFFFF).astype(np.uint32)], axis=1)
    msg = _mismatch(f"{name}, guides", rays, got, wanted)
    assert msg is None, msg
    assert ((wprim >> 24) == 1).mean() > 0.05


# ----------------------------------------------------------- render level --
NX = NY = 64
RENDERED = ["count9", "count300", "duplicates", "near_ties", "extreme", "nested", "cluster"]


def _pixels(n, seed=5):
    return np.sort(np.random.default_rng(seed).choice(NX * NY, n, replace=False)).astype(np.int64)


def _want(oracle, key, z, pix, spp=4, depth=50):
    """The oracle's render, computed once per scene and camera."""
    if key not in _wants:
        _wants[key] = oracle.render_pixels(z.scene(oracle), z.oracle_camera(oracle, NX, NY), NX, NY, spp, depth, pix)
    return _wants[key]


def _render_case(device, oracle, rtp, monkeypatch, z, key, mode, pix):
    builder, lds, walk = {"global": ("host", "0", "global"), "global_gpu": ("gpu", "0", "global"),
                          "lds": ("host", "1", "lds")}[mode]
    want = _want(oracle, key, z, pix)
    try:
        monkeypatch.setenv("RTP_BVH_BUILD", builder)
        monkeypatch.setenv("RTP_BVH_LDS", lds)
        set_scene_from_oracle(device, z.scene(oracle))
        assert device.sphere_walk() == walk
        got = device.render_pixels(z.camera(rtp), NX, NY, 4, 50, pix)[:3]
    finally:
        monkeypatch.delenv("RTP_BVH_LDS", raising=False)
        device.set_cornell_box(0)
    assert_render_equal(got, want, f"{key}, {mode}")


@pytest.mark.parametrize("mode", ["global", "global_gpu", "lds"])
@pytest.mark.parametrize("name", RENDERED)
def test_render_equals_oracle(device, oracle, rtp, monkeypatch, name, mode):
    """The pool kernel's resumable walk (either builder's tree) and the LDS
    walk (every one of these sets fits the block's LDS): 256 pixels, 4 spp,
    depth 50 against the oracle -- rgb, final RNG state, live bounces."""
    _render_case(device, oracle, rtp, monkeypatch, Z.variant(name), name, mode, _pixels(256))


def narrow_camera(z):
    """A camera 2.0 in front of the silhouette point of the cloud's lowest
    sphere in x, looking along +z at it, whose 64 x 64 frame spans 64 * 2e-5
    there: the primary rays are themselves in the grazing band."""
    k, a, up = z.extreme[0]
    assert (a, up) == (0, False)
    p = Z.centres(z)[k].astype(np.float64) - (float(Z.radii(z)[k]), 0.0, 0.0)
    fov = np.degrees(2 * np.arctan(32 * 2e-5 / 2.0))
    return dict(position=(p - (0.0, 0.0, 2.0)).astype(F), look_at=p.astype(F), view_up=np.array([0, 1, 0], dtype=F),
                fov_y=float(F(fov)))


@pytest.mark.parametrize("mode", ["global", "global_gpu", "lds"])
def test_render_grazing_camera_equals_oracle(device, oracle, rtp, monkeypatch, mode):
    import copy

    z = copy.copy(Z.variant("extreme"))
    z.cam = narrow_camera(z)
    cam12 = z.oracle_camera(oracle, NX, NY)
    o, d = S.pixel_centre_rays(cam12, NX, NY)
    t, i = Z.sphere_hits_f32(z, o.astype(F), d.astype(F))
    share = float((i == z.extreme[0][0]).mean())
    assert 0.2 < share < 0.8, f"the silhouette crosses the frame: {share:.2f} of the pixel centres hit the sphere"
    _render_case(device, oracle, rtp, monkeypatch, z, "extreme, grazing camera", mode, _pixels(256, 6))


def test_lds_fit_boundary(device, oracle, rtp, monkeypatch):
    """The largest count of the uniform generator whose tree the LDS walk
    takes (found by bisection over set_scene and sphere_walk alone), and that
    count + 1, which walks the global tree: both render as the oracle does."""
    monkeypatch.setenv("RTP_BVH_BUILD", "host")
    monkeypatch.setenv("RTP_BVH_LDS", "1")

    def walk(n):
        set_scene_from_oracle(device, Z.uniform(n, 41).scene(oracle))
        return device.sphere_walk()

    try:
        lo, hi = 300, 2000
        assert walk(lo) == "lds" and walk(hi) == "global"
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if walk(mid) == "lds":
                lo = mid
            else:
                hi = mid
        print(f"the LDS walk takes {lo} uniform spheres, not {hi}")
        pix = _pixels(128, 7)
        for n, want_walk in ((lo, "lds"), (hi, "global")):
            z = Z.uniform(n, 41)
            sc = z.scene(oracle)
            want = oracle.render_pixels(sc, z.oracle_camera(oracle, NX, NY), NX, NY, 4, 50, pix)
            set_scene_from_oracle(device, sc)
            assert device.sphere_walk() == want_walk
            got = device.render_pixels(z.camera(rtp), NX, NY, 4, 50, pix)[:3]
            assert_render_equal(got, want, f"{n} uniform spheres, {want_walk} walk")
    finally:
        device.set_cornell_box(0)


def test_count2000_does_not_fit_the_lds(device, oracle, monkeypatch):
    monkeypatch.setenv("RTP_BVH_BUILD", "host")
    monkeypatch.setenv("RTP_BVH_LDS", "1")
    try:
        set_scene_from_oracle(device, Z.variant("count2000").scene(oracle))
        assert device.sphere_walk() == "global"
    finally:
        device.set_cornell_box(0)
