"""Adaptive sampling on the device (include/rtp_adaptive.h; csrc/rtp_adaptive.hip):
the noise estimate and the selection against their numpy float32 restatements
(tests/_adaptive_ref.py) bit for bit, and the adaptive pass against its parts --
ProgressiveRender.step over the restatement's pixel list -- and against
Device.render_pixels of each pixel's sample count.  A mismatch here is a kernel
or compiler-flag problem, never a tolerance to loosen."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from _adaptive_ref import F, active_ref, finite_ref, noise_ref
from _util import assert_render_equal, same_bits_or_both_nan
from raytracingtherestofyourlife_amd.adaptive import SELECT_BLOCK as B  # entries per block of the selection

pytestmark = pytest.mark.gpu

DEPTH = 8
# The adaptive tests' threshold: the median noise of the 4-spp state of the
# 64x48 variant-0 canvas at depth 8 (measured: 0.6002; the 48x40 canvas 0.5977).
# Measured shares of the canvas selected at this value by the three rounds of
# test_gpu_refine_pass_equals_its_parts: 0.500, 0.339, 0.220; by the one round
# on the 32x32 variant-3 canvas (most of it black: median noise 0): 0.163.
THRESHOLD = 0.6
POISON = -7


def _dev(device, a):
    import torch

    return torch.from_numpy(np.array(a, copy=True)).to(torch.device("cuda", device.device))


def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return bool(same_bits_or_both_nan(a, b).all())
    return bool(np.array_equal(a, b))


def _states_equal(sa, sb, what):
    for k in ("sums", "seed", "live", "m2", "count"):
        assert _bits_equal(sa[k], sb[k]), f"{what}: {k} differs"


def run_noise(device, sums, m2, count):
    import torch

    from raytracingtherestofyourlife_amd import adaptive

    n = count.size
    d_s, d_m, d_c = _dev(device, sums), _dev(device, m2), _dev(device, count)
    out = torch.full((n + 64,), 7.0, dtype=torch.float32, device=d_s.device)
    st = adaptive.noise_device(device, d_s.data_ptr(), d_m.data_ptr(), d_c.data_ptr(), n, out.data_ptr(), timed=True)
    assert st.kernel_ms > 0
    got = out.cpu().numpy()
    assert (got[n:] == 7.0).all(), "the kernel wrote past its n entries"
    return got[:n]


def run_select(device, sums, m2, count, spp, threshold, max_spp):
    """(ids int64 [n] with POISON where nothing was written, total)."""
    import torch

    from raytracingtherestofyourlife_amd import adaptive

    n = count.size
    d_s, d_m, d_c = _dev(device, sums), _dev(device, m2), _dev(device, count)
    keep = (d_s.clone(), d_m.clone(), d_c.clone())
    ids = torch.full((n + 64,), POISON, dtype=torch.int64, device=d_s.device)
    total = torch.full((3,), POISON, dtype=torch.int64, device=d_s.device)
    adaptive.select_active_device(device, d_s.data_ptr(), d_m.data_ptr(), d_c.data_ptr(), n, spp, threshold, max_spp,
                                  ids.data_ptr(), total[1:].data_ptr())
    torch.cuda.synchronize()
    for t, k in zip((d_s, d_m, d_c), keep):
        assert torch.equal(t.view(torch.int32), k.view(torch.int32)), "the selection wrote its input"
    tot = total.cpu().numpy()
    assert tot[0] == POISON and tot[2] == POISON
    got = ids.cpu().numpy()
    assert (got[n:] == POISON).all(), "the selection wrote past d_ids[n]"
    return got[:n], int(tot[1])


def crafted_state():
    """The estimate's corner cases, one entry each (rtp_adaptive.h, "Noise")."""
    rows = []  # (sx, sy, sz, m2, count)
    for c in (0, 1, 2, -3):
        rows.append((1.0, 2.0, 0.5, 3.0, c))
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(4):
            r = [1.0, 2.0, 0.5, 3.0, 4]
            r[k] = bad
            rows.append(tuple(r))
    # a constant pixel: 8 samples of one colour, accumulated in float32
    c = F([0.3, 0.5, 0.2])
    y = (F(0.2126) * c[0] + F(0.7152) * c[1]) + F(0.0722) * c[2]
    s, m = np.zeros(3, F), F(0)
    for _ in range(8):
        s, m = s + c, m + y * y
    rows.append((s[0], s[1], s[2], m, 8))
    rows.append((0.0, 0.0, 0.0, 0.0, 5))  # black
    # the spread around zero and around the guard 1e-6 * m2: m2 = (Y*Y)/nf + k ulps
    sums = F([1.5, 1.25, 0.75])
    Y = (F(0.2126) * sums[0] + F(0.7152) * sums[1]) + F(0.0722) * sums[2]
    q = (Y * Y) / F(4)
    m = q
    for _ in range(3):
        m = np.nextafter(m, F(-np.inf))
    for _ in range(24):  # k = -3 .. 20: negative, zero, below and above the guard (13.5 ulps)
        rows.append((sums[0], sums[1], sums[2], m, 4))
        m = np.nextafter(m, F(np.inf))
    rows.append((-1.0, -2.0, -0.5, 30.0, 4))  # mean < 0, sem > 0
    rows.append((0.0, 0.0, 0.0, 1.0, 3))  # mean = 0, sem > 0
    rows.append((3.0e38, 3.0e38, 3.0e38, 1.0, 4))  # Y overflows
    rows.append((1e-30, 1e-30, 1e-30, 1e-44, 2))  # denormal m2
    a = np.array(rows, dtype=np.float64)
    sums4 = np.zeros((len(rows), 4), dtype=F)
    sums4[:, :3] = a[:, :3].astype(F)
    return sums4, a[:, 3].astype(F), a[:, 4].astype(np.int32)


def random_state(n, seed):
    """A finite state of plausible magnitudes."""
    rng = np.random.default_rng(seed)
    count = rng.integers(2, 40, n).astype(np.int32)
    sums = np.zeros((n, 4), dtype=F)
    sums[:, :3] = (rng.uniform(0, 2, (n, 3)) * count[:, None]).astype(F)
    m2 = (rng.uniform(0.5, 6, n) * count).astype(F)
    return sums, m2, count


_rendered = {}


def rendered_state(device):
    """The 48 x 40 variant-0 canvas after 4 spp at depth 8 (host arrays, cached)."""
    import raytracingtherestofyourlife_amd as rtp

    if not _rendered:
        device.set_cornell_box(0)
        r = rtp.ProgressiveRender(device, rtp.default_camera(), 48, 40, DEPTH)
        r.step(4)
        _rendered.update(r.state())
        for a in _rendered.values():
            a.setflags(write=False)
    return _rendered


def test_gpu_noise_bits_crafted(device):
    sums, m2, count = crafted_state()
    want = noise_ref(sums, m2, count)
    got = run_noise(device, sums, m2, count)
    ok = same_bits_or_both_nan(got, want)
    assert ok.all(), (np.flatnonzero(~ok).tolist(), got[~ok], want[~ok])
    # the cases are what they claim to be
    assert np.isinf(want[[0, 1, 3]]).all() and np.isfinite(want[2]) and want[2] > 0 and np.isinf(want[4:16]).all()
    assert want[16] == 0 and want[17] == 0
    guard = want[18:42]
    assert (guard[:4] == 0).all() and (guard[-4:] > 0).all() and np.isfinite(guard).all()
    assert 4 < int((guard == 0).sum()) < 20  # the guard switches inside the run
    assert np.isinf(want[42]) and np.isinf(want[43])


def test_gpu_noise_bits_rendered_and_sizes(device):
    s = rendered_state(device)
    got = run_noise(device, s["sums"], s["m2"], s["count"])
    want = noise_ref(s["sums"], s["m2"], s["count"])
    ok = same_bits_or_both_nan(got, want)
    assert ok.all(), (np.flatnonzero(~ok)[:8].tolist(), got[~ok][:4], want[~ok][:4])
    assert np.isfinite(want).sum() > 0.8 * want.size and (want > 0).sum() > 0.5 * want.size
    # every size at which the launch's last block changes
    cs, cm, cc = crafted_state()
    rs, rm, rc = random_state(2 * B + 1, 11)
    rs[: cc.size], rm[: cc.size], rc[: cc.size] = cs, cm, cc
    rs[100:2020], rm[100:2020], rc[100:2020] = s["sums"], s["m2"], s["count"]
    full = noise_ref(rs, rm, rc)
    for n in (1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1):
        got = run_noise(device, rs[:n], rm[:n], rc[:n])
        assert same_bits_or_both_nan(got, full[:n]).all(), n


def _pattern_state(n, active, seed=5):
    """A random finite state whose predicate is `active`, driven through the
    count: a one-sample entry is always noisy enough, a full one never fits."""
    sums, m2, _ = random_state(n, seed)
    count = np.where(active, 1, 100).astype(np.int32)
    return sums, m2, count


def _runs(n):
    a = np.zeros(n, dtype=bool)
    for lo, hi in ((60, 70), (250, 262), (B - 8, B + 12), (2 * B - 1, 2 * B + 1), (3 * B + 60, n)):
        a[lo:hi] = True
    return a


N_SEL = 3 * B + 77
PATTERNS = {
    "all": lambda n: np.ones(n, dtype=bool),
    "none": lambda n: np.zeros(n, dtype=bool),
    "alternating": lambda n: np.arange(n) % 2 == 1,
    "last": lambda n: np.arange(n) == n - 1,
    "first": lambda n: np.arange(n) == 0,
    "runs": _runs,
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_gpu_select_patterns(device, pattern):
    active = PATTERNS[pattern](N_SEL)
    sums, m2, count = _pattern_state(N_SEL, active)
    spp, max_spp = 4, 50
    ref = active_ref(sums, m2, count, spp, 0.0, max_spp)
    assert np.array_equal(ref, active)  # the restatement sees the pattern
    want = np.flatnonzero(ref)
    ids, total = run_select(device, sums, m2, count, spp, 0.0, max_spp)
    assert total == want.size
    assert np.array_equal(ids[:total], want)
    assert (ids[total:] == POISON).all()


def test_gpu_select_small_sizes_and_noise_rule(device):
    """Sizes around a wave and a block, the predicate through the noise
    threshold (the rendered state) and through max_spp < spp."""
    s = rendered_state(device)
    for n in (1, 63, 64, 65, 1920):
        sums, m2, count = s["sums"][:n], s["m2"][:n], s["count"][:n]
        for thr, spp, max_spp in ((THRESHOLD, 4, 16), (0.0, 4, 16), (THRESHOLD, 4, 7), (0.0, 8, 7)):
            want = np.flatnonzero(active_ref(sums, m2, count, spp, thr, max_spp))
            ids, total = run_select(device, sums, m2, count, spp, thr, max_spp)
            assert total == want.size and np.array_equal(ids[:total], want), (n, thr, spp, max_spp)
            assert (ids[total:] == POISON).all()
    want = np.flatnonzero(active_ref(s["sums"], s["m2"], s["count"], 4, THRESHOLD, 16))
    assert 0.05 * 1920 < want.size < 0.95 * 1920


def test_gpu_select_more_blocks_than_scan_threads(device):
    from raytracingtherestofyourlife_amd import adaptive

    n = (1 << 21) + 77
    assert (n + B - 1) // B > 4 * adaptive.SCAN_THREADS  # the scan loops over five chunks
    rng = np.random.default_rng(9)
    active = rng.uniform(size=n) < 0.3
    active[-1] = active[12345] = True
    active[B * 700: B * 702] = False  # two empty blocks
    active[B * 900: B * 901] = True  # a full one
    sums, m2, count = _pattern_state(n, active, seed=6)
    sums[12345, 0], m2[B * 900 + 5] = np.nan, np.inf  # never active, whatever their count
    want = np.flatnonzero(active_ref(sums, m2, count, 4, 0.0, 50))
    assert want.size == active.sum() - 2
    ids, total = run_select(device, sums, m2, count, 4, 0.0, 50)
    assert total == want.size
    assert np.array_equal(ids[:total], want)
    assert (ids[total:] == POISON).all()


def _refine_round(device, a, b, spp, max_spp, what):
    """One round of `a.step(active = the restatement's list)` against
    b.refine_device; returns the share of the canvas selected."""
    s = b.state()
    ids = np.flatnonzero(active_ref(s["sums"], s["m2"], s["count"], spp, THRESHOLD, max_spp)).astype(np.int64)
    share = ids.size / s["count"].size
    print(f"{what}: selects {ids.size} of {s['count'].size} ({share:.3f}); median noise "
          f"{np.median(noise_ref(s['sums'], s['m2'], s['count'])):.4f}")
    assert 0.05 < share < 0.95, what
    a.step(spp, active=ids)
    got = b.refine_device(spp, THRESHOLD, max_spp)
    assert got == ids.size, what
    sa, sb = a.state(), b.state()
    _states_equal(sa, sb, what)
    rest = np.ones(s["count"].size, dtype=bool)
    rest[ids] = False
    for k in s:
        assert _bits_equal(sb[k][rest], s[k][rest]), f"{what}: unselected {k} changed"
    assert np.array_equal(sb["count"][ids], s["count"][ids] + spp)
    return share


def _count_groups_equal_render_pixels(device, r, what):
    s = r.state()
    for c in np.unique(s["count"]):
        pix = np.flatnonzero(s["count"] == c).astype(np.int64)
        want = device.render_pixels(r.camera, r.nx, r.ny, int(c), r.depth, pix)[:3]
        assert_render_equal((s["sums"][pix], s["seed"][pix], s["live"][pix]), want, f"{what}: count {c}")


def test_gpu_refine_pass_equals_its_parts(device):
    import raytracingtherestofyourlife_amd as rtp

    device.set_cornell_box(0)
    cam = rtp.default_camera()
    a = rtp.ProgressiveRender(device, cam, 64, 48, DEPTH)
    b = rtp.ProgressiveRender(device, cam, 64, 48, DEPTH)
    a.step(4)
    b.step(4)
    for rnd in range(3):
        _refine_round(device, a, b, 4, 16, f"round {rnd}")
    assert len(np.unique(b.state()["count"])) >= 3
    _count_groups_equal_render_pixels(device, b, "after three rounds")


def test_gpu_converge(device):
    import torch

    import raytracingtherestofyourlife_amd as rtp

    device.set_cornell_box(0)
    r = rtp.ProgressiveRender(device, rtp.default_camera(), 48, 40, DEPTH)
    r.step(2)
    r.sums[5, 0] = float("nan")
    r.m2[7] = float("inf")
    torch.cuda.synchronize()
    one = rtp.ProgressiveRender(device, rtp.default_camera(), 48, 40, DEPTH)
    one.step(2)
    assert len(one.converge(2, THRESHOLD, 8, 1)) == 1  # max_passes is kept
    per_pass = r.converge(2, THRESHOLD, 8, 8)
    assert 2 <= len(per_pass) <= 8 and per_pass[-1] == 0 and all(v > 0 for v in per_pass[:-1]), per_pass
    assert per_pass == sorted(per_pass, reverse=True)  # an unselected pixel's state, hence its noise, stays
    s = r.state()
    assert s["count"].max() <= 8 and s["count"].min() == 2 and (s["count"] % 2 == 0).all()
    assert s["count"][5] == 2 and s["count"][7] == 2  # a non-finite state is never selected
    assert int(((s["count"] - 2) // 2).sum()) == sum(per_pass)
    assert r.refine_device(2, THRESHOLD, 8) == 0
    # what is left is below the threshold, full, or not finite
    left = active_ref(s["sums"], s["m2"], s["count"], 2, THRESHOLD, 8)
    assert not left.any()
    nd = r.noise_device().cpu().numpy()
    assert same_bits_or_both_nan(nd, noise_ref(s["sums"], s["m2"], s["count"])).all()


def test_gpu_refine_stream_order(device):
    """step and refine_device queued on a non-default stream with no host
    synchronisation between them equal the synchronised sequence."""
    import torch

    import raytracingtherestofyourlife_amd as rtp

    device.set_cornell_box(0)
    cam = rtp.default_camera()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        q = rtp.ProgressiveRender(device, cam, 48, 40, DEPTH)
        q.step(2)
        n_q = q.refine_device(2, THRESHOLD, 8)
        q.step(1)
    stream.synchronize()
    torch.cuda.synchronize()
    w = rtp.ProgressiveRender(device, cam, 48, 40, DEPTH)
    w.step(2)
    torch.cuda.synchronize()
    n_w = w.refine_device(2, THRESHOLD, 8)
    torch.cuda.synchronize()
    w.step(1)
    torch.cuda.synchronize()
    assert n_q == n_w and 0 < n_q < 1920
    _states_equal(q.state(), w.state(), "queued against synchronised")


def test_gpu_refine_sphere_bvh(device):
    import raytracingtherestofyourlife_amd as rtp

    device.set_cornell_box(3)
    try:
        assert device.sphere_walk() == "global"
        cam = rtp.default_camera()
        a = rtp.ProgressiveRender(device, cam, 32, 32, DEPTH)
        b = rtp.ProgressiveRender(device, cam, 32, 32, DEPTH)
        a.step(4)
        b.step(4)
        _refine_round(device, a, b, 4, 16, "sphere BVH")
        _count_groups_equal_render_pixels(device, b, "sphere BVH")
    finally:
        device.set_cornell_box(0)


def test_gpu_refine_host_variant(device):
    import raytracingtherestofyourlife_amd as rtp
    from raytracingtherestofyourlife_amd import adaptive

    device.set_cornell_box(0)
    cam = rtp.default_camera()
    r = rtp.ProgressiveRender(device, cam, 48, 40, DEPTH)
    r.step(4)
    h = {k: np.array(v, copy=True) for k, v in r.state().items()}
    before = {k: v.copy() for k, v in h.items()}
    for with_live in (True, False):
        hh = {k: v.copy() for k, v in before.items()}
        n_h = adaptive.refine(device, cam, 48, 40, DEPTH, hh["sums"], hh["seed"], hh["m2"], hh["count"], 4, THRESHOLD,
                              16, live=hh["live"] if with_live else None)
        if with_live:
            h = hh
        else:
            assert _bits_equal(hh["live"], before["live"])
            for k in ("sums", "seed", "m2", "count"):
                assert _bits_equal(hh[k], h[k]), k
    n_d = r.refine_device(4, THRESHOLD, 16)
    assert n_h == n_d and 0.05 * 1920 < n_d < 0.95 * 1920
    _states_equal(h, r.state(), "rtp_refine against rtp_refine_device")
    # nothing selected: the arrays keep their bits
    hh = {k: v.copy() for k, v in h.items()}
    assert adaptive.refine(device, cam, 48, 40, DEPTH, hh["sums"], hh["seed"], hh["m2"], hh["count"], 4, 1e30, 16,
                           live=hh["live"]) == 0
    _states_equal(hh, h, "a pass that selects nothing")
    # the host noise entry too
    got = adaptive.noise(device, h["sums"], h["m2"], h["count"])
    assert same_bits_or_both_nan(got, noise_ref(h["sums"], h["m2"], h["count"])).all()


def test_gpu_refine_refusals(device, monkeypatch):
    import torch

    import raytracingtherestofyourlife_amd as rtp
    from raytracingtherestofyourlife_amd import _lib, adaptive

    device.set_cornell_box(0)
    L = device._L
    nx, ny = 16, 8
    n = nx * ny
    td = torch.device("cuda", device.device)
    # a state every entry of which a pass would select and rewrite
    sums = torch.full((n, 4), 1.5, dtype=torch.float32, device=td)
    seed = torch.arange(n, dtype=torch.int32, device=td)
    live = torch.full((n,), 3, dtype=torch.int32, device=td)
    m2 = torch.full((n,), 2.5, dtype=torch.float32, device=td)
    count = torch.ones(n, dtype=torch.int32, device=td)
    tensors = (sums, seed, live, m2, count)
    keep = [t.clone() for t in tensors]
    cam = rtp.default_camera().to_c()
    P = lambda t: t.data_ptr()

    def call(entry="rtp_refine_device", cam=cam, nx=nx, ny=ny, depth=DEPTH, state="ok", rgba=P(sums), seed_p=P(seed),
             m2_p=P(m2), count_p=P(count), spp=4, threshold=0.0, max_spp=16, params="ok", out="ok", handle=None):
        st = _lib.render_state(rgba, seed_p, P(live), m2_p) if state == "ok" else None
        prm = adaptive.refine_params(spp, threshold, max_spp) if params == "ok" else None
        total = ctypes.c_int64(-77)
        status = L.rtp_refine_device(handle or device.handle, cam, nx, ny, depth, st, count_p, prm,
                                     total if out == "ok" else None, 0, None)
        return status, total.value

    bad_cam = rtp.default_camera().to_c()
    bad_cam.fov_y_deg = 0.0
    wide_cam = rtp.default_camera().to_c()
    wide_cam.fov_y_deg = 181.0
    bad_calls = [dict(state=None), dict(rgba=0), dict(seed_p=0), dict(m2_p=0), dict(count_p=0), dict(params=None),
                 dict(out=None), dict(spp=0), dict(spp=-1), dict(spp=8388608), dict(max_spp=0), dict(max_spp=-5),
                 dict(threshold=float("nan")), dict(threshold=-0.5), dict(cam=None), dict(cam=bad_cam),
                 dict(cam=wide_cam), dict(nx=0), dict(ny=-1), dict(nx=1 << 16, ny=1 << 16), dict(depth=0),
                 dict(depth=-2)]
    for change in bad_calls:
        status, total = call(**change)
        assert status == _lib.RTP_ERR_INVALID_ARGUMENT and total == -77, change
    for var in ("RTP_KERNEL", "RTP_DEBUG_STATS"):
        monkeypatch.setenv(var, "1")
        status, total = call()
        monkeypatch.delenv(var)
        assert status == _lib.RTP_ERR_INVALID_ARGUMENT and total == -77, var
    # the host variant and the loop share the checks
    h = [t.cpu().numpy() for t in tensors]
    total = ctypes.c_int64(-77)
    st = _lib.render_state(h[0], h[1].view(np.uint32), h[2].view(np.uint32), h[3])
    assert L.rtp_refine(device.handle, cam, nx, ny, DEPTH, st, _lib.ptr(h[4]), adaptive.refine_params(0, 0.0, 16),
                        total, None) == _lib.RTP_ERR_INVALID_ARGUMENT
    per_pass = np.full(4, -77, dtype=np.int64)
    run = ctypes.c_int32(-77)
    dst = _lib.render_state(P(sums), P(seed), P(live), P(m2))
    for prm, passes in ((adaptive.refine_params(4, 0.0, 0), 4), (adaptive.refine_params(4, 0.0, 16), 0)):
        assert L.rtp_render_adaptive_device(device.handle, cam, nx, ny, DEPTH, dst, P(count), prm, passes,
                                            _lib.ptr(per_pass), run, 0, None) == _lib.RTP_ERR_INVALID_ARGUMENT
    assert total.value == -77 and run.value == -77 and (per_pass == -77).all()
    # noise and selection: NULL pointers, bad sizes, bad params
    out = torch.full((n,), 7.0, dtype=torch.float32, device=td)
    ids = torch.full((n,), POISON, dtype=torch.int64, device=td)
    tot = torch.full((1,), POISON, dtype=torch.int64, device=td)
    for args in ((0, P(m2), P(count), n, P(out)), (P(sums), 0, P(count), n, P(out)), (P(sums), P(m2), 0, n, P(out)),
                 (P(sums), P(m2), P(count), 0, P(out)), (P(sums), P(m2), P(count), n, 0)):
        assert L.rtp_noise_device(device.handle, *args, 0, None) == _lib.RTP_ERR_INVALID_ARGUMENT
    good = adaptive.refine_params(4, 0.0, 16)
    for args in ((0, P(m2), P(count), n, good, P(ids), P(tot)), (P(sums), P(m2), P(count), n, None, P(ids), P(tot)),
                 (P(sums), P(m2), P(count), n, good, 0, P(tot)), (P(sums), P(m2), P(count), n, good, P(ids), 0),
                 (P(sums), P(m2), P(count), -1, good, P(ids), P(tot)),
                 (P(sums), P(m2), P(count), n, adaptive.refine_params(4, float("nan"), 16), P(ids), P(tot))):
        assert L.rtp_select_active_device(device.handle, *args, 0, None) == _lib.RTP_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    for t, k in zip(tensors, keep):
        assert torch.equal(t, k), "a rejected call wrote the state"
    assert bool((out == 7.0).all()) and bool((ids == POISON).all()) and bool((tot == POISON).all())
    # without a scene
    fresh = rtp.Device(device.device)
    try:
        status, total = call(handle=fresh.handle)
        assert status == _lib.RTP_ERR_NO_SCENE and total == -77
    finally:
        fresh.close()
    torch.cuda.synchronize()
    for t, k in zip(tensors, keep):
        assert torch.equal(t, k)
    # the good call runs: every entry is selected and rewritten
    status, total = call()
    torch.cuda.synchronize()
    assert status == _lib.RTP_OK and total == n
    assert bool((count == 5).all()) and not torch.equal(seed, keep[1])
