"""rtp_resolve_device and rtp_denoise_device on synthetic data (no rendering)
against their numpy float32 restatements (tests/_denoise_ref.py), bit for bit,
and the argument checks of the filter.  A mismatch here is a kernel or
compiler-flag problem, never a tolerance to loosen."""
from __future__ import annotations

import numpy as np
import pytest

from _denoise_ref import F, denoise_ref, resolve_ref
from _util import same_bits_or_both_nan

pytestmark = pytest.mark.gpu

PRM = dict(sigma_l=4.0, sigma_z=0.75, sigma_a=0.3)
CANVASES = [(37, 29), (1, 1), (3, 2), (64, 64)]  # 37x29: no multiple of the 64x4 block, taps leave it at steps 8, 16
_inputs = {}


def synth(nx, ny):
    """Random cv, g0, g1 (cached, read-only): ~5 % invalid pixels, a block of
    misses (t = +inf), one valid pixel whose 24 neighbours are all invalid and
    one invalid pixel in a 5x5 block of invalid ones."""
    if (nx, ny) in _inputs:
        return _inputs[(nx, ny)]
    rng = np.random.default_rng(1000 * nx + ny)
    n = nx * ny
    cv = rng.uniform(0, 2, (n, 4)).astype(F)
    cv[:, 3] = rng.uniform(1e-4, 0.5, n).astype(F)
    cv[rng.uniform(size=n) < 0.05] = (0, 0, 0, -1)
    nrm = rng.normal(size=(n, 3))
    g0 = np.concatenate([nrm / np.linalg.norm(nrm, axis=1, keepdims=True), rng.uniform(1, 10, (n, 1))], 1).astype(F)
    # a few shared normals and albedos, so that some neighbours agree
    flat = rng.uniform(size=n) < 0.5
    g0[flat, :3] = F([0, 0, -1])
    pal = rng.uniform(0, 1, (4, 3)).astype(F)
    g1 = np.concatenate([pal[rng.integers(0, 4, n)], np.ones((n, 1), F)], 1).astype(F)
    X, Y = np.meshgrid(np.arange(nx), np.arange(ny))
    X, Y = X.reshape(-1), Y.reshape(-1)
    miss = (X >= nx // 3) & (X < max(2 * nx // 3, 1)) & (Y >= ny // 4) & (Y < max(ny // 2, 1))
    g0[miss] = (0, 0, 0, np.inf)
    g1[miss] = 0
    if nx >= 16 and ny >= 16:
        for cx, cy, centre_valid in ((nx // 2 + 5, ny // 2 + 4, True), (4, ny - 5, False)):
            blk = (abs(X - cx) <= 2) & (abs(Y - cy) <= 2)
            cv[blk] = (0, 0, 0, -1)
            if centre_valid:
                cv[cy * nx + cx] = (0.5, 1.0, 1.5, 0.02)
    for a in (cv, g0, g1):
        a.setflags(write=False)
    _inputs[(nx, ny)] = (cv, g0, g1)
    return _inputs[(nx, ny)]


def run_filter(device, cv, g0, g1, nx, ny, levels, normal_log2, **kw):
    import torch

    td = torch.device("cuda", device.device)
    t = lambda a: torch.from_numpy(np.array(a, copy=True)).to(td)
    d_cv = t(cv)
    keep = d_cv.clone()
    d_g0, d_g1 = (t(g0), t(g1)) if g0 is not None else (None, None)
    out = torch.full((nx * ny, 4), 7.0, dtype=torch.float32, device=td)
    scratch = torch.full((nx * ny, 4), 7.0, dtype=torch.float32, device=td)
    prm = dict(PRM)
    prm.update(kw)
    st = device.denoise_device(d_cv.data_ptr(), nx, ny, out.data_ptr(), scratch.data_ptr(),
                               g0_ptr=d_g0.data_ptr() if d_g0 is not None else 0,
                               g1_ptr=d_g1.data_ptr() if d_g1 is not None else 0, levels=levels,
                               normal_log2=normal_log2, timed=True, **prm)
    assert torch.equal(d_cv, keep), "the input was written"
    assert st.kernel_ms > 0
    return out.cpu().numpy()


@pytest.mark.parametrize("normal_log2", [0, 5])
@pytest.mark.parametrize("guides", [True, False])
@pytest.mark.parametrize("levels", [1, 5])
@pytest.mark.parametrize("nx,ny", CANVASES)
def test_gpu_denoise_equals_restatement(device, nx, ny, levels, guides, normal_log2):
    cv, g0, g1 = synth(nx, ny)
    if not guides:
        g0 = g1 = None
    got = run_filter(device, cv, g0, g1, nx, ny, levels, normal_log2)
    want = denoise_ref(cv, g0, g1, nx, ny, levels, normal_log2=normal_log2, **PRM)
    ok = same_bits_or_both_nan(got, want).all(axis=1)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (f"{bad.size} of {nx * ny} pixels differ, first {bad[:6].tolist()}: got "
                           f"{got[bad[:3]].tolist()} want {want[bad[:3]].tolist()}")
    if nx >= 16 and levels == 1:
        lone = (ny // 2 + 4) * nx + nx // 2 + 5  # only its centre tap counts
        np.testing.assert_allclose(got[lone], cv[lone], rtol=3e-7)
        dead = (ny - 5) * nx + 4  # nothing valid within reach: the input pixel
        assert np.array_equal(got[dead], F([0, 0, 0, -1]))


def test_gpu_denoise_fills_holes_without_spreading(device):
    nx, ny = 37, 29
    cv, g0, g1 = synth(nx, ny)
    got = run_filter(device, cv, None, None, nx, ny, 5, 5)
    assert np.isfinite(got).all() and (got[:, 3] >= 0).all()  # five levels reach over every hole of this canvas


def test_gpu_resolve_equals_restatement(device):
    import torch

    td = torch.device("cuda", device.device)
    rng = np.random.default_rng(5)
    n = 1000
    count = rng.choice(np.array([0, 1, 2, 2, 7, 100], dtype=np.int32), n)
    count[:3] = (0, 1, 2)
    sums = (rng.uniform(0, 3, (n, 4)) * np.maximum(count, 1)[:, None]).astype(F)
    m2 = (rng.uniform(0, 30, n) * np.maximum(count, 1)).astype(F)
    sums[10, 0], sums[11, 1], sums[12, 2], sums[13, 0] = np.nan, np.inf, -np.inf, np.nan
    m2[20], m2[21], m2[13] = np.nan, np.inf, np.nan
    m2[30:40] = 0  # spread < 0: clamped
    sums[40:44, :3] = 3.0e38  # Y*Y overflows
    d_s, d_m, d_c = (torch.from_numpy(a).to(td) for a in (sums, m2, count))
    for with_m2, with_count, spp in ((True, True, 0), (False, True, 0), (True, False, 4), (False, False, 1),
                                     (True, False, 1), (True, False, 0)):
        out = torch.full((n, 4), 7.0, dtype=torch.float32, device=td)
        device.resolve_device(d_s.data_ptr(), n, out.data_ptr(), m2_ptr=d_m.data_ptr() if with_m2 else 0,
                              count_ptr=d_c.data_ptr() if with_count else 0, spp=spp)
        got = out.cpu().numpy()
        want = resolve_ref(sums, m2 if with_m2 else None, count if with_count else None, spp)
        ok = same_bits_or_both_nan(got, want).all(axis=1)
        assert ok.all(), (with_m2, with_count, spp, np.flatnonzero(~ok)[:8].tolist(), got[~ok][:3], want[~ok][:3])
        if with_count:
            assert np.array_equal(got[0], F([0, 0, 0, -1]))
            assert np.array_equal(got[10:13], np.tile(F([0, 0, 0, -1]), (3, 1)))


def test_gpu_denoise_argument_checks(device):
    import torch

    import raytracingtherestofyourlife_amd as rtp

    td = torch.device("cuda", device.device)
    nx, ny = 8, 4
    n = nx * ny
    cv = torch.rand((n, 4), dtype=torch.float32, device=td)
    g0 = torch.rand((n, 4), dtype=torch.float32, device=td)
    g1 = torch.ones((n, 4), dtype=torch.float32, device=td)
    out = torch.full((n, 4), 7.0, dtype=torch.float32, device=td)
    scratch = torch.full((n, 4), 7.0, dtype=torch.float32, device=td)
    big = torch.full((2 * n, 4), 7.0, dtype=torch.float32, device=td)
    P = lambda t: t.data_ptr()
    good = dict(cv_ptr=P(cv), out_ptr=P(out), scratch_ptr=P(scratch), g0_ptr=P(g0), g1_ptr=P(g1), levels=2,
                sigma_l=4.0, sigma_z=1.0, sigma_a=0.1, normal_log2=5)
    bad_calls = [
        dict(out_ptr=P(cv)), dict(scratch_ptr=P(cv)), dict(out_ptr=P(scratch)), dict(out_ptr=P(g0)),
        dict(scratch_ptr=P(g1)),
        dict(out_ptr=P(big), scratch_ptr=P(big) + 16 * (n // 2)),  # a partial overlap
        dict(levels=0), dict(levels=9), dict(sigma_l=0.0), dict(sigma_z=-1.0), dict(sigma_a=0.0),
        dict(sigma_l=float("nan")), dict(normal_log2=-1), dict(normal_log2=9), dict(g0_ptr=0), dict(g1_ptr=0),
        dict(out_ptr=0), dict(scratch_ptr=0), dict(cv_ptr=0),
    ]
    keep = [t.clone() for t in (cv, g0, g1)]
    for change in bad_calls:
        kw = dict(good)
        kw.update(change)
        with pytest.raises(rtp.RtpError) as e:
            device.denoise_device(kw.pop("cv_ptr"), nx, ny, kw.pop("out_ptr"), kw.pop("scratch_ptr"), **kw)
        assert e.value.status == rtp._lib.RTP_ERR_INVALID_ARGUMENT, change
    for bad_size in ((0, 4), (8, -1)):
        with pytest.raises(rtp.RtpError) as e:
            device.denoise_device(P(cv), bad_size[0], bad_size[1], P(out), P(scratch))
        assert e.value.status == rtp._lib.RTP_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize(td)
    for t in (out, scratch, big):
        assert bool((t == 7.0).all()), "a rejected call wrote an output"
    for t, k in zip((cv, g0, g1), keep):
        assert torch.equal(t, k)
    device.denoise_device(P(cv), nx, ny, P(out), P(scratch), g0_ptr=P(g0), g1_ptr=P(g1), levels=2)  # the good call runs
    torch.cuda.synchronize(td)
    assert not bool((out == 7.0).any())
