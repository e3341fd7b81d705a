"""Adaptive sampling without a GPU: include/rtp_adaptive.h against librtp.so's
exports (tests/test_abi.py holds its rows of the ctypes table to it); the
float32 restatement of the noise estimate and the selection
(tests/_adaptive_ref.py) against the package's float64 rule
(progressive.noise_from_state, select_active); rtp_normalize_counts against
ProgressiveRender.image()'s arithmetic."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _adaptive_ref import F, active_ref, finite_ref, noise_ref, spread_ref
from _abi import prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "include/rtp_adaptive.h"
EPS = 2.0 ** -24


def test_library_exports_the_adaptive_symbols_and_rtp_h_is_unchanged():
    import raytracingtherestofyourlife_amd as rtp
    from raytracingtherestofyourlife_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", rtp.LIB_PATH], capture_output=True, text=True).stdout
    adaptive = prototypes(HEADER)
    assert list(adaptive) == list(_lib.SIGNATURES[HEADER])
    for n in adaptive:
        assert re.search(rf"\bT {n}$", out, flags=re.M), n
    assert len(prototypes("include/rtp.h")) == 40  # include/rtp.h keeps its prototypes ...
    assert not set(adaptive) & set(_lib.SIGNATURES["include/rtp.h"])  # ... and _lib its group of them
    assert not set(adaptive) & set(_lib.EXPORTED_SYMBOLS)
    assert '#include "rtp.h"' in open(os.path.join(ROOT, HEADER)).read()


def test_progressive_render_has_the_device_methods():
    import raytracingtherestofyourlife_amd as rtp

    for m in ("noise_device", "refine_device", "converge", "refine", "noise", "step", "image"):
        assert callable(getattr(rtp.ProgressiveRender, m)), m
    for f in ("noise_device", "noise", "select_active_device", "refine_device", "refine", "render_adaptive_device",
              "normalize_counts"):
        assert callable(getattr(rtp.adaptive, f)), f


def test_python_geometry_constants_are_the_kernels():
    """adaptive.SELECT_BLOCK / SCAN_THREADS, which size the boundary cases of
    tests/test_gpu_adaptive.py, against csrc/rtp_adaptive.hpp."""
    from raytracingtherestofyourlife_amd import adaptive

    hpp = open(os.path.join(os.path.dirname(adaptive.__file__), "csrc", "rtp_adaptive.hpp")).read()
    val = lambda name: int(re.search(rf"\b{name} = (\d+)\b", hpp).group(1))
    assert re.search(r"\bkSelBlock = kSelThreads \* kSelRounds\b", hpp)
    assert adaptive.SELECT_BLOCK == val("kSelThreads") * val("kSelRounds")
    assert adaptive.SCAN_THREADS == val("kScanThreads")


# --------------------------------------------------------------------------
_state = {}


def synthetic_state():
    """8192 pixels with counts 1..64, accumulated sample by sample in float32
    as the kernel does (sums += c; m2 += y*y): 20 % of the pixels repeat one
    colour (constant luminance), 5 % of the samples have radiance 15 (a light
    hit), 10 % are black; then a NaN sum, an inf m2 and a zero count."""
    if _state:
        return _state
    rng = np.random.default_rng(20240)
    n, kmax = 8192, 64
    count = rng.integers(1, kmax + 1, n).astype(np.int32)
    const = rng.uniform(size=n) < 0.20
    base = rng.uniform(0.05, 1.0, (n, 3)).astype(F)
    sums = np.zeros((n, 4), dtype=F)
    m2 = np.zeros(n, dtype=F)
    for k in range(kmax):
        c = rng.uniform(0.0, 1.0, (n, 3)).astype(F)
        u = rng.uniform(size=n)
        c[u < 0.05] = F(15)
        c[(u >= 0.05) & (u < 0.15)] = F(0)
        c[const] = base[const]
        on = k < count
        y = (F(0.2126) * c[:, 0] + F(0.7152) * c[:, 1]) + F(0.0722) * c[:, 2]
        sums[on, :3] = sums[on, :3] + c[on]
        m2[on] = m2[on] + y[on] * y[on]
    sums[100, 1] = np.nan
    m2[101] = np.inf
    count[102] = 0
    for a in (sums, m2, count):
        a.setflags(write=False)
    _state.update(sums=sums, m2=m2, count=count)
    return _state


def _bound(s, n64):
    """|n32 - n64| allowed: the cancellation in m2 - Y*Y/n amplifies the
    roundings of Y*Y/n and of the difference (each 2^-24 relative to about m2)
    by m2 / spread; the remaining operations (luma, two divisions, sqrt, the
    final division) add a few 2^-24 each: n64 * 2^-24 * (4 * m2 / spread + 8)."""
    with np.errstate(all="ignore"):
        amp = s["m2"].astype(np.float64) / spread_ref(s["sums"], s["m2"], s["count"]).astype(np.float64)
        return n64 * EPS * (4 * amp + 8)


def test_noise_ref_against_the_float64_rule():
    from raytracingtherestofyourlife_amd.progressive import noise_from_state

    s = synthetic_state()
    n32 = noise_ref(s["sums"], s["m2"], s["count"])
    n64 = noise_from_state(s["sums"], s["m2"], s["count"])
    assert n32.dtype == F and n32.shape == (8192,)
    inf32, inf64 = np.isinf(n32), np.isinf(n64)
    assert np.array_equal(inf32, inf64)
    assert inf32[[100, 101, 102]].all() and inf32[s["count"] < 2].all()
    # zeros: both, except where the float64 spread sits on the guard
    m2 = s["m2"].astype(np.float64)
    k = s["count"].astype(np.float64)
    with np.errstate(all="ignore"):
        Y = 0.2126 * s["sums"][:, 0].astype(np.float64) + 0.7152 * s["sums"][:, 1] + 0.0722 * s["sums"][:, 2]
        spread64 = m2 - Y * Y / k
        on_guard = np.abs(spread64 - 1e-6 * m2) <= 4 * EPS * m2
    z32, z64 = n32 == 0, n64 == 0
    differ = (z32 != z64) & ~inf32
    assert not (differ & ~on_guard).any(), np.flatnonzero(differ & ~on_guard)[:8]
    assert z32.sum() >= 0.15 * 8192  # the constant pixels (and nothing hides here)
    rest = ~inf32 & ~z32 & ~z64
    assert rest.sum() > 0.7 * 8192
    with np.errstate(invalid="ignore"):
        err = np.abs(n32.astype(np.float64) - n64)[rest]
    lim = _bound(s, n64)[rest]
    worst = float((err / lim).max())
    print(f"noise_ref vs float64: {rest.sum()} entries, worst error / bound = {worst:.3f}")
    assert (err <= lim).all(), (worst, np.flatnonzero(rest)[err > lim][:8])


@pytest.mark.parametrize("threshold", [0.05, 0.1, 0.2])
def test_active_ref_against_select_active(threshold):
    from raytracingtherestofyourlife_amd.progressive import noise_from_state, select_active, state_finite

    s = synthetic_state()
    spp, max_spp = 4, 48
    n64 = noise_from_state(s["sums"], s["m2"], s["count"])
    want = np.zeros(8192, dtype=bool)
    want[select_active(n64, s["count"], spp, threshold, max_spp, finite=state_finite(s["sums"], s["m2"]))] = True
    got = active_ref(s["sums"], s["m2"], s["count"], spp, threshold, max_spp)
    assert 0.05 * 8192 < got.sum() < 0.95 * 8192
    with np.errstate(all="ignore"):
        near = np.abs(n64 - threshold) <= _bound(s, n64)
    near &= np.isfinite(n64)
    differ = got != want
    print(f"threshold {threshold}: {got.sum()} active, {differ.sum()} differ, {near.sum()} within the bound")
    assert near.sum() <= 0.005 * 8192
    assert not (differ & ~near).any(), np.flatnonzero(differ & ~near)[:8]
    # the count rule, exactly: nothing with count + spp > max_spp, nothing at all when max_spp < spp
    assert not got[s["count"].astype(np.int64) + spp > max_spp].any()
    assert not active_ref(s["sums"], s["m2"], s["count"], 8, 0.0, 7).any()
    assert not got[~finite_ref(s["sums"], s["m2"])].any()
    assert got[(s["count"] == 1) & finite_ref(s["sums"], s["m2"])].all()


def test_normalize_counts_is_image_arithmetic():
    import raytracingtherestofyourlife_amd as rtp

    rng = np.random.default_rng(3)
    n = 4000
    sums = (rng.random((n, 4), dtype=np.float32) * 50).astype(F)
    sums[:, 3] = 0
    sums[::7, 1] = np.nan
    sums[::11, 0] = np.inf
    count = rng.integers(1, 300, n).astype(np.int32)
    count[5] = 0
    keep = sums.copy()
    got = rtp.normalize_counts(sums, count)
    assert np.array_equal(sums.view(np.uint32), keep.view(np.uint32)), "the input was written"
    a = sums.copy()  # ProgressiveRender.image()
    rgb = a[:, :3]
    rgb[np.isnan(rgb)] = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.sqrt(a / count.astype(np.float32)[:, None])
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), np.flatnonzero(~same.all(axis=1))[:8]
    # a uniform count: rtp_normalize's bytes
    uni = rtp.normalize_counts(sums, np.full(n, 10, dtype=np.int32))
    ref = rtp.normalize(sums.copy(), 10)
    assert uni.tobytes() == ref.tobytes()
    with pytest.raises(rtp.ErrorBadValue):
        rtp.normalize_counts(sums, count[:-1])
