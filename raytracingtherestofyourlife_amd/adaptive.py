"""Adaptive sampling on the device: the entry points of include/rtp_adaptive.h
as functions of a Device.

Each function is one entry point: its argument checks, its output buffers and
its argument order, like Device's methods, over the same marshalling: _lib's
table (the rows of include/rtp_adaptive.h) and Device._call.  A library
without these symbols (an experiment's RTP_LIB_PATH baseline) still loads;
calling one of them then raises AttributeError.
"""
from __future__ import annotations

import ctypes
from typing import TYPE_CHECKING

import numpy as np

from ._lib import ErrorBadValue, RtpRefineParams, RtpStats, check, load, ptr, render_state

if TYPE_CHECKING:
    from .device import Device
    from .mapper import Camera

SELECT_BLOCK = 2048  # entries per block of the selection (csrc/rtp_adaptive.hpp kSelBlock)
SCAN_THREADS = 256   # block counts the scan takes per chunk (kScanThreads)


def refine_params(spp: int, threshold: float, max_spp: int) -> RtpRefineParams:
    return RtpRefineParams(float(threshold), int(spp), int(max_spp))


def noise_device(dev: "Device", sums_ptr: int, m2_ptr: int, count_ptr: int, n: int, noise_ptr: int, stream: int = 0,
                 timed: bool = False) -> RtpStats:
    """rtp_noise_device: the noise estimate of a device-resident render state
    (sums_ptr float4[n], m2_ptr float[n], count_ptr int32[n]) into noise_ptr
    float[n].  Asynchronous unless timed."""
    return dev._call("rtp_noise_device", sums_ptr, m2_ptr, count_ptr, int(n), noise_ptr, stream, stats=timed)


def noise(dev: "Device", sums: np.ndarray, m2: np.ndarray, count: np.ndarray) -> np.ndarray:
    """rtp_noise on host arrays (sums float32 [n, 4], m2 float32 [n], count
    int32 [n]): float32 [n]."""
    n = sums.shape[0]
    _expect("noise", [(sums, np.float32, (n, 4)), (m2, np.float32, (n,)), (count, np.int32, (n,))])
    out = np.zeros(n, dtype=np.float32)
    dev._call("rtp_noise", ptr(sums), ptr(m2), ptr(count), n, ptr(out))
    return out


def select_active_device(dev: "Device", sums_ptr: int, m2_ptr: int, count_ptr: int, n: int, spp: int,
                         threshold: float, max_spp: int, ids_ptr: int, n_selected_ptr: int, stream: int = 0,
                         timed: bool = False) -> RtpStats:
    """rtp_select_active_device: the active entries' ids, ascending, into
    ids_ptr (device int64[n]) and their number into n_selected_ptr (device
    int64).  Asynchronous unless timed."""
    return dev._call("rtp_select_active_device", sums_ptr, m2_ptr, count_ptr, int(n),
                     refine_params(spp, threshold, max_spp), ids_ptr, n_selected_ptr, stream, stats=timed)


def refine_device(dev: "Device", camera: "Camera", nx: int, ny: int, depth: int, rgba_ptr: int, seed_ptr: int,
                  m2_ptr: int, count_ptr: int, spp: int, threshold: float, max_spp: int, live_ptr: int = 0,
                  stream: int = 0, timed: bool = False):
    """rtp_refine_device: one adaptive pass over a device-resident state of
    the whole canvas and its int32 counts: (entries selected, stats).  Waits
    for the selection's total; the pass's launches are queued, not waited for
    (unless timed)."""
    total = ctypes.c_int64(-1)
    st = dev._call("rtp_refine_device", camera.to_c() if camera is not None else None, nx, ny, depth,
                   render_state(rgba_ptr, seed_ptr, live_ptr, m2_ptr), count_ptr,
                   refine_params(spp, threshold, max_spp), total, stream, stats=timed)
    return int(total.value), st


def refine(dev: "Device", camera: "Camera", nx: int, ny: int, depth: int, rgba: np.ndarray, seed: np.ndarray,
           m2: np.ndarray, count: np.ndarray, spp: int, threshold: float, max_spp: int,
           live: np.ndarray | None = None) -> int:
    """rtp_refine on host arrays, in place (rgba float32 [n, 4], seed uint32
    [n], m2 float32 [n], count int32 [n], live uint32 [n] optional; n = nx *
    ny): the number of entries selected."""
    n = rgba.shape[0]
    want = [(rgba, np.float32, (n, 4)), (seed, np.uint32, (n,)), (m2, np.float32, (n,)), (count, np.int32, (n,))]
    if live is not None:
        want.append((live, np.uint32, (n,)))
    _expect("refine", want)
    if n != int(nx) * int(ny):
        raise ErrorBadValue(f"refine: a state of {n} entries for a {nx} x {ny} canvas")
    total = ctypes.c_int64(-1)
    dev._call("rtp_refine", camera.to_c(), nx, ny, depth, render_state(rgba, seed, live, m2), ptr(count),
              refine_params(spp, threshold, max_spp), total)
    return int(total.value)


def render_adaptive_device(dev: "Device", camera: "Camera", nx: int, ny: int, depth: int, rgba_ptr: int,
                           seed_ptr: int, m2_ptr: int, count_ptr: int, spp: int, threshold: float, max_spp: int,
                           max_passes: int, live_ptr: int = 0, stream: int = 0) -> list:
    """rtp_render_adaptive_device: passes until one selects nothing or
    max_passes have run; what each selected (a final 0 included)."""
    if int(max_passes) < 1:
        raise ErrorBadValue("render_adaptive_device: max_passes must be >= 1")
    per_pass = np.full(int(max_passes), -1, dtype=np.int64)
    run = ctypes.c_int32(0)
    dev._call("rtp_render_adaptive_device", camera.to_c(), nx, ny, depth,
              render_state(rgba_ptr, seed_ptr, live_ptr, m2_ptr), count_ptr, refine_params(spp, threshold, max_spp),
              int(max_passes), ptr(per_pass), run, stream, stats=False)
    return [int(v) for v in per_pass[: run.value]]


def refine_last_timing(dev: "Device") -> dict:
    """The device times (ms) of the parts of the last timed refine_device."""
    ms = (ctypes.c_double * 4)()
    check(dev._L.rtp_refine_last_timing(dev.handle, ms))
    return dict(select=ms[0], gather=ms[1], resume=ms[2], scatter=ms[3])


def normalize_counts(rgba_sum: np.ndarray, count: np.ndarray) -> np.ndarray:
    """rtp_normalize_counts: rtp_normalize with each pixel's own count (no
    device needed): a float32 [n, 4] copy."""
    a = np.array(rgba_sum, dtype=np.float32, order="C", copy=True).reshape(-1, 4)
    c = np.ascontiguousarray(count, dtype=np.int32).reshape(-1)
    if c.size != a.shape[0]:
        raise ErrorBadValue(f"normalize_counts: {c.size} counts for {a.shape[0]} pixels")
    check(load().rtp_normalize_counts(ptr(a), ptr(c), a.shape[0]))
    return a


def _expect(who: str, want) -> None:
    for a, dt, shape in want:
        if not (isinstance(a, np.ndarray) and a.flags.c_contiguous and a.dtype == dt and a.shape == shape):
            raise ErrorBadValue(f"{who}: expects C-contiguous {np.dtype(dt).name} arrays of shape {shape}")
