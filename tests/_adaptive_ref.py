"""numpy float32 restatements of rtp_noise_device and of the selection rule of
rtp_select_active_device (include/rtp_adaptive.h states both operation by
operation).  Every step is one whole-array float32 operation, so the order of
operations is the definition's and the kernels must reproduce these bits."""
from __future__ import annotations

import numpy as np

F = np.float32
LR, LG, LB = F(0.2126), F(0.7152), F(0.0722)
GUARD = F(1e-6)


def finite_ref(sums, m2) -> np.ndarray:
    sums = np.asarray(sums, dtype=F)
    return np.isfinite(sums[:, :3]).all(axis=1) & np.isfinite(np.asarray(m2, dtype=F))


def spread_ref(sums, m2, count) -> np.ndarray:
    """The float32 spread m2 - (Y*Y)/nf of every entry (whatever its state)."""
    sums, m2 = np.asarray(sums, dtype=F), np.asarray(m2, dtype=F)
    with np.errstate(all="ignore"):
        nf = np.asarray(count, dtype=np.int32).astype(F)
        Y = (LR * sums[:, 0] + LG * sums[:, 1]) + LB * sums[:, 2]
        return m2 - (Y * Y) / nf


def noise_ref(sums, m2, count) -> np.ndarray:
    """sums float32 [n, >=3], m2 float32 [n], count int32 [n] -> float32 [n]."""
    sums, m2 = np.asarray(sums, dtype=F), np.asarray(m2, dtype=F)
    cnt = np.asarray(count, dtype=np.int32)
    with np.errstate(all="ignore"):
        nf = cnt.astype(F)
        Y = (LR * sums[:, 0] + LG * sums[:, 1]) + LB * sums[:, 2]
        spread = m2 - (Y * Y) / nf
        s2 = np.where(spread <= GUARD * m2, F(0), spread / (nf - F(1)))
        sem = np.sqrt(s2 / nf)
        mean = Y / nf
        noise = np.where(sem == F(0), F(0), np.where(mean > F(0), sem / mean, F(np.inf)))
    out = np.where(finite_ref(sums, m2) & (cnt >= 2), noise, F(np.inf)).astype(F)
    assert out.dtype == F and s2.dtype == F and sem.dtype == F and mean.dtype == F
    return out


def active_ref(sums, m2, count, spp: int, threshold: float, max_spp: int) -> np.ndarray:
    """The selection's predicate, bool [n]: finite, noise > threshold (the
    threshold as float32) and count <= max_spp - spp (nothing when max_spp < spp)."""
    cnt = np.asarray(count, dtype=np.int64)
    room = (int(max_spp) >= int(spp)) & (cnt <= int(max_spp) - int(spp))
    return finite_ref(sums, m2) & (noise_ref(sums, m2, count) > F(threshold)) & room
