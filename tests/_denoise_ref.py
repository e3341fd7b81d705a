"""numpy float32 restatements of rtp_resolve_device and rtp_denoise_device
(include/rtp.h states both operation by operation).  Every step is one
whole-array float32 operation, so the order of operations is the definition's
and the kernels must reproduce these bits."""
from __future__ import annotations

import numpy as np

F = np.float32
H = (F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16))
LR, LG, LB = F(0.2126), F(0.7152), F(0.0722)


def luma(c: np.ndarray) -> np.ndarray:
    return (LR * c[..., 0] + LG * c[..., 1]) + LB * c[..., 2]


def resolve_ref(sums, m2=None, count=None, spp: int = 0) -> np.ndarray:
    """sums float32 [n, 4], m2 float32 [n] or None, count int32 [n] or None
    (then every entry has spp samples) -> cv float32 [n, 4]."""
    sums = np.asarray(sums, dtype=F)
    n = sums.shape[0]
    cnt = np.full(n, spp, dtype=np.int32) if count is None else np.asarray(count, dtype=np.int32)
    ok = (cnt > 0) & np.isfinite(sums[:, :3]).all(axis=1)
    if m2 is not None:
        m2 = np.asarray(m2, dtype=F)
        ok &= np.isfinite(m2)
    out = np.zeros((n, 4), dtype=F)
    out[:, 3] = F(-1)
    with np.errstate(all="ignore"):
        nf = cnt.astype(F)
        Y = luma(sums)
        l = Y / nf
        var = l * l
        if m2 is not None:
            spread = m2 - (Y * Y) / nf
            v2 = (np.where(spread > 0, spread, F(0)) / (nf - F(1))) / nf
            var = np.where(cnt == 1, var, v2)
        rgb = sums[:, :3] / nf[:, None]
    out[ok, :3] = rgb[ok]
    out[ok, 3] = var[ok]
    return out


def atrous_level(cv, g0, g1, nx, ny, step, sigma_l, sigma_z, sigma_a, normal_log2) -> np.ndarray:
    """One level: cv float32 [ny*nx, 4] -> float32 [ny*nx, 4]."""
    c = np.asarray(cv, dtype=F).reshape(ny, nx, 4)
    guides = g0 is not None
    if guides:
        G0 = np.asarray(g0, dtype=F).reshape(ny, nx, 4)
        G1 = np.asarray(g1, dtype=F).reshape(ny, nx, 4)
    sc = np.zeros((ny, nx, 3), dtype=F)
    sv = np.zeros((ny, nx), dtype=F)
    sw = np.zeros((ny, nx), dtype=F)
    valid = ~(c[..., 3] < 0)
    lum = luma(c)
    with np.errstate(all="ignore"):
        lden = F(sigma_l) * np.sqrt(c[..., 3]) + F(1e-4)
        sz_step = F(sigma_z) * F(step)
        sa2 = F(sigma_a) * F(sigma_a)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = step * dx, step * dy
                x0, x1 = max(0, -ox), min(nx, nx - ox)
                y0, y1 = max(0, -oy), min(ny, ny - oy)
                if x0 >= x1 or y0 >= y1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                cq = c[Q]
                vp = valid[P]
                if dx == 0 and dy == 0:
                    ok = vp
                    w = np.full(vp.shape, F(9 / 64), dtype=F)
                else:
                    ok = valid[Q]
                    k = H[dx + 2] * H[dy + 2]
                    w = np.full(vp.shape, k, dtype=F)
                    if guides:
                        hp, hq = G1[P][..., 3] != 0, G1[Q][..., 3] != 0
                        np_, nq = G0[P], G0[Q]
                        m = np.maximum(F(0), (np_[..., 0] * nq[..., 0] + np_[..., 1] * nq[..., 1]) +
                                       np_[..., 2] * nq[..., 2])
                        wn = m
                        for _ in range(normal_log2):
                            wn = wn * wn
                        dz = np.abs(np_[..., 3] - nq[..., 3]) / sz_step
                        wz = F(1) / (F(1) + dz * dz)
                        a = G1[P][..., :3] - G1[Q][..., :3]
                        da = (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]
                        wa = F(1) / (F(1) + da / sa2)
                        wg = ((k * wn) * wz) * wa
                        w = np.where(hp != hq, F(0), np.where(hp, wg, w))
                    dl = np.abs(lum[P] - lum[Q]) / lden[P]
                    wl = F(1) / (F(1) + dl * dl)
                    w = np.where(vp, w * wl, w)
                w = w.astype(F)
                sc[P] = np.where(ok[..., None], sc[P] + w[..., None] * cq[..., :3], sc[P])
                sv[P] = np.where(ok, sv[P] + (w * w) * cq[..., 3], sv[P])
                sw[P] = np.where(ok, sw[P] + w, sw[P])
        out = c.copy()
        good = sw > 0
        res = np.concatenate([sc / sw[..., None], (sv / (sw * sw))[..., None]], axis=-1)
    out[good] = res[good]
    assert out.dtype == F
    return out.reshape(ny * nx, 4)


def denoise_ref(cv, g0, g1, nx, ny, levels, sigma_l, sigma_z, sigma_a, normal_log2) -> np.ndarray:
    cur = np.asarray(cv, dtype=F).reshape(ny * nx, 4)
    for s in range(levels):
        cur = atrous_level(cur, g0, g1, nx, ny, 1 << s, sigma_l, sigma_z, sigma_a, normal_log2)
    return cur
