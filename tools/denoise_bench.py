"""What a denoised preview costs on the device (development tool): the first-hit
guides, the resolve and each level of the a-trous filter (include/rtp.h
rtp_denoise_device) timed with device events, beside the same filter written
with plain torch tensors -- shifted slices and elementwise ops, what a user
would write without the kernel.

    python tools/denoise_bench.py [--nx 800 --ny 800 --levels 5 --reps 15 --inner 50] [--spp 8]

The state is a real render (--spp samples of the Cornell box, depth 50).  A
window is --inner back-to-back calls between two events on the torch stream;
the sides alternate inside one process after a warm-up of each, and the report
is the median (min, max) over --reps windows, per call.  The library runs its
L levels in one call, so level s is reported as the difference of the medians
of the (s+1)-level and the s-level call; the torch side times each level on
its own.  bytes/s is the level's minimum traffic, n x (48 B read + 16 B
write), over its time.  The torch result is compared with the kernel's.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import raytracingtherestofyourlife_amd as rtp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nx", type=int, default=800)
ap.add_argument("--ny", type=int, default=800)
ap.add_argument("--levels", type=int, default=5)
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--depth", type=int, default=50)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--inner", type=int, default=50)
a = ap.parse_args()
if a.reps < 10:
    ap.error("--reps must be at least 10")

nx, ny, n, L = a.nx, a.ny, a.nx * a.ny, a.levels
dev = rtp.Device(0)
dev.set_cornell_box(0)
dev.set_ff_tables("off")
r = rtp.ProgressiveRender(dev, rtp.default_camera(), nx, ny, a.depth)
r.step(a.spp)
g = r.guides()
prm = dict(sigma_l=rtp.progressive.DENOISE_SIGMA_L, sigma_z=r.default_sigma_z(), sigma_a=rtp.progressive.DENOISE_SIGMA_A,
           normal_log2=rtp.progressive.DENOISE_NORMAL_LOG2)
new = lambda: torch.empty((n, 4), dtype=torch.float32, device="cuda")
cv, out, scratch, tg0, tg1 = new(), new(), new(), new(), new()
stream = torch.cuda.current_stream().cuda_stream


def resolve():
    dev.resolve_device(r.sums.data_ptr(), n, cv.data_ptr(), m2_ptr=r.m2.data_ptr(), count_ptr=r.count.data_ptr(),
                       stream=stream)


def guides():
    dev.render_guides_device(r.camera, nx, ny, tg0.data_ptr(), tg1.data_ptr(), stream=stream)


def kernel(levels):
    return lambda: dev.denoise_device(cv.data_ptr(), nx, ny, out.data_ptr(), scratch.data_ptr(),
                                      g0_ptr=g["g0"].data_ptr(), g1_ptr=g["g1"].data_ptr(), levels=levels,
                                      stream=stream, **prm)


def one_spp_pass():
    dev.render_resume_device(r.camera, nx, ny, 1, a.depth, r.sums.data_ptr(), r.seed.data_ptr(),
                             live_ptr=r.live.data_ptr(), m2_ptr=r.m2.data_ptr(), stream=stream)


H = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def luma(c):
    return (0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]


def torch_level(cin, step):
    """One level of the filter over [ny, nx, 4] tensors, tap by tap."""
    c, G0, G1 = cin.view(ny, nx, 4), g["g0"].view(ny, nx, 4), g["g1"].view(ny, nx, 4)
    valid = ~(c[..., 3] < 0)
    lum = luma(c)
    lden = prm["sigma_l"] * torch.sqrt(c[..., 3]) + 1e-4
    sc = torch.zeros((ny, nx, 3), dtype=torch.float32, device="cuda")
    sv = torch.zeros((ny, nx), dtype=torch.float32, device="cuda")
    sw = torch.zeros((ny, nx), dtype=torch.float32, device="cuda")
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ox, oy = step * dx, step * dy
            x0, x1, y0, y1 = max(0, -ox), min(nx, nx - ox), max(0, -oy), min(ny, ny - oy)
            if x0 >= x1 or y0 >= y1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
            cq, vp = c[Q], valid[P]
            if dx == 0 and dy == 0:
                ok, w = vp, torch.full_like(lum[P], 9 / 64)
            else:
                ok = valid[Q]
                k = H[dx + 2] * H[dy + 2]
                hp, hq = G1[P][..., 3] != 0, G1[Q][..., 3] != 0
                m = torch.clamp_min((G0[P][..., 0] * G0[Q][..., 0] + G0[P][..., 1] * G0[Q][..., 1]) +
                                    G0[P][..., 2] * G0[Q][..., 2], 0.0)
                wn = m
                for _ in range(prm["normal_log2"]):
                    wn = wn * wn
                dz = torch.abs(G0[P][..., 3] - G0[Q][..., 3]) / (prm["sigma_z"] * step)
                da = ((G1[P][..., :3] - G1[Q][..., :3]) ** 2).sum(-1)
                wg = ((k * wn) * (1 / (1 + dz * dz))) * (1 / (1 + da / prm["sigma_a"] ** 2))
                w = torch.where(hp != hq, torch.zeros_like(wg), torch.where(hp, wg, torch.full_like(wg, k)))
                dl = torch.abs(lum[P] - lum[Q]) / lden[P]
                w = torch.where(vp, w * (1 / (1 + dl * dl)), w)
            w = torch.where(ok, w, torch.zeros_like(w))
            w = torch.nan_to_num(w, nan=0.0)
            sc[P] += w[..., None] * torch.where(ok[..., None], cq[..., :3], torch.zeros_like(cq[..., :3]))
            sv[P] += (w * w) * torch.where(ok, cq[..., 3], torch.zeros_like(sv[P]))
            sw[P] += w
    res = torch.cat([sc / sw[..., None], (sv / (sw * sw))[..., None]], dim=-1)
    return torch.where((sw > 0)[..., None], res, c).reshape(n, 4)


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


resolve()
torch.cuda.synchronize()
# the torch side: level s on the torch output of level s - 1 (computed once, untimed)
t_in = [cv]
for s in range(L):
    t_in.append(torch_level(t_in[s], 1 << s))
kernel(L)()
torch.cuda.synchronize()
diff = (out[:, :3] - t_in[L][:, :3]).abs()
scale = float(out[:, :3].abs().max())
same_valid = bool(((out[:, 3] < 0) == (t_in[L][:, 3] < 0)).all())

sides = {"guides": (guides, a.inner), "resolve": (resolve, a.inner)}
sides.update({f"kernel_L{k}": (kernel(k), a.inner) for k in range(1, L + 1)})
sides.update({f"torch_level{s}": ((lambda s=s: torch_level(t_in[s], 1 << s)), max(1, a.inner // 10)) for s in range(L)})
for fn, _ in sides.values():
    fn()
torch.cuda.synchronize()
ms = {k: [] for k in sides}
for _ in range(a.reps):
    for name, (fn, inner) in sides.items():
        ms[name].append(window(fn, inner))
# (last: the pass adds samples to the state the other sides read)
ms["resume_1spp"] = [window(one_spp_pass, 5) for _ in range(a.reps)]

stat = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
rep = {"nx": nx, "ny": ny, "levels": L, "spp": a.spp, "reps": a.reps, "inner": a.inner, "params": prm,
       "torch_vs_kernel": {"max_abs_rgb_diff": float(diff.max()), "max_rgb": scale, "same_invalid_pixels": same_valid},
       "ms_per_call": {k: stat(v) for k, v in ms.items()}}
med = lambda k: statistics.median(ms[k])
levels = []
prev = 0.0
for s in range(L):
    t = med(f"kernel_L{s + 1}") - prev
    prev = med(f"kernel_L{s + 1}")
    tt = med(f"torch_level{s}")
    levels.append({"level": s, "step": 1 << s, "kernel_ms": round(t, 4), "kernel_GBps_of_min_traffic": round(n * 64 / t / 1e6, 1),
                   "torch_ms": round(tt, 4), "torch_over_kernel": round(tt / t, 1)})
rep["levels_detail"] = levels
rep["preview_ms"] = round(med("resolve") + med(f"kernel_L{L}"), 4)
print(json.dumps(rep), flush=True)
print(f"guides {med('guides'):.4f} ms  resolve {med('resolve'):.4f} ms  filter L={L} {med(f'kernel_L{L}'):.4f} ms  "
      f"one 1-spp resume pass {med('resume_1spp'):.4f} ms")
for d in levels:
    print(f"level {d['level']} step {d['step']:2d}: kernel {d['kernel_ms']:.4f} ms "
          f"({d['kernel_GBps_of_min_traffic']:.0f} GB/s of the minimum 64 B/pixel)  torch {d['torch_ms']:.3f} ms "
          f"({d['torch_over_kernel']:.0f}x)")
dev.close()
