"""Batched views against the per-view loop (development tool): one
rtp_render_views_device launch over all views vs one rtp_render_device per
view, outputs resident on the device.

    python tools/views_bench.py [--loop-lib build_exp/parent.so] [--reps 12]
        [--phicount 15 --thetacount 15 --nx 128 --ny 128 --spp 10 --depth 5]

Each timed window runs from the first enqueue to one final synchronise (no
stats call inside it: those synchronise).  Both sides are warmed up first and
then alternate within this process; the report is the median, minimum and
maximum of --reps windows each, and the batched launch's kernel time from one
extra timed call.  --loop-lib names a second librtp (e.g. the parent revision,
tools/build_variant.sh with RTP_SRC_REV) whose rtp_render_device runs the
loop, so that the baseline is not the code under test; without it the in-tree
library runs both.  The RNG jump tables are off on both sides (a one-shot
rtp_path run never builds them, and two libraries' tables do not fit one
device together).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import raytracingtherestofyourlife_amd as rtp  # noqa: E402
from raytracingtherestofyourlife_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--phicount", type=int, default=15)
ap.add_argument("--thetacount", type=int, default=15)
ap.add_argument("--views", type=int, default=0, help="use only the first N hemisphere views (0: all)")
ap.add_argument("--nx", type=int, default=128)
ap.add_argument("--ny", type=int, default=128)
ap.add_argument("--spp", type=int, default=10)
ap.add_argument("--depth", type=int, default=5)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--loop-lib", default="", help="librtp.so whose rtp_render_device runs the per-view loop")
a = ap.parse_args()
if a.reps < 10:
    ap.error("--reps must be at least 10")

cams = rtp.hemisphere_cameras(a.phicount, a.thetacount)
if a.views:
    cams = cams[: a.views]
V, N = len(cams), a.nx * a.ny
dev = rtp.Device(0)
dev.set_cornell_box(0)
dev.set_ff_tables("off")
out_b = torch.zeros((V * N, 4), dtype=torch.float32, device="cuda")
out_l = torch.zeros((V * N, 4), dtype=torch.float32, device="cuda")
stream = torch.cuda.current_stream().cuda_stream
c_cams = [c.to_c() for c in cams]

if a.loop_lib:  # the baseline library beside the package's own, bound with the same table
    P = ctypes.CDLL(os.path.abspath(a.loop_lib))
    vp = ctypes.c_void_p
    _lib.bind(P)  # (a baseline from an earlier revision lacks the later entry points: they stay unbound)

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"{a.loop_lib}: {P.rtp_last_error().decode(errors='replace')}")

    ctx = vp()
    ok(P.rtp_create(0, ctypes.byref(ctx)))
    desc = _lib.RtpSceneDesc()
    ok(P.rtp_cornell_box(0, ctypes.byref(desc)))
    ok(P.rtp_set_scene(ctx, ctypes.byref(desc)))
    ok(P.rtp_set_ff_tables(ctx, _lib.RTP_FF_TABLES_OFF))

    def loop():
        for v, cam in enumerate(c_cams):
            ok(P.rtp_render_device(ctx, ctypes.byref(cam), a.nx, a.ny, a.spp, a.depth, 0, 0, N, None,
                                   vp(out_l.data_ptr() + 16 * N * v), None, vp(stream or None), None))
else:
    def loop():
        for v, cam in enumerate(cams):
            dev.render_device(cam, a.nx, a.ny, a.spp, a.depth, out_l.data_ptr() + 16 * N * v, stream=stream)


def batched():
    dev.render_views_device(cams, a.nx, a.ny, a.spp, a.depth, out_b.data_ptr(), stream=stream)


def window(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


for _ in range(a.warmup):
    window(batched), window(loop)
same = bool(((out_b.view(torch.int32) == out_l.view(torch.int32)) | (torch.isnan(out_b) & torch.isnan(out_l))).all())
ms = {"batched": [], "loop": []}
for _ in range(a.reps):
    ms["batched"].append(window(batched))
    ms["loop"].append(window(loop))
st = dev.render_views_device(cams, a.nx, a.ny, a.spp, a.depth, out_b.data_ptr(), stream=stream, timed=True)
samples = V * N * a.spp
rep = {"views": V, "nx": a.nx, "ny": a.ny, "spp": a.spp, "depth": a.depth, "samples": samples, "reps": a.reps,
       "loop_lib": a.loop_lib or "in-tree", "outputs_equal": same, "batched_kernel_ms": round(st.kernel_ms, 4),
       "batched_kernel_msamples_per_s": round(samples / st.kernel_ms / 1e3, 1)}
for k, v in ms.items():
    rep[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
rep["loop_over_batched_median"] = round(rep["loop_ms"]["median"] / rep["batched_ms"]["median"], 3)
print(json.dumps(rep), flush=True)
if a.loop_lib:
    P.rtp_destroy(ctx)
dev.close()
