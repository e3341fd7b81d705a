"""What an adaptive pass costs (development tool): ProgressiveRender.refine()
-- the host path: the state copied to the host, the float64 estimate, the id
list uploaded, torch gather and scatter around the resume pass -- beside
ProgressiveRender.refine_device() (include/rtp_adaptive.h) on identical states.

    python tools/adaptive_bench.py [--canvas 800x800 --canvas 3840x2160] [--spp 8] [--passspp 1]
                                   [--depth 50] [--reps 12]

Per canvas: the Cornell box (variant 0) rendered --spp samples per pixel; the
threshold is the median of the finite noise estimates, so a pass selects about
half of the canvas.  A window restores that state (untimed), runs one pass of
--passspp samples and waits for the device: wall time.  The sides alternate in
one process after a warm-up of each; the report is the median (min-max) over
--reps windows per side.  The device path's parts are the device-event times
of further timed passes on the same state (adaptive.refine_last_timing):
select (three launches), gather, the resume launch, scatter; the selection's
achieved bytes per second are against its minimum traffic, 2 x 28 B read per
entry plus 8 B per selected id.  The yardstick is a 1-spp step() of the whole
canvas, timed with device events.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import raytracingtherestofyourlife_amd as rtp  # noqa: E402
from raytracingtherestofyourlife_amd import adaptive  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--canvas", action="append", help="NXxNY; default: 800x800 and 3840x2160")
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--passspp", type=int, default=1)
ap.add_argument("--depth", type=int, default=50)
ap.add_argument("--reps", type=int, default=12)
a = ap.parse_args()
if a.reps < 10:
    ap.error("--reps must be at least 10")
canvases = [tuple(int(v) for v in c.split("x")) for c in (a.canvas or ["800x800", "3840x2160"])]
MAX_SPP = 1 << 20

dev = rtp.Device(0)
dev.set_cornell_box(0)
dev.set_ff_tables("off")
stat = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
fmt = lambda d: f"{d['median']:.3f} ({d['min']:.3f}-{d['max']:.3f})"

for nx, ny in canvases:
    n = nx * ny
    r = rtp.ProgressiveRender(dev, rtp.default_camera(), nx, ny, a.depth)
    r.step(a.spp)
    torch.cuda.synchronize()
    base = [t.clone() for t in (r.sums, r.seed, r.live, r.m2, r.count)]
    noise = r.noise_device()
    threshold = float(noise[torch.isfinite(noise)].median())

    def restore():
        for t, b in zip((r.sums, r.seed, r.live, r.m2, r.count), base):
            t.copy_(b)
        torch.cuda.synchronize()

    def wall(fn):
        restore()
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, got

    host = lambda: r.refine(a.passspp, threshold, MAX_SPP)
    device = lambda: r.refine_device(a.passspp, threshold, MAX_SPP)
    _, sel_host = wall(host)  # warm-up of each side
    _, sel_dev = wall(device)
    ms = {"host": [], "device": []}
    for _ in range(a.reps):
        ms["host"].append(wall(host)[0])
        ms["device"].append(wall(device)[0])
    parts = {k: [] for k in ("select", "gather", "resume", "scatter")}
    for _ in range(a.reps):
        restore()
        adaptive.refine_device(dev, r.camera, nx, ny, a.depth, r.sums.data_ptr(), r.seed.data_ptr(), r.m2.data_ptr(),
                               r.count.data_ptr(), a.passspp, threshold, MAX_SPP, live_ptr=r.live.data_ptr(),
                               stream=torch.cuda.current_stream().cuda_stream, timed=True)
        for k, v in adaptive.refine_last_timing(dev).items():
            parts[k].append(v)
    restore()
    step_ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        r.step(1)
        e1.record()
        e1.synchronize()
        step_ms.append(e0.elapsed_time(e1))
    sel_ms = statistics.median(parts["select"])
    min_bytes = 2 * 28 * n + 8 * sel_dev
    rep = {"nx": nx, "ny": ny, "depth": a.depth, "first_spp": a.spp, "pass_spp": a.passspp, "reps": a.reps,
           "threshold": threshold, "selected_host": sel_host, "selected_device": sel_dev,
           "wall_ms_per_pass": {k: stat(v) for k, v in ms.items()},
           "device_parts_ms": {k: stat(v) for k, v in parts.items()},
           "select_min_bytes": min_bytes, "select_GBps_of_min_traffic": round(min_bytes / sel_ms / 1e6, 1),
           "step_1spp_whole_canvas_ms": stat(step_ms)}
    print(json.dumps(rep), flush=True)
    w, p = rep["wall_ms_per_pass"], rep["device_parts_ms"]
    print(f"{nx} x {ny}, {a.spp} spp first, threshold {threshold:.4f}: refine() selects {sel_host}, "
          f"refine_device() {sel_dev} of {n}")
    print(f"  wall ms per pass of {a.passspp} spp, median (min-max) of {a.reps}: host path {fmt(w['host'])}   "
          f"device path {fmt(w['device'])}   ratio {w['host']['median'] / w['device']['median']:.1f}x")
    print(f"  device path, device ms: select {fmt(p['select'])}  gather {fmt(p['gather'])}  resume launch "
          f"{fmt(p['resume'])}  scatter {fmt(p['scatter'])}")
    print(f"  select: {rep['select_GBps_of_min_traffic']:.0f} GB/s of its minimum {min_bytes / 1e6:.1f} MB;  "
          f"a 1-spp step of the whole canvas: {fmt(rep['step_1spp_whole_canvas_ms'])} ms", flush=True)
    del r, base, noise
    torch.cuda.empty_cache()
dev.close()
