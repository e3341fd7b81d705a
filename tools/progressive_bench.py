"""What cutting a render into passes costs (development tool): a frame rendered
as 1, 4, 10 and 100 rtp_render_resume_device passes against the one-shot
rtp_render_device, the state resident on the device.

    python tools/progressive_bench.py [--base-lib build_exp/parent.so] [--reps 12]
        [--nx 800 --ny 800 --spp 1000 --depth 50] [--passes 1,4,10,100]

Each timed window runs from the first enqueue to one final synchronise (the
passes are queued back to back, no stats call inside: those synchronise).  All
sides are warmed up first and then alternate within this process; the report
is the median, minimum and maximum of --reps windows each.  --base-lib names a
second librtp (e.g. the parent revision, tools/build_variant.sh with
RTP_SRC_REV) whose rtp_render_device renders the one-shot frame, so that the
baseline is not the code under test; without it the in-tree library does.
The RNG jump tables are off on every side (two libraries' tables do not fit
one device together); the report states it.  Every split's sums, final seeds
and live counts are compared with the one-shot frame's bit for bit.
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
ap.add_argument("--nx", type=int, default=800)
ap.add_argument("--ny", type=int, default=800)
ap.add_argument("--spp", type=int, default=1000)
ap.add_argument("--depth", type=int, default=50)
ap.add_argument("--passes", default="1,4,10,100")
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--base-lib", default="", help="librtp.so whose rtp_render_device renders the one-shot baseline")
a = ap.parse_args()
if a.reps < 10:
    ap.error("--reps must be at least 10")
splits = [int(v) for v in a.passes.split(",")]

N = a.nx * a.ny
cam = rtp.default_camera()
c_cam = cam.to_c()
dev = rtp.Device(0)
dev.set_cornell_box(0)
dev.set_ff_tables("off")
stream = torch.cuda.current_stream().cuda_stream


def buffers():
    return (torch.zeros((N, 4), dtype=torch.float32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda"),
            torch.zeros(N, dtype=torch.int32, device="cuda"))


base_out, base_seed, base_live = buffers()
st_sums, st_seed, st_live = buffers()
st_m2 = torch.zeros(N, dtype=torch.float32, device="cuda")
fresh_seed = torch.arange(N, dtype=torch.int32, device="cuda")  # seed_base 0

if a.base_lib:  # the baseline library beside the package's own, bound with the same table
    P = ctypes.CDLL(os.path.abspath(a.base_lib))
    vp = ctypes.c_void_p
    _lib.bind(P)  # (a baseline from an earlier revision lacks the later entry points: they stay unbound)

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"{a.base_lib}: {P.rtp_last_error().decode(errors='replace')}")

    ctx = vp()
    ok(P.rtp_create(0, ctypes.byref(ctx)))
    desc = _lib.RtpSceneDesc()
    ok(P.rtp_cornell_box(0, ctypes.byref(desc)))
    ok(P.rtp_set_scene(ctx, ctypes.byref(desc)))
    ok(P.rtp_set_ff_tables(ctx, _lib.RTP_FF_TABLES_OFF))
    aux = _lib.RtpPixelAux(ctypes.cast(base_seed.data_ptr(), _lib.u32p), ctypes.cast(base_live.data_ptr(), _lib.u32p))

    def oneshot():
        ok(P.rtp_render_device(ctx, ctypes.byref(c_cam), a.nx, a.ny, a.spp, a.depth, 0, 0, N, None,
                               vp(base_out.data_ptr()), ctypes.byref(aux), vp(stream or None), None))
else:
    def oneshot():
        dev.render_device(cam, a.nx, a.ny, a.spp, a.depth, base_out.data_ptr(), stream=stream,
                          seed_ptr=base_seed.data_ptr(), live_ptr=base_live.data_ptr())


def split(n_passes):
    sizes = rtp.split_passes(a.spp, n_passes)

    def run():  # (the state's reset is part of the window: four small fills)
        st_sums.zero_(), st_live.zero_(), st_m2.zero_(), st_seed.copy_(fresh_seed)
        for s in sizes:
            dev.render_resume_device(cam, a.nx, a.ny, s, a.depth, st_sums.data_ptr(), st_seed.data_ptr(),
                                     live_ptr=st_live.data_ptr(), m2_ptr=st_m2.data_ptr(), stream=stream)
    return run


def window(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def equal_to_baseline():
    x, y = st_sums[:, :3].contiguous(), base_out[:, :3].contiguous()
    same = (x.view(torch.int32) == y.view(torch.int32)) | (torch.isnan(x) & torch.isnan(y))
    return bool(same.all()) and torch.equal(st_seed, base_seed) and torch.equal(st_live, base_live)


sides = {"oneshot": oneshot}
sides.update({f"passes_{k}": split(k) for k in splits})
equal = {}
for _ in range(a.warmup):
    for name, fn in sides.items():
        window(fn)
        if name != "oneshot":
            equal[name] = equal_to_baseline()
ms = {name: [] for name in sides}
for _ in range(a.reps):
    for name, fn in sides.items():
        ms[name].append(window(fn))
rep = {"nx": a.nx, "ny": a.ny, "spp": a.spp, "depth": a.depth, "reps": a.reps, "ff_tables": "off (every side)",
       "base_lib": a.base_lib or "in-tree", "state": "device-resident, m2 and live counts on",
       "outputs_equal": equal}
med0 = statistics.median(ms["oneshot"])
for name, v in ms.items():
    rep[name + "_ms"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                         "over_oneshot": round(statistics.median(v) / med0, 4)}
print(json.dumps(rep), flush=True)
if a.base_lib:
    P.rtp_destroy(ctx)
dev.close()
