"""Mesh scenes: the device build of the quad BVH (rtp_set_scene_mesh_device)
against the host build (rtp_set_scene_mesh) on tools/mesh_bench.py's terrains
(development tool; its output is profiles/mesh_device_build.txt).

    python tools/mesh_build_bench.py [--sizes 1024,16384,262144,1048576] [--reps 10]
        [--nx 512 --ny 512 --spp 16 --depth 50] [--scene grid|hills|hills_quads]

--scene hills: hills(n), the curved terrain of tests/_trimeshes.py at n terrain
cells as 2 n triangle cells; hills_quads: the same terrain as n bent quads.
Per size, one JSON line:
  build wall time (ms) of (a) rtp_set_scene_mesh from host arrays -- host build
  plus upload -- and (b) rtp_set_scene_mesh_device from tensors already on the
  device, alternating call by call on one context, --reps calls each after 2;
  kernel time (ms) of the same frame under each tree, each on a context of its
  own, alternating window by window (mesh_bench.py's method), --reps windows
  after 2, the RNG jump tables off; and the nodes per octant copy of each tree.
Median (min-max) throughout.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _meshes  # noqa: E402  (the generated terrains of the tests)
import _trimeshes  # noqa: E402
import raytracingtherestofyourlife_amd as rtp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1024,16384,262144,1048576")
ap.add_argument("--nx", type=int, default=512)
ap.add_argument("--ny", type=int, default=512)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--depth", type=int, default=50)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--scene", choices=("grid", "hills", "hills_quads"), default="grid")
a = ap.parse_args()
if a.reps < 10:
    ap.error("--reps must be at least 10")
os.environ.pop("RTP_MESH_BUILD", None)

L = rtp.load()
cam = rtp.default_camera()
N = a.nx * a.ny
out = torch.zeros((N, 4), dtype=torch.float32, device="cuda")


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def nodes_per_octant(dev):
    nn = ctypes.c_int32(0)
    assert L.rtp_debug_mesh_readback(dev.handle, 0, 0, nn, None, None, None, None) == 0
    return nn.value


def kernel_ms(dev):
    return dev.render_device(cam, a.nx, a.ny, a.spp, a.depth, out.data_ptr(), timed=True).kernel_ms


for n in [int(s) for s in a.sizes.split(",") if s]:
    m = _meshes.grid(n) if a.scene == "grid" else _trimeshes.hills(n, a.scene == "hills")
    args = m.set_args()
    tens = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (m.points, m.quads, m.quad_mat, m.quad_tex)]
    torch.cuda.synchronize()
    builders = {"host": lambda d: d.set_scene_mesh(*args), "device": lambda d: d.set_scene_mesh_device(*tens, *args[4:])}
    dev = rtp.Device(0)
    wall = {k: [] for k in builders}
    for i in range(a.warmup + a.reps):
        for k, build in builders.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            build(dev)
            if i >= a.warmup:
                wall[k].append(1e3 * (time.perf_counter() - t0))
    dev.close()
    devs = {}
    for k, build in builders.items():
        devs[k] = rtp.Device(0)
        devs[k].set_ff_tables("off")
        build(devs[k])
    for _ in range(a.warmup):
        for d in devs.values():
            kernel_ms(d)
    ms = {k: [] for k in devs}
    for _ in range(a.reps):
        for k, d in devs.items():
            ms[k].append(kernel_ms(d))
    rep = {"case": f"{a.scene}({n})", "quads": len(m.quads), "counts_host": devs["host"].mesh_counts(),
           "counts_device": devs["device"].mesh_counts(), "nx": a.nx, "ny": a.ny, "spp": a.spp, "depth": a.depth,
           "reps": a.reps}
    for k in builders:
        rep[k + "_build_ms"] = summary(wall[k])
        rep[k + "_nodes_per_octant"] = nodes_per_octant(devs[k])
        rep[k + "_walk_kernel_ms"] = summary(ms[k])
    rep["build_host_over_device"] = round(rep["host_build_ms"]["median"] / rep["device_build_ms"]["median"], 2)
    rep["walk_device_over_host"] = round(rep["device_walk_kernel_ms"]["median"] / rep["host_walk_kernel_ms"]["median"], 3)
    print(json.dumps(rep), flush=True)
    for d in devs.values():
        d.close()
