"""Mesh scenes (rtp_set_scene_mesh): the walk of the quad BVH against the
brute-force scan on generated planar-facet terrains in a lit room, and the
Cornell box through rtp_set_scene_mesh against rtp_set_scene (development
tool; its output is profiles/mesh_bench.txt).

    python tools/mesh_bench.py [--sizes 1024,16384,262144,1048576] [--reps 10]
        [--nx 512 --ny 512 --spp 16 --depth 50] [--scan-max 16384]
        [--scene grid|hills|hills_quads]
    RTP_LIB_PATH=variants/mesh_leaf1.so python tools/mesh_bench.py ...   # kMeshLeaf
        (tools/build_variant.sh variants/mesh_leaf1.so -DRTP_MESH_LEAF=1)

Per size: the host build (rtp_mesh_build_host, seconds, nodes per octant copy,
bytes of the eight compact copies and of the quad records), then kernel
milliseconds of timed rtp_render_device calls from the default camera.  Where
the scan finishes in seconds (<= --scan-max quads) a second context holds the
same scene set under RTP_MESH_SCAN=1 and the two alternate, window by window;
every side is warmed up first; the report is the median, minimum and maximum
of --reps windows.  The RNG jump tables are off.  One JSON line per case.

--scene hills: hills(n), the curved terrain of tests/_trimeshes.py at n terrain
cells, each given as two triangle cells (2 n + 5 cells); hills_quads: the same
terrain as n bent quads, most of them with the unbounded box (the report's
"cells", "triangles", "unbounded" are Device.mesh_counts()).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

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
ap.add_argument("--scan-max", type=int, default=16384)
ap.add_argument("--scene", choices=("grid", "hills", "hills_quads"), default="grid")
a = ap.parse_args()
if a.reps < 10:
    ap.error("--reps must be at least 10")

L = rtp.load()
leaf = L.rtp_mesh_leaf_size()
cam = rtp.default_camera()
N = a.nx * a.ny
out = torch.zeros((N, 4), dtype=torch.float32, device="cuda")


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def kernel_ms(dev):
    return dev.render_device(cam, a.nx, a.ny, a.spp, a.depth, out.data_ptr(), timed=True).kernel_ms


def context(setter, scan=False):
    dev = rtp.Device(0)
    dev.set_ff_tables("off")
    if scan:
        os.environ["RTP_MESH_SCAN"] = "1"
    try:
        setter(dev)
    finally:
        os.environ.pop("RTP_MESH_SCAN", None)
    return dev


def alternate(devs):
    for _ in range(a.warmup):
        for d in devs.values():
            kernel_ms(d)
    ms = {k: [] for k in devs}
    for _ in range(a.reps):
        for k, d in devs.items():
            ms[k].append(kernel_ms(d))
    return ms


for n in [int(s) for s in a.sizes.split(",") if s]:
    m = _meshes.grid(n) if a.scene == "grid" else _trimeshes.hills(n, a.scene == "hills")
    t0 = time.perf_counter()
    b = _meshes.build_host(m)
    build_s = time.perf_counter() - t0
    nodes = len(b["nodes"])
    devs = {"walk": context(lambda d: d.set_scene_mesh(*m.set_args()))}
    if n <= a.scan_max:
        devs["scan"] = context(lambda d: d.set_scene_mesh(*m.set_args()), scan=True)
    ms = alternate(devs)
    # (a baseline library named by RTP_LIB_PATH may be from before rtp_mesh_counts)
    cells, triangles, unbounded = devs["walk"].mesh_counts() if hasattr(L, "rtp_mesh_counts") else (None, None, None)
    rep = {"case": f"{a.scene}({n})", "quads": len(m.quads), "triangles": triangles, "unbounded": unbounded, "mesh_leaf": leaf, "host_build_s": round(build_s, 3),
           "nodes_per_octant": nodes, "node_bytes": 8 * 16 * nodes, "quad_bytes": 160 * len(m.quads),
           "nx": a.nx, "ny": a.ny, "spp": a.spp, "depth": a.depth, "reps": a.reps}
    for k, v in ms.items():
        rep[k + "_kernel_ms"] = summary(v)
        rep[k + "_msamples_per_s"] = round(N * a.spp / statistics.median(v) / 1e3, 2)
    print(json.dumps(rep), flush=True)
    for d in devs.values():
        d.close()

# the Cornell box: 18 quads behind the BVH against the inline scalar scan (informative: nothing switches over)
c = _meshes.cornell(0)
devs = {"mesh": context(lambda d: d.set_scene_mesh(*c.set_args())), "inline": context(lambda d: d.set_cornell_box(0))}
ms = alternate(devs)
rep = {"case": "cornell0", "quads": len(c.quads), "mesh_leaf": leaf, "nx": a.nx, "ny": a.ny, "spp": a.spp,
       "depth": a.depth, "reps": a.reps}
for k, v in ms.items():
    rep[k + "_kernel_ms"] = summary(v)
    rep[k + "_msamples_per_s"] = round(N * a.spp / statistics.median(v) / 1e3, 2)
print(json.dumps(rep), flush=True)
for d in devs.values():
    d.close()
