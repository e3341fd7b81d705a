"""Triangle cells of a mesh scene: builds of the library against each other on
one scene, window by window (development tool; its output is
profiles/mesh_tri_bench.txt).

    python tools/mesh_tri_bench.py --libs tree=,parent=variants/parent.so,parent2=variants/parent2.so \\
        --cases grid:16384,grid:262144 [--reps 10] [--nx 512 --ny 512 --spp 16 --depth 50]

--libs: name=path pairs; an empty path is the in-tree library.  Every library
is loaded into this process once (two copies of one build need two files), each
gets a context of its own with the scene of the case, and the timed
rtp_render_device calls alternate library by library: 2 warm-ups, then --reps
windows, the RNG jump tables off (tools/mesh_bench.py's protocol).  The report
per case and library: kernel ms as median / min / max, and where the library
has rtp_mesh_counts the scene's cells, triangle cells and unbounded cells.

--cases: scene:n pairs -- grid (tests/_meshes.py grid(n), planar facets),
hills (tests/_trimeshes.py hills(n): n curved terrain cells as 2 n triangle
cells) and hills_quads (the same terrain as n bent quads).

The parent commit as a library: RTP_SRC_REV=<rev> tools/build_variant.sh
variants/parent.so; the walk's general test on triangle records:
tools/build_variant.sh variants/tri0.so -DRTP_MESH_TRI_TEST=0.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import torch  # noqa: E402

import _meshes  # noqa: E402
import _trimeshes  # noqa: E402
import raytracingtherestofyourlife_amd as rtp  # noqa: E402
from raytracingtherestofyourlife_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--libs", required=True)
ap.add_argument("--cases", required=True)
ap.add_argument("--nx", type=int, default=512)
ap.add_argument("--ny", type=int, default=512)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--depth", type=int, default=50)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()
if a.reps < 10:
    ap.error("--reps must be at least 10")


def library(path):
    if not path:
        return rtp.load()
    L = ctypes.CDLL(os.path.abspath(path))
    _lib.bind(L)  # (a library of an earlier revision lacks the later entry points: they stay unbound)
    return L


def device(L):
    d = rtp.Device(0, lib=L)
    d.set_ff_tables("off")
    return d


libs = {}
for pair in a.libs.split(","):
    name, _, path = pair.partition("=")
    libs[name] = library(path)
cam = rtp.default_camera()
N = a.nx * a.ny
out = torch.zeros((N, 4), dtype=torch.float32, device="cuda")
os.environ.pop("RTP_MESH_SCAN", None)
os.environ.pop("RTP_MESH_BUILD", None)


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def kernel_ms(dev):
    return dev.render_device(cam, a.nx, a.ny, a.spp, a.depth, out.data_ptr(), timed=True).kernel_ms


for case in a.cases.split(","):
    scene, _, n = case.partition(":")
    n = int(n)
    m = _meshes.grid(n) if scene == "grid" else _trimeshes.hills(n, scene == "hills")
    devs = {}
    for name, L in libs.items():
        devs[name] = device(L)
        devs[name].set_scene_mesh(*m.set_args())
    for _ in range(a.warmup):
        for d in devs.values():
            kernel_ms(d)
    ms = {k: [] for k in devs}
    for _ in range(a.reps):
        for k, d in devs.items():
            ms[k].append(kernel_ms(d))
    rep = {"case": f"{scene}({n})", "cells": len(m.quads), "nx": a.nx, "ny": a.ny, "spp": a.spp, "depth": a.depth,
           "reps": a.reps}
    for k, d in devs.items():
        rep[k + "_kernel_ms"] = summary(ms[k])
        if hasattr(d._L, "rtp_mesh_counts"):
            rep[k + "_counts"] = d.mesh_counts()
    print(json.dumps(rep), flush=True)
    for d in devs.values():
        d.close()
