"""Resident waves the pool kernel plans for a pixel count (device occupancy query)."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401  (one HIP runtime)
from raytracingtherestofyourlife_amd import _lib

L = _lib.load()
STATS = 1 if os.environ.get("RTP_DEBUG_STATS", "")[:1] == "1" else 0  # (the diagnostics build's occupancy)
for npix in [int(a) for a in sys.argv[1:]] or [640000]:
    for bvh in (0, 1):
        v, w = ctypes.c_int(), ctypes.c_int()
        lanes = L.rtp_plan_history_lanes(npix, 1000, bvh, STATS, v, w)
        print(f"npix {npix} bvh {bvh}: waves {w.value}, history lanes {lanes}")
