"""The three diagnostics instances of the pool kernel (RTP_DEBUG_STATS=1:
rtp_render_pool<true,false>, <true,true> and the planned <true,false,false,true>)
against the production instance of the same call: the same sums, final seeds
and live counts bit for bit, and per-wave counters that satisfy what the
scheduling loop implies:

  ff_lanes     == npix * spp     every finished sample passes the fast-forward batch once;
  bounce_lanes == sum(live)      one lane-iteration per live depth (the sphere-BVH instance
                                 also counts the iterations a lane spends walking: >=);
  dead_lanes   == npix * spp * depth - sum(live) + ended   with the jump tables off every
                                 dead depth is hashed.  pool_body: rem = D - 1 - k_end +
                                 (res != kAlive), live += k_end + 1: a path that misses or hits
                                 the light at depth k_end leaves that depth's own draws to the
                                 fast-forward (bounce<.., kDeferDead>), so its sample hashes
                                 depth - live + 1 depths, and only the path that survives depth
                                 D - 1 hashes depth - live = 0.  `ended` counts the former: every
                                 live depth is shaded once and misses (sum(live) - hit_lanes),
                                 hits the light (light_lanes) or scatters and lives on.
                                 (The identity without `ended`, every sample hashing depth - live,
                                 does not hold on any build: it forgets the deferred draws.)
  ffrad_lanes  == light_lanes    the batch computes one radiance product per light hit.

62 x 47 = 2914 entries: the interleaved deal gives 46 waves of 63 or 64 slots (the
last round of the deal and of the write-out is partial), the plan 22 full
128-entry waves and one of 98."""
from __future__ import annotations

import numpy as np
import pytest

from _util import assert_render_equal

pytestmark = pytest.mark.gpu
NX, NY, SPP, DEPTH = 62, 47, 5, 8
N = NX * NY


def _render(device, planned):
    import torch

    import raytracingtherestofyourlife_amd as rtp

    rgba = torch.full((N, 4), 7.0, dtype=torch.float32, device="cuda")
    seed = torch.zeros(N, dtype=torch.int32, device="cuda")
    live = torch.zeros(N, dtype=torch.int32, device="cuda")
    if planned:
        begin = np.minimum(np.arange(0, N + 128, 128), N).astype(np.int32)
        assert begin[-1] == N and 0 < begin[-1] - begin[-2] < 128
        wb = torch.from_numpy(begin).cuda()
        device.render_planned_device(rtp.default_camera(), NX, NY, SPP, DEPTH, rgba.data_ptr(), N, wb.data_ptr(),
                                     begin.size - 1, seed_ptr=seed.data_ptr(), live_ptr=live.data_ptr())
    else:
        device.render_device(rtp.default_camera(), NX, NY, SPP, DEPTH, rgba.data_ptr(), seed_ptr=seed.data_ptr(),
                             live_ptr=live.data_ptr())
    torch.cuda.synchronize()
    return rgba.cpu().numpy(), seed.cpu().numpy().view(np.uint32), live.cpu().numpy().view(np.uint32)


@pytest.fixture(params=["off", "on"])
def tables(request, device):
    before = device.ff_info()["policy"]
    device.set_ff_tables(request.param)
    yield request.param
    device.set_ff_tables(before)


@pytest.mark.parametrize("instance", ["plain", "bvh", "planned"])
def test_stats_instance(device, tables, instance, monkeypatch):
    device.set_cornell_box(3 if instance == "bvh" else 0)
    try:
        assert (device.sphere_walk() != "scan") == (instance == "bvh")
        want = _render(device, instance == "planned")
        monkeypatch.setenv("RTP_DEBUG_STATS", "1")
        got = _render(device, instance == "planned")
        c = device.debug_counters()
        records = device.debug_wave_records() if instance == "plain" else None
        monkeypatch.delenv("RTP_DEBUG_STATS")
    finally:
        device.set_cornell_box(0)
    assert_render_equal(got, want, f"{instance} stats instance, tables {tables}")
    live = int(got[2].astype(np.int64).sum())
    ended = live - c["hit_lanes"] + c["light_lanes"]
    print({k: c[k] for k in ("waves", "ff_lanes", "bounce_lanes", "dead_lanes", "hit_lanes", "light_lanes",
                             "ffrad_lanes", "end_lanes")}, "sum(live)", live, "ended", ended)
    assert c["waves"] > 0
    assert c["waves"] == 23 or instance != "planned"
    assert c["ff_lanes"] == N * SPP
    if instance == "bvh":
        assert c["bounce_lanes"] >= live
    else:
        assert c["bounce_lanes"] == live
    assert 0 <= ended <= N * SPP and c["ffrad_lanes"] == c["light_lanes"]
    if tables == "off":
        assert c["dead_lanes"] == N * SPP * DEPTH - live + ended
    if records is not None:  # the raw per-wave records are what debug_counters() sums
        names = device.DEBUG_COUNTERS[:-1]
        assert records.dtype == np.uint64 and records.shape == (c["waves"], len(names))
        assert records.sum(axis=0, dtype=np.uint64).tolist() == [c[k] for k in names]
        assert int(records[:, names.index("cycles_total")].max()) == c["max_wave_cycles"]
