"""The table of render-kernel instances (csrc/rtp_launch.hpp kInstances): every
mode a launch can be in resolves to the kernel it must run, and every other
mode is refused (rtp_launch_render: hipErrorNotSupported).  CPU only: the
lookup touches no device.

The expected list is written out by hand, one line per instance.  The names
are the kernels with their template arguments as the table spells them,
rtp_render_pool<kStats, kBvh, kTiles, kPlan, kSteal, kViews, kResume> and
rtp_render_pool_lds<kTiles, kSteal> (trailing false arguments left out)."""
from __future__ import annotations

import itertools

# (variant, stats, walk, tiles, plan, steal, views, resume) -> kernel
#  walk: 0 no sphere BVH, 1 the global walk, 2 the LDS walk
EXPECTED = {
    # lockstep
    (1, 0, 0, 0, 0, 0, 0, 0): "rtp_render_lockstep<false>",
    (1, 0, 1, 0, 0, 0, 0, 0): "rtp_render_lockstep<true>",
    # the LDS walk: {tiles} x {steal}
    (2, 0, 2, 0, 0, 0, 0, 0): "rtp_render_pool_lds<false, false>",
    (2, 0, 2, 1, 0, 0, 0, 0): "rtp_render_pool_lds<true, false>",
    (2, 0, 2, 0, 0, 1, 0, 0): "rtp_render_pool_lds<false, true>",
    (2, 0, 2, 1, 0, 1, 0, 0): "rtp_render_pool_lds<true, true>",
    # resume: {bvh} x {steal}
    (2, 0, 0, 0, 0, 0, 0, 1): "rtp_render_pool<false, false, false, false, false, false, true>",
    (2, 0, 1, 0, 0, 0, 0, 1): "rtp_render_pool<false, true, false, false, false, false, true>",
    (2, 0, 0, 0, 0, 1, 0, 1): "rtp_render_pool<false, false, false, false, true, false, true>",
    (2, 0, 1, 0, 0, 1, 0, 1): "rtp_render_pool<false, true, false, false, true, false, true>",
    # views: {steal}
    (2, 0, 0, 0, 0, 0, 1, 0): "rtp_render_pool<false, false, false, false, false, true>",
    (2, 0, 0, 0, 0, 1, 1, 0): "rtp_render_pool<false, false, false, false, true, true>",
    # a wave plan: {stats}
    (2, 0, 0, 0, 1, 0, 0, 0): "rtp_render_pool<false, false, false, true>",
    (2, 1, 0, 0, 1, 0, 0, 0): "rtp_render_pool<true, false, false, true>",
    # stealing: {bvh} x {tiles}
    (2, 0, 0, 0, 0, 1, 0, 0): "rtp_render_pool<false, false, false, false, true>",
    (2, 0, 1, 0, 0, 1, 0, 0): "rtp_render_pool<false, true, false, false, true>",
    (2, 0, 0, 1, 0, 1, 0, 0): "rtp_render_pool<false, false, true, false, true>",
    (2, 0, 1, 1, 0, 1, 0, 0): "rtp_render_pool<false, true, true, false, true>",
    # the tile deal without stealing: {bvh}
    (2, 0, 0, 1, 0, 0, 0, 0): "rtp_render_pool<false, false, true>",
    (2, 0, 1, 1, 0, 0, 0, 0): "rtp_render_pool<false, true, true>",
    # plain: {stats} x {bvh}
    (2, 0, 0, 0, 0, 0, 0, 0): "rtp_render_pool<false, false>",
    (2, 0, 1, 0, 0, 0, 0, 0): "rtp_render_pool<false, true>",
    (2, 1, 0, 0, 0, 0, 0, 0): "rtp_render_pool<true, false>",
    (2, 1, 1, 0, 0, 0, 0, 0): "rtp_render_pool<true, true>",
}
# The one fallback: the tile deal has no stats build, so a tile-deal launch
# under RTP_DEBUG_STATS=1 runs the production tile instance.
STATS_TILES = {
    (2, 1, 0, 1, 0, 0, 0, 0): "rtp_render_pool<false, false, true>",
    (2, 1, 1, 1, 0, 0, 0, 0): "rtp_render_pool<false, true, true>",
}


def _lookup():
    import raytracingtherestofyourlife_amd as rtp

    L = rtp.load()

    def name(mode):
        got = L.rtp_instance_name(*mode)
        return got.decode() if got is not None else None

    return name


def test_expected_list_is_the_24_instances():
    assert len(EXPECTED) == 24 and len(set(EXPECTED.values())) == 24
    assert not set(EXPECTED) & set(STATS_TILES)


def test_every_pool_mode_resolves_or_is_refused():
    name = _lookup()
    modes = [(2, *m) for m in itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1))]
    assert len(modes) == 192
    want = {**EXPECTED, **STATS_TILES}
    found = {}
    for m in modes:
        got = name(m)
        assert got == want.get(m), f"mode {m}: {got!r}, expected {want.get(m)!r}"
        if got is not None:
            found[m] = got
    pool = {m: k for m, k in EXPECTED.items() if m[0] == 2}
    assert {m: k for m, k in found.items() if m not in STATS_TILES} == pool and len(pool) == 22


def test_stats_with_tiles_runs_the_production_tile_instance():
    name = _lookup()
    for m, kernel in STATS_TILES.items():
        plain = (m[0], 0, *m[2:])
        assert name(m) == kernel == EXPECTED[plain] == name(plain)


def test_lockstep_takes_a_list_or_range_only():
    name = _lookup()
    for walk in (0, 1):
        assert name((1, 0, walk, 0, 0, 0, 0, 0)) == EXPECTED[(1, 0, walk, 0, 0, 0, 0, 0)]
        for tiles, views, resume in itertools.product((0, 1), repeat=3):
            if tiles or views or resume:
                assert name((1, 0, walk, tiles, 0, 0, views, resume)) is None, (walk, tiles, views, resume)
    assert name((1, 0, 2, 0, 0, 0, 0, 0)) is None  # (the LDS walk is the pool kernel's)
    for variant in (0, 3):
        assert name((variant, 0, 0, 0, 0, 0, 0, 0)) is None
