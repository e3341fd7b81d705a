"""The generated scenes of tests/_scenes.py are what the GPU parity tests of
test_gpu_scene_zoo.py render.  This file guards those inputs on the CPU, so
that the GPU tests cannot pass vacuously: the zoo holds every reachable
(kind, exact-parallelogram) pair, each variant sits on the side of its gate
it is meant for, the oracle's two implementations agree on every variant bit
for bit, and the renders are mostly lit, mostly NaN-free and really bounce.

Measured on the oracle at 64 x 64, 8 spp, depth 12:

    classification of zoo(): (0,F) 5, (0,T) 4, (1,T) 1, (2,T) 2, (3,T) 1,
        (4,T) 1, (5,T) 1, (6,T) 2, (7,T) 2, (8,T) 2, (9,F) 2, (9,T) 1, (10,F) 1
        (scaled(17) and scaled(555): (0,F) 7, (0,T) 2 -- rounding breaks two
        chance parallelograms of the box turned about a general axis)

    variant                  NaN pixels   lit pixels   max live bounces
    zoo, scaled(16)            0.0 %        86.2 %        86
    scaled(17)                 0.0 %        86.3 %        86
    scaled(555)                0.0 %        86.2 %        87
    many_axis                  2.0 %        84.4 %        86
    full                       3.7 %        82.3 %        88
    dups                       0.0 %        86.2 %        86
    turned(1 / 2 / 3)          2.7 / 4.6 / 6.3 %   83.5 / 81.8 / 80.1 %   90 / 87 / 86
    ior(1.33)                  0.0 %        86.5 %        87
    light_sphere_elsewhere     0.0 %        84.1 %        84

(NaN pixels come from paths that start a bounce exactly on a second surface:
the tiles 1/512 above the floor, the turned room's rounded corners.)"""
from __future__ import annotations

import numpy as np
import pytest

import _scenes as S
from _util import assert_render_equal

NX = NY = 64
SPP, DEPTH = 8, 12

CASES = S.VARIANTS

_renders = {}


def _render(oracle, name, z=None):
    if name not in _renders:
        z = CASES[name]() if z is None else z
        _renders[name] = oracle.render_pixels(z.scene(oracle), z.oracle_camera(oracle, NX, NY), NX, NY, SPP, DEPTH,
                                              np.arange(NX * NY, dtype=np.int64))
    return _renders[name]


def test_classify_reproduces_the_cornell_tally(oracle):
    """The four built-in scenes hold seven of the thirteen reachable pairs."""
    c012 = {(1, True): 9, (2, True): 5, (4, True): 2, (7, True): 2, (8, True): 2, (9, False): 1, (10, False): 1}
    c3 = {(1, True): 1, (2, True): 3, (4, True): 2}
    for variant, want, nq in ((0, c012, 22), (1, c012, 22), (2, c012, 22), (3, c3, 6)):
        sc = oracle.cornell_box(variant)
        assert sc.n_quads == nq
        assert S.tally(S.classify(sc.points_np(), sc.quad_ids_np()[:, 1:])) == want, variant


def test_classify_on_hand_made_quads():
    """One quad per rule of the definition: exact zeros decide the kind,
    componentwise float32 equality decides the parallelogram flag."""
    P = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0],          # unit square in z = 0
                  [1, 1, 1e-30],                                       # ... with v11 a tiny step off the plane
                  [1.5, 1, 0]], dtype=np.float32)                      # ... with v11 moved within the plane
    assert S.classify(P, [[0, 1, 2, 3]]) == [(1, True)]
    assert S.classify(P, [[0, 3, 2, 1]]) == [(3, True)]
    assert S.classify(P, [[0, 1, 4, 3]]) == [(0, False)]  # masks {1, 2, 6, 5}
    assert S.classify(P, [[0, 1, 5, 3]]) == [(0, False)]  # a trapezoid: masks {1, 2, 3, 1}


def test_zoo_holds_every_reachable_pair():
    t = S.tally(S.zoo().classify())
    assert sorted(t) == sorted(S.REACHABLE), t
    assert t == {(0, False): 5, (0, True): 4, (1, True): 1, (2, True): 2, (3, True): 1, (4, True): 1, (5, True): 1,
                 (6, True): 2, (7, True): 2, (8, True): 2, (9, False): 2, (9, True): 1, (10, False): 1}
    for name, fn in CASES.items():
        if not name.startswith("turned"):
            assert set(S.tally(fn().classify())) == set(S.REACHABLE), name


def test_zoo_keeps_the_reference_light_coupling():
    z = S.zoo()
    assert z.light == (8, 9, 10, 11) and z.quads[2][0] == (8, 9, 10, 11) and z.quads[2][1:] == [3, 3]
    assert np.unique(z.points[8:12, 1]).size == 1, "the light quad lies in a plane y = const"
    assert z.light_sphere_point == z.spheres[0][0]
    assert [S.MAT_TYPE[s[2]] for s in z.spheres] == [2, 0, 1], "glass, Lambertian, emissive"
    assert len(z.spheres) < 9, "below the sphere-BVH threshold"
    glass = [q for q, (_, m, _) in enumerate(z.quads) if S.MAT_TYPE[m] == 2]
    assert len(glass) == 1 and 1 <= z.classify()[glass[0]][0] <= 6, "one axis-plane glass pane"
    e = S.light_sphere_elsewhere()
    assert e.light_sphere_point == e.spheres[1][0] != z.light_sphere_point
    assert e.spheres[0][1] == z.spheres[0][1]


def test_variants_sit_on_their_side_of_each_gate():
    def axis_quads(z):
        return sum(1 for k, _ in z.classify() if 1 <= k <= 6)

    z = S.zoo()
    assert axis_quads(z) == 8 and np.abs(z.points).max() == 1.0 and S.prefilter_expected(z)
    # the coordinate limit: 16 is inside, 17 and 555 are not
    assert np.abs(S.scaled(16).points).max() == S.PRE_LIM and S.prefilter_expected(S.scaled(16))
    for s in (17, 555):
        assert axis_quads(S.scaled(s)) == 8 and not S.prefilter_expected(S.scaled(s))
    for s in (16, 17, 555):  # (scaling keeps every kind; 17 and 555 round two chance parallelograms away)
        assert [k for k, _ in S.scaled(s).classify()] == [k for k, _ in z.classify()]
        assert S.scaled(s).spheres[0][1] == np.float32(0.15625) * np.float32(s)
    # the count limit
    m = S.many_axis()
    assert axis_quads(m) == 8 + 36 > S.MAX_PRE and np.abs(m.points).max() == 1.0 and not S.prefilter_expected(m)
    # no axis-plane quad at all
    for deg in (1.0, 2.0, 3.0):
        assert axis_quads(S.turned(deg)) == 0 and not S.prefilter_expected(S.turned(deg))

    def distinct(z):
        return len({(v.tobytes(), q[1], q[2]) for v, q in zip(z.verts(), z.quads)})

    # the quad limit: 259 quads of which 256 are distinct; 257 distinct
    f = S.full()
    assert len(f.quads) == 259 and distinct(f) == S.MAX_QUADS
    dropped = sorted(set(range(259)) - set(S.kept_quads(f)))
    assert dropped == [2, 6, 11], "the copies sit at low indices, each after its original"
    assert axis_quads(f) - 2 <= S.MAX_PRE and S.prefilter_expected(f)  # (two of the three copies are axis-plane quads)
    o = S.overfull()
    assert len(o.quads) == distinct(o) == S.MAX_QUADS + 1
    # repeats with another material or vertex order are distinct quads
    d = S.dups()
    assert len(d.quads) == distinct(d) == len(z.quads) + 3
    V = d.verts()
    assert V[25].tobytes() == V[1].tobytes() and d.quads[25][1:] == [1, 1] and d.quads[1][1:] == [0, 0]
    assert V[26].tobytes() == V[4].tobytes() and d.quads[26][1:] == [0, 0] and d.quads[4][1:] == [1, 1]
    assert V[27].tobytes() == V[14][[1, 2, 3, 0]].tobytes() and d.classify()[14] == (0, True)


def test_prefilter_expectations_cover_both_states():
    """What prefilter_expected derives for each variant, pinned once."""
    on = {n for n, fn in S.VARIANTS.items() if S.prefilter_expected(fn())}
    assert on == {"zoo", "scaled16", "full", "dups", "ior133", "light_sphere_elsewhere"}
    assert set(S.VARIANTS) - on == {"scaled17", "scaled555", "many_axis", "turned1", "turned2", "turned3"}


def test_first_hits_of_the_two_cameras_show_every_pair(oracle):
    """The float64 first-hit check of the guides (test_gpu_scene_zoo.py) sees,
    over the default and the high camera, a clearly closest quad of every
    reachable pair and each sphere.  Measured: 90.3 % and 98.1 % of the
    pixels are clear; the rarest pair is (10, F) with 8 + 17 pixels."""
    z = S.zoo()
    nq = len(z.quads)
    pairs = z.classify()
    count = np.zeros(nq + len(z.spheres), dtype=np.int64)
    for cam in (z.cam, S.HIGH_CAM):
        _, first, _, clear = S.clear_first_hits(z, oracle.camera_setup(NX, NY, **cam), NX, NY)
        assert clear.mean() > 0.75
        count += np.bincount(first[clear], minlength=count.size)
    per_pair = {p: int(sum(count[q] for q in range(nq) if pairs[q] == p)) for p in S.REACHABLE}
    print(per_pair, count[nq:].tolist())
    assert min(per_pair.values()) >= 20, per_pair
    assert (count[nq:] >= 10).all(), count[nq:]


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_variants_agree_and_the_render_is_a_fair_input(oracle, name):
    z = CASES[name]()
    want = _render(oracle, name, z)
    soa = oracle.render_soa(z.scene(oracle), z.oracle_camera(oracle, NX, NY), NX, NY, SPP, DEPTH)
    assert_render_equal(soa, want, f"{name}: scalar against stage-structured oracle")
    rgb, _, live = want
    nan = np.isnan(rgb[:, :3]).any(axis=1)
    lit = ~nan & (rgb[:, :3].sum(axis=1) != 0)
    print(f"{name}: NaN pixels {nan.mean():.4f}, lit {lit.mean():.4f}, max live bounces {live.max()}")
    assert nan.mean() <= (0.15 if name.startswith("turned") else 0.10)
    assert lit.mean() >= 0.60
    assert live.max() > SPP, "no pixel bounced"


def test_each_special_input_changes_the_render(oracle):
    """The glass pane, the emissive sphere, the index of refraction and the
    light sphere's point all reach the image: a renderer that ignored one of
    them could not match the oracle."""
    base = _render(oracle, "zoo")

    def differs(z):
        got = oracle.render_pixels(z.scene(oracle), z.oracle_camera(oracle, NX, NY), NX, NY, SPP, DEPTH,
                                   np.arange(NX * NY, dtype=np.int64))
        return not (np.array_equal(got[0], base[0], equal_nan=True) and np.array_equal(got[1], base[1]))

    z = S.zoo()
    glass = [q for q, (_, m, _) in enumerate(z.quads) if S.MAT_TYPE[m] == 2][0]
    z.quads[glass][1:] = [1, 1]  # the pane in white
    assert differs(z)
    z = S.zoo()
    z.spheres[2][2:] = [1, 1]  # the emissive sphere in white
    assert differs(z)
    assert differs(S.ior(1.33))
    assert differs(S.light_sphere_elsewhere())
    # the kept repeats: lower indices win equal t, so swapping a pair's materials changes the image
    d = S.dups()
    d.quads[1][1:], d.quads[25][1:] = d.quads[25][1:], d.quads[1][1:]
    want = _render(oracle, "dups")
    got = oracle.render_pixels(d.scene(oracle), d.oracle_camera(oracle, NX, NY), NX, NY, SPP, DEPTH,
                               np.arange(NX * NY, dtype=np.int64))
    assert not np.array_equal(got[0], want[0], equal_nan=True)
