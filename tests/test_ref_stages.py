"""The oracle against what the reference's own worklet headers computed.

tests/golden/ref_stages.npz holds results of oracle/_ref/ref_stages (the reference's PdfWorklet.h, EmitWorklet.h,
ScatterWorklet.h, SurfaceWorklets.h, Surface.h, onb.h, wangXor.h and vec3.h, compiled unchanged over
tests/cpp/vtkm_min by tests/cpp/ref_stage_driver.cpp) on the cases of tests/_ref_cases.py: every stage function
on 2048 cases, and the state of 4096 rays of five scenes after each of the thirteen worklets of one depth of
RenderCellsImpl.  Every stage export of oracle/rtp_oracle.c and rtpo_bounce must reproduce them bit for bit (NaN
equals NaN).  Where oracle/_ref/ref_stages exists it is run again and held to the same file.

tests/golden/ref_frames.npz holds what the reference's code outside those headers computes: Camera::RayGen
(pathtracing/Camera.cxx; its constructor's camera constants and its operator()), details::WangInit
(MapperPathTracer.cxx), the backward product through PathAlgorithms.h's BinarySliceTransformIdxKernel, and whole small
frames: the sample and depth loop of RenderCellsImpl:278-354 with every array kept from depth to depth and from
sample to sample.  rtpo_camera_setup, rtpo_stage_raygen, rtpo_stage_backward, rtpo_render_pixels and
rtpo_render_soa (every ray's state after every depth of every sample) must reproduce them bit for bit."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import _ref_cases as rc

F, U = np.float32, np.uint32
_memo = {}


@pytest.fixture(scope="module")
def fx():
    z = np.load(rc.FIXTURE, allow_pickle=False)
    g = {k: z[k] for k in z.files}
    g["meta"] = json.loads(str(g["meta"]))
    return g


@pytest.fixture(scope="module")
def scs(oracle):
    return rc.scenes(oracle)


def _cases(name, scs, fx):
    if name not in _memo:
        _memo[name] = rc.stage_cases(name, scs, fx)
    return _memo[name]


def _rays(name, scs):
    if ("rays", name) not in _memo:
        _memo["rays", name] = rc.bounce_rays(name, scs[name])
    return _memo["rays", name]


def test_the_cases_are_the_recorded_ones(fx, scs, oracle):
    """The fixture stores the reference's results and a digest of each case array; the arrays are rebuilt here."""
    want = fx["meta"]["cases_sha256"]
    got = {name: rc.digest(_cases(name, scs, fx)) for name in rc.STAGES}
    got.update({"bounce_" + nm: rc.digest(rc.words(*_rays(nm, scs))) for nm in rc.BOUNCE_SCENES})
    got.update({nm: rc.digest(np.concatenate([rc.scene_words(sc), rays.view(U).reshape(-1)]))
                for nm, (sc, rays, _) in rc.hit_scenes(oracle, scs).items()})
    assert got == want


def _compare_stage(name, got, fx, cases):
    types = rc.STAGES[name][2]
    got, want = rc.canonical(got, types), fx[name + "_out"]
    assert got.shape == want.shape == (rc.N_STAGE, len(types))
    bad = np.flatnonzero((got != want).any(1))
    if bad.size:
        i = bad[0]
        cols = sorted(set(np.nonzero(got != want)[1].tolist()))
        raise AssertionError(
            f"{name}: {bad.size} of {len(got)} cases differ from the reference in result words {cols}; case {i}: "
            f"words {cases[i].tolist()} (as floats {cases[i].view(F).tolist()}): got {got[i].tolist()} "
            f"{got[i].view(F).tolist()}, reference {want[i].tolist()} {want[i].view(F).tolist()}")


@pytest.mark.parametrize("name", list(rc.STAGES))
def test_oracle_stage_equals_the_reference(oracle, fx, scs, name):
    cases = _cases(name, scs, fx)
    _compare_stage(name, oracle.stage(name, scs[rc.STAGE_SCENE], cases), fx, cases)


def _compare_bounce(nm, rec, fx, scs):
    rays, seeds = _rays(nm, scs)
    can = rc.canonical(rec.reshape(-1, rc.REC_WORDS), rc.REC_TYPES).reshape(len(rays), len(rc.PASSES), rc.REC_WORDS)
    got = [rc.digest(can[:, c]) for c in range(len(rc.PASSES))]
    want = fx["meta"]["pass_sha256"][nm]
    bad_rays = np.flatnonzero(rc.row_hashes(can.reshape(len(can), -1)) != fx[nm + "_ray_hash"])
    first = next((rc.PASSES[c] for c in range(len(got)) if got[c] != want[c]), None)
    assert first is None and bad_rays.size == 0, (
        f"{nm}: the state after {first} is the first to differ from the reference's; {bad_rays.size} rays differ, "
        f"first {bad_rays[:4].tolist()}: rays {rays[bad_rays[:2]].tolist()} seeds {seeds[bad_rays[:2]].tolist()}")
    assert np.array_equal(rc.row_hashes(rc.final_state(can)), fx[nm + "_final_hash"])
    assert np.array_equal(rc.bounce_outcomes(scs[nm], can), fx[nm + "_outcome"])


@pytest.mark.parametrize("nm", rc.BOUNCE_SCENES)
def test_oracle_bounce_equals_the_reference(oracle, fx, scs, nm):
    """Every ray's status, hit and scatter records, which, generated direction, sum_value, emitted[0],
    attenuation[0], origin, direction and seed after each worklet of one depth."""
    rays, seeds = _rays(nm, scs)
    _compare_bounce(nm, oracle.bounce(scs[nm], rays, seeds), fx, scs)


def test_coverage(fx, scs):
    """Every outcome the fixture was built to reach is in the committed file, counted from the reference's results."""
    cov = rc.coverage(fx, scs)
    assert cov == fx["meta"]["coverage"]
    low = {k: v for k, v in cov.items() if v < rc.MIN_COVER}
    assert not low, low
    assert set(cov) >= {"missed", "light_front", "light_behind", "lambertian_cosine", "lambertian_quad",
                        "lambertian_sphere", "dielectric_reflected_schlick", "dielectric_refracted",
                        "dielectric_total_internal", "de_nan_changed", "quad_pdf_zero", "quad_pdf_nonzero",
                        "sphere_pdf_zero", "sphere_pdf_nonzero", "quad_hit_axis0", "quad_hit_axis1", "quad_hit_axis2",
                        "quad_hit_bilinear0", "quad_hit_bilinear1", "quad_hit_bilinear2", "quad_hit_first_triangle",
                        "quad_hit_second_triangle", "quad_hit_det_below_eps", "quad_hit_det_above_eps",
                        "quad_hit_t_below_tmin", "quad_hit_t_above_tmin", "quad_hit_t_below_tmax",
                        "quad_hit_t_beyond_tmax", "sphere_hit_second_root"}


def test_dielectric_cases_straddle_reflect_prob(fx, scs):
    """_rand one ulp below the recorded reflect_prob is reflected, at it and above it is not, and a double between
    the two floats below it is reflected: only a comparison in double tells that one from reflect_prob."""
    cases = _cases("dielectric_scatter", scs, fx)
    bits = cases[:, 9].astype(np.uint64) | (cases[:, 10].astype(np.uint64) << np.uint64(32))
    rnd = bits.view(np.float64)
    th = fx["dielectric_thresholds"].astype(np.float64)
    cls = fx["dielectric_class"]
    tir = th >= 1.0
    assert ((cls == 2) == tir).all()
    assert (cls[~tir & (rnd < th)] == 0).all() and (cls[~tir & (rnd >= th)] == 1).all()
    between = ~tir & (rnd < th) & (rnd.astype(F).astype(np.float64) == th)
    assert between.sum() >= rc.MIN_COVER and (cls[between] == 0).all()


# ------------------------------------ ray generation, backward product, frames --
@pytest.fixture(scope="module")
def ffx():
    z = np.load(rc.FRAMES_FIXTURE, allow_pickle=False)
    g = {k: z[k] for k in z.files}
    g["meta"] = json.loads(str(g["meta"]))
    return g


def _frame_case_digests(scs):
    got = {name: rc.digest(rc.frame_stage_cases(name)) for name in rc.FRAME_STAGES if name != "backward"}
    got.update({f"backward_{d}_{s}": rc.digest(rc.backward_cases(d, s)) for d, s in rc.BACKWARD_SHAPES})
    got.update({"frame_" + nm: rc.digest(np.concatenate([rc.scene_words(scs[f[0]]), rc.frame_case(nm)[0]]))
                for nm, f in rc.FRAMES.items()})
    return got


def test_the_frame_cases_are_the_recorded_ones(ffx, scs):
    assert _frame_case_digests(scs) == ffx["meta"]["cases_sha256"]
    assert len(rc.raygen_cases()) == rc.N_STAGE
    assert {tuple(c[10:12].tolist()) for c in rc.camera_cases()} == set(rc.CANVASES)
    big = rc.raygen_cases()
    big = big[(big[:, 10] == rc.CORNERS_ONLY[0]) & (big[:, 11] == rc.CORNERS_ONLY[1])]
    n = rc.CORNERS_ONLY[0]
    assert set(big[:, 12].tolist()) == {0, n - 1, n * (n - 1), n * n - 1}  # an index of 2^28 - 1 among them


def _compare_rows(what, got, want, types, cases, cols=None):
    got, want = rc.canonical(got, types), np.asarray(want)
    assert got.shape == want.shape
    if cols is not None:
        got, want = got[:, cols], want[:, cols]
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, (
        f"{what}: {bad.size} of {len(got)} cases differ from the reference; case {bad[0]}: words "
        f"{cases[bad[0]][:16].tolist()} (as floats {cases[bad[0]][:16].view(F).tolist()}): got {got[bad[0]].tolist()} "
        f"{got[bad[0]].view(F).tolist()}, reference {want[bad[0]].tolist()} {want[bad[0]].view(F).tolist()}")


def _oracle_camera(oracle, row):
    return oracle.camera_setup(int(row[10]), int(row[11]), row[0:3].view(F), row[3:6].view(F), row[6:9].view(F),
                               row[9:10].view(F)[0])


def test_oracle_camera_constants_equal_the_reference(oracle, ffx):
    """nlook, delta_x and delta_y of RayGen's constructor under CreateRaysImpl's arguments, the signs of zeros
    included; the oracle's first three constants are the position it was given."""
    cases = rc.camera_cases()
    got = np.stack([_oracle_camera(oracle, c) for c in cases])
    assert np.array_equal(got[:, :3].view(U), cases[:, :3])
    _compare_rows("camera", got[:, 3:].view(U), ffx["camera_out"], "f" * 9, cases)


def test_oracle_raygen_equals_the_reference(oracle, ffx):
    """Direction, seed after and pixel index of all 2048 rays."""
    cases = rc.raygen_cases()
    _compare_rows("raygen", oracle.stage_raygen(cases), ffx["raygen_out"], "fffui", cases)


def test_wang_init_copies_every_seed(ffx):
    """CopyIf(counting, constant 1, seeds, WangInit()) (MapperPathTracer.cxx:265-267): WangInit is the predicate and
    sees the stencil value 1; its value is not zero, so every index is copied and seed0 = pixel."""
    assert ffx["seed_init_out"].shape == (1, 1) and int(ffx["seed_init_out"][0, 0]) != 0


@pytest.mark.parametrize("d,s", rc.BACKWARD_SHAPES)
def test_oracle_backward_product_equals_the_reference(oracle, ffx, d, s):
    """rgb of the canvas after S samples of D planes.  The fourth lane is not compared: the reference multiplies and
    adds buffers there (alphaChannelAE, alphaChannel) that nothing in it writes or reads otherwise."""
    cases = rc.backward_cases(d, s)
    _compare_rows(f"backward D={d} S={s}", oracle.stage_backward(cases), ffx[f"backward_{d}_{s}_out"], "ffff", cases,
                  cols=[0, 1, 2])


def _compare_frame(nm, ffx, rgba, seeds, live, states=None):
    _, _, nx, ny, spp, depth = rc.FRAMES[nm]
    if states is not None:  # first, so that a mismatch names where it starts
        got, want = rc.state_digests(states), ffx["meta"]["state_sha256"][nm]
        first = next(((s, d) for s in range(spp) for d in range(depth) if got[s][d] != want[s][d]), None)
        assert first is None, f"{nm}: the rays' states first differ from the reference's after sample {first[0]}, depth {first[1]}"
    rgb = rc.canonical(np.ascontiguousarray(rgba[:, :3], dtype=F).view(U), "fff")
    bad = np.flatnonzero((rgb != ffx[nm + "_rgb"]).any(1) | (seeds != ffx[nm + "_seed"]) | (live != ffx[nm + "_live"]))
    assert bad.size == 0, (
        f"{nm}: {bad.size} of {nx * ny} pixels differ from the reference, first {bad[:4].tolist()}: rgb "
        f"{rgb[bad[0]].view(F).tolist()} seed {seeds[bad[0]]} live {live[bad[0]]}, reference "
        f"{ffx[nm + '_rgb'][bad[0]].view(F).tolist()} {ffx[nm + '_seed'][bad[0]]} {ffx[nm + '_live'][bad[0]]}")


def _frame_camera(oracle, nm):
    _, cam, nx, ny, _, _ = rc.FRAMES[nm]
    return _oracle_camera(oracle, rc.camera_words(rc.cameras()[cam], nx, ny))


@pytest.mark.parametrize("nm", list(rc.FRAMES))
def test_oracle_frame_equals_the_reference(oracle, ffx, scs, nm):
    """rtpo_render_pixels over every pixel: rgb sums, final seeds and live counts; rtpo_render_soa: the same, and
    every ray's state after every depth of every sample."""
    scn, _, nx, ny, spp, depth = rc.FRAMES[nm]
    cam = _frame_camera(oracle, nm)
    rgba, seeds, live = oracle.render_pixels(scs[scn], cam, nx, ny, spp, depth, np.arange(nx * ny), nthreads=1)
    _compare_frame(nm, ffx, rgba, seeds, live)
    rgba, seeds, live, states = oracle.render_soa_states(scs[scn], cam, nx, ny, spp, depth)
    _compare_frame(nm, ffx, rgba, seeds, live, states)


def test_frame_coverage(ffx):
    """Counted again from the committed file: ray-depths of every outcome, samples that start where the sample before
    died early, rays whose direction is nudged in each component, draws of exactly 0 and exactly 1.0f."""
    cov = {**rc.frame_coverage(ffx), **rc.frame_stage_coverage(ffx)}
    assert cov == ffx["meta"]["coverage"]
    low = {k: v for k, v in cov.items() if v < rc.MIN_COVER}
    assert not low, low
    assert set(cov) >= set(rc.FRAME_OUTCOMES) | {"sample_after_early_death", "raygen_nudged_x", "raygen_nudged_y",
                                                  "raygen_nudged_z", "raygen_first_draw_0", "raygen_first_draw_1",
                                                  "raygen_second_draw_0", "raygen_second_draw_1"}
    for nm, (_, _, nx, ny, spp, depth) in rc.FRAMES.items():
        oc = ffx[nm + "_outcome"]
        assert oc.shape == (spp, depth, nx * ny)
        assert np.array_equal((oc != 7).sum((0, 1)), ffx[nm + "_live"])  # the live count is the reference's own
    shapes = {(f[2] * f[3], f[5]) for f in rc.FRAMES.values()}
    assert {d for _, d in shapes} >= {1, 2, 8, 50} and (1, 8) in shapes


def test_the_nudge_changes_the_recorded_rays(ffx):
    """The reference's nudged rays are not what a generator without the nudge would give: the component that was
    zero comes out as 1e-7 / |ray_dir|, not 0."""
    nud = rc.raygen_nudged(rc.raygen_cases(), ffx["camera_out"])
    d = ffx["raygen_out"][:, :3].view(F)
    assert (d[nud] > 0).all() and (d[nud] < 2e-7).all()


def test_recipe_cuts_one_class_by_anchor_and_braces():
    """oracle/ref_build.py cut_class on a text of its own: the class from its anchor line to the closing brace and
    semicolon, braces in comments, strings and character literals not counted; a missing anchor, one that matches
    twice and braces that do not close are errors."""
    import ref_build

    text = ("struct Before { int a; };\nclass Outer::Inner : public Base\n{\n  // a brace in a comment: }\n"
            "  /* and here } } */ const char* s = \"}{\"; char c = '}';\n  void f() { if (s) { g(); } }\n}\n;\n"
            "class Outer::Other {};\nint after;\n")
    cut = ref_build.cut_class(text, r"^\s*class\s+Outer::Inner\b")
    assert cut.lstrip().startswith("class Outer::Inner") and cut.rstrip().endswith("}\n;") and "after" not in cut
    assert "Other" not in cut and "void f() { if (s) { g(); } }" in cut
    with pytest.raises(RuntimeError, match="matches 0 lines"):
        ref_build.cut_class(text, r"^\s*class\s+Outer::Missing\b")
    with pytest.raises(RuntimeError, match="matches 2 lines"):
        ref_build.cut_class(text, r"^\s*class\s+Outer::")
    with pytest.raises(RuntimeError, match="do not close"):
        ref_build.cut_class("struct Before { int a;", r"^\s*struct\s+Before\b")
    assert set(ref_build.REF_CUTS) == {"camera_raygen.inc", "wang_init.inc"}


# ------------------------------------------------------- the live driver --
@pytest.fixture(scope="module")
def ref_stages():
    if not os.path.exists(rc.REF_STAGES):
        pytest.skip("the reference's worklet headers are absent and no prebuilt oracle/_ref/ref_stages exists")
    return rc.REF_STAGES


@pytest.mark.parametrize("name", list(rc.STAGES))
def test_live_driver_stage_equals_the_fixture(ref_stages, fx, scs, name):
    cases = _cases(name, scs, fx)
    _compare_stage(name, rc.driver_stage(name, scs[rc.STAGE_SCENE], cases, ref_stages), fx, cases)


@pytest.mark.parametrize("nm", rc.BOUNCE_SCENES)
def test_live_driver_bounce_equals_the_fixture(ref_stages, fx, scs, nm):
    rays, seeds = _rays(nm, scs)
    _compare_bounce(nm, rc.driver_bounce(scs[nm], rays, seeds, ref_stages), fx, scs)


@pytest.mark.parametrize("name", [n for n in rc.FRAME_STAGES if n != "backward"])
def test_live_driver_frame_stage_equals_the_fixture(ref_stages, ffx, scs, name):
    cases = rc.frame_stage_cases(name)
    types = rc.FRAME_STAGES[name][2]
    _compare_rows(name, rc.driver_frame_stage(name, scs[rc.STAGE_SCENE], cases, ref_stages), ffx[name + "_out"], types,
                  cases)


@pytest.mark.parametrize("d,s", rc.BACKWARD_SHAPES)
def test_live_driver_backward_equals_the_fixture(ref_stages, ffx, scs, d, s):
    cases = rc.backward_cases(d, s)
    _compare_rows(f"backward D={d} S={s}", rc.driver_frame_stage("backward", scs[rc.STAGE_SCENE], cases, ref_stages),
                  ffx[f"backward_{d}_{s}_out"], "ffff", cases)


@pytest.mark.parametrize("nm", list(rc.FRAMES))
def test_live_driver_frame_equals_the_fixture(ref_stages, ffx, scs, nm):
    pix, states = rc.driver_frame(nm, scs, ref_stages)
    _compare_frame(nm, ffx, pix[:, :3].view(F), pix[:, 3], pix[:, 4], states)
    assert np.array_equal(rc.frame_outcomes(scs[rc.FRAMES[nm][0]], states), ffx[nm + "_outcome"])
