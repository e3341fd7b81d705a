"""The oracle against what the reference's own worklet headers computed.

tests/golden/ref_stages.npz holds results of oracle/_ref/ref_stages (the reference's PdfWorklet.h, EmitWorklet.h,
ScatterWorklet.h, SurfaceWorklets.h, Surface.h, onb.h, wangXor.h and vec3.h, compiled unchanged over
tests/cpp/vtkm_min by tests/cpp/ref_stage_driver.cpp) on the cases of tests/_ref_cases.py: every stage function
on 2048 cases, and the state of 4096 rays of five scenes after each of the thirteen worklets of one depth of
RenderCellsImpl.  Every stage export of oracle/rtp_oracle.c and rtpo_bounce must reproduce them bit for bit (NaN
equals NaN).  Where oracle/_ref/ref_stages exists it is run again and held to the same file."""
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
