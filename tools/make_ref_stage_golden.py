#!/usr/bin/env python3
"""Record tests/golden/ref_stages.npz: what the reference's own worklet headers compute
(oracle/_ref/ref_stages, built from tests/cpp/ref_stage_driver.cpp where the reference tree
exists) on the cases of tests/_ref_cases.py.  Host only; a few seconds.

The file holds results of the reference's programs and what identifies their inputs, nothing else:
  <stage>_out               every stage's results, full: (2048, kout) words, NaNs canonical
  dielectric_thresholds     reflect_prob of each dielectric geometry as the reference decides it
                            (bisection on _rand); the cases are built from them
  dielectric_class          0 reflected by Schlick, 1 refracted, 2 total internal reflection
  <scene>_ray_hash          one 64-bit hash per ray of its state after all thirteen worklets of a depth
  <scene>_final_hash        ... of what rtp_debug_bounce reports for the ray (_ref_cases.final_state)
  <scene>_outcome           index into _ref_cases.OUTCOMES per ray
  hit_quads / hit_spheres   the expected closest hit of the hit stages' rays in the two hit scenes
  meta                      JSON: SHA-256 of every case array (the tests rebuild the cases and check
                            them against these), SHA-256 of every scene's state after each worklet,
                            the coverage counts
A 37-word state after each of 13 worklets for 5 x 4096 rays is 39 MB; digests per worklet and
hashes per ray keep the comparison bit for bit, name the stage and the ray of a mismatch, and fit
the repository's size limit.

Generation fails if an outcome the issue lists has fewer than _ref_cases.MIN_COVER cases."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import _ref_cases as rc  # noqa: E402
import oracle_ctypes as oracle  # noqa: E402

F, U = np.float32, np.uint32


def bisect_thresholds(sc):
    """reflect_prob per geometry: the smallest float32 _rand that is NOT reflected (`_rand < reflect_prob`,
    EmitWorklet.h:209), found from the reference's outputs alone.  A reflected case repeats the direction of
    _rand = 0 (always reflected: reflect_prob >= r0 > 0)."""
    n = rc.N_STAGE
    d0 = rc.driver_stage("dielectric_scatter", sc, rc.dielectric_probe(np.zeros(n, dtype=F)))[:, 3:6]
    one = np.ones(1, dtype=F).view(np.int32)[0]
    lo, hi = np.zeros(n, dtype=np.int64), np.full(n, one, dtype=np.int64)  # bit patterns: lo reflected, hi not (1.0 never is)
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        out = rc.driver_stage("dielectric_scatter", sc, rc.dielectric_probe(mid.astype(np.int32).view(F)))[:, 3:6]
        refl = (out == d0).all(1)
        lo, hi = np.where(refl, mid, lo), np.where(refl, hi, mid)
    return hi.astype(np.int32).view(F)


def main():
    if not os.path.exists(rc.REF_STAGES):
        sys.exit(f"{rc.REF_STAGES} is missing: build it where the reference tree is (raytracingtherestofyourlife_amd/build.py)")
    scs = rc.scenes(oracle)
    sc = scs[rc.STAGE_SCENE]
    fx, meta = {}, {"cases_sha256": {}, "pass_sha256": {}}
    th = bisect_thresholds(sc)
    fx["dielectric_thresholds"] = th
    for name, (_, _, types, _) in rc.STAGES.items():
        cases = rc.stage_cases(name, scs, fx)
        assert cases.shape == (rc.N_STAGE, rc.STAGES[name][1]), name
        meta["cases_sha256"][name] = rc.digest(cases)
        fx[name + "_out"] = rc.canonical(rc.driver_stage(name, sc, cases), types)
    # the dielectric's classes: the direction of _rand = 0 is the reflected one
    cases = rc.stage_cases("dielectric_scatter", scs, fx)
    d0 = rc.driver_stage("dielectric_scatter", sc, rc.dielectric_probe(np.zeros(rc.N_STAGE, dtype=F)))[:, 3:6]
    refl = (fx["dielectric_scatter_out"][:, 3:6] == rc.canonical(d0, "fff")).all(1)
    fx["dielectric_class"] = np.where(th >= 1.0, 2, np.where(refl, 0, 1)).astype(np.int8)
    for nm in rc.BOUNCE_SCENES:
        rays, seeds = rc.bounce_rays(nm, scs[nm])
        meta["cases_sha256"]["bounce_" + nm] = rc.digest(rc.words(rays, seeds))
        rec = rc.driver_bounce(scs[nm], rays, seeds)
        can = rc.canonical(rec.reshape(-1, rc.REC_WORDS), rc.REC_TYPES).reshape(rec.shape)
        meta["pass_sha256"][nm] = [rc.digest(can[:, c]) for c in range(len(rc.PASSES))]
        fx[nm + "_ray_hash"] = rc.row_hashes(can.reshape(len(can), -1))
        fx[nm + "_final_hash"] = rc.row_hashes(rc.final_state(can))
        fx[nm + "_outcome"] = rc.bounce_outcomes(scs[nm], can)
    for nm, (hsc, rays, _) in rc.hit_scenes(oracle, scs).items():
        meta["cases_sha256"][nm] = rc.digest(np.concatenate([rc.scene_words(hsc), rays.view(U).reshape(-1)]))
        fx[nm] = rc.reference_closest_hits(hsc, rays)
    meta["coverage"] = rc.coverage(fx, scs)
    low = {k: v for k, v in meta["coverage"].items() if v < rc.MIN_COVER}
    print(json.dumps(meta["coverage"], indent=1))
    if low:
        sys.exit(f"coverage: fewer than {rc.MIN_COVER} cases of {low}")
    fx["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(rc.FIXTURE, **fx)
    print(rc.FIXTURE, os.path.getsize(rc.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
