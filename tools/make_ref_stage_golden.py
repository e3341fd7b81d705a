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

A second file, tests/golden/ref_frames.npz, holds what the reference's code outside the worklet headers computes
(ref_stage_driver.cpp modes camera, raygen, seed_init, backward, frame):
  camera_out, raygen_out, seed_init_out, backward_<D>_<S>_out
                            those stages' results, full
  <frame>_rgb/_seed/_live   per pixel of a whole small frame: the canvas rgb bits, the final seed, and the depths
                            the ray entered with the scatter bit set
  <frame>_outcome           index into _ref_cases.FRAME_OUTCOMES per (sample, depth, ray)
  meta                      JSON: SHA-256 of every case array, SHA-256 of all rays' states after every depth of
                            every sample of every frame, the coverage counts
It is written with fixed zip timestamps, so the same driver gives the same bytes.

Generation fails if an outcome the issue lists has fewer than _ref_cases.MIN_COVER cases."""
from __future__ import annotations

import io
import json
import os
import sys
import zipfile

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


def save_npz(path, arrays):
    """An .npz np.load reads, byte for byte the same for the same arrays (np.savez stamps the time of day)."""
    with zipfile.ZipFile(path + ".tmp", "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())
    os.replace(path + ".tmp", path)


def frames(path=None):
    """tests/golden/ref_frames.npz"""
    scs = rc.scenes(oracle)
    sc = scs[rc.STAGE_SCENE]  # the stages of this file read no scene; the driver's file format carries one
    fx, meta = {}, {"cases_sha256": {}, "state_sha256": {}}
    for name, (_, _, types) in rc.FRAME_STAGES.items():
        if name == "backward":
            continue
        cases = rc.frame_stage_cases(name)
        meta["cases_sha256"][name] = rc.digest(cases)
        fx[name + "_out"] = rc.canonical(rc.driver_frame_stage(name, sc, cases), types)
    for d, s in rc.BACKWARD_SHAPES:
        cases = rc.backward_cases(d, s)
        meta["cases_sha256"][f"backward_{d}_{s}"] = rc.digest(cases)
        fx[f"backward_{d}_{s}_out"] = rc.canonical(rc.driver_frame_stage("backward", sc, cases), "ffff")
    for nm, (scn, _, nx, ny, spp, depth) in rc.FRAMES.items():
        meta["cases_sha256"]["frame_" + nm] = rc.digest(np.concatenate([rc.scene_words(scs[scn]), rc.frame_case(nm)[0]]))
        pix, states = rc.driver_frame(nm, scs)
        fx[nm + "_rgb"] = rc.canonical(pix[:, :3], "fff")
        fx[nm + "_seed"], fx[nm + "_live"] = pix[:, 3].copy(), pix[:, 4].copy()
        meta["state_sha256"][nm] = rc.state_digests(states)
        fx[nm + "_outcome"] = rc.frame_outcomes(scs[scn], states)
    meta["coverage"] = {**rc.frame_coverage(fx), **rc.frame_stage_coverage(fx)}
    print(json.dumps(meta["coverage"], indent=1))
    low = {k: v for k, v in meta["coverage"].items() if v < rc.MIN_COVER}
    if low:
        sys.exit(f"coverage: fewer than {rc.MIN_COVER} cases of {low}")
    if int(fx["seed_init_out"][0, 0]) == 0:
        sys.exit("WangInit(1) is 0: CopyIf would copy no seed")
    fx["meta"] = np.array(json.dumps(meta, sort_keys=True))
    path = path or rc.FRAMES_FIXTURE
    save_npz(path, fx)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if not os.path.exists(rc.REF_STAGES):
        sys.exit(f"{rc.REF_STAGES} is missing: build it where the reference tree is (raytracingtherestofyourlife_amd/build.py)")
    if "--frames-only" not in sys.argv:
        main()
    frames()
