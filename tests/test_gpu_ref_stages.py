"""The HIP bounce and closest hit against what the reference's own worklet headers computed
(tests/golden/ref_stages.npz; tests/test_ref_stages.py holds the oracle to the same file).

rtp_debug_bounce runs the path kernel's bounce() -- the merged generators, the dielectric on precomputed
constants, dead_step's fast-forward -- once per ray, as depth 0 of a two-deep path, on the fixture's 4096 rays
and seeds of each scene.  Its record is compared bit for bit with the reference's state after PDFCosineWorklet,
mapped as _ref_cases.final_state states it:
  missed -> result 1, attenuation 1, emitted 0, the ray unchanged;
  light  -> result 2 (the reference's status 0), emitted[0], attenuation 1, the ray unchanged;
  else   -> result 0, attenuation[0], the scattered origin and direction;
  the seed after every draw of the depth (a dead ray's which and generator draws included), and the flag of an
  attenuation that is not finite.
The fixture keeps one 64-bit hash of that record per ray; where a ray differs, the message shows the oracle's
record of it (bit-identical to the reference's: test_ref_stages.py).

The hit stages need no kernel of their own: the fixture's quad cases' quads and 253 of its sphere cases' spheres
are set as scenes (the sphere cases' far origins with 5 spheres in a scene the device scans: the sphere BVH promises
the scan's hit only within two diagonals of the scene), and columns 3-5 of rtp_debug_closest_hit must be the minimum over the reference's recorded
per-primitive t within (0.001, FLT_MAX), a tie to the lower index.  (The device names a quad by its position in
its own table -- repeats dropped, grouped by kind: _scenes.kept_quads, _scenes.scan_order -- which is mapped back
to the scene's index here.)

Ray generation and whole frames (tests/golden/ref_frames.npz: the reference's Camera::RayGen and the whole sample and
depth loop of RenderCellsImpl over its worklets, run by the same driver).  rtp_debug_raygen reports the camera
constants the host derives for a launch and runs the render kernels' camera_ray once per (pixel, seed) row; both must
equal the reference's constructor constants and rays bit for bit, on every case camera and canvas.  The recorded
frames are rendered through device.render_pixels over every pixel, and one through the whole-canvas launches: rgb
sums, final seeds and live counts are compared with numbers the reference's own code produced, not the oracle's."""
from __future__ import annotations

import json

import numpy as np
import pytest

import _ref_cases as rc
import _scenes as S
from _util import set_scene_from_oracle

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32
WORDS = ("result", "emitted.x", "emitted.y", "emitted.z", "attenuation.x", "attenuation.y", "attenuation.z", "origin.x",
         "origin.y", "origin.z", "direction.x", "direction.y", "direction.z", "seed", "nonfinite")


@pytest.fixture(scope="module")
def fx():
    z = np.load(rc.FIXTURE, allow_pickle=False)
    g = {k: z[k] for k in z.files}
    g["meta"] = json.loads(str(g["meta"]))
    return g


@pytest.fixture(scope="module")
def scs(oracle):
    return rc.scenes(oracle)


@pytest.mark.parametrize("nm", rc.BOUNCE_SCENES)
def test_device_bounce_equals_the_reference(device, oracle, fx, scs, nm):
    rays, seeds = rc.bounce_rays(nm, scs[nm])
    assert rc.digest(rc.words(rays, seeds)) == fx["meta"]["cases_sha256"]["bounce_" + nm]
    try:
        set_scene_from_oracle(device, scs[nm])
        got = device.debug_bounce(rays, seeds)
    finally:
        device.set_cornell_box(0)
    got = rc.canonical(got, rc.FINAL_TYPES)
    bad = np.flatnonzero(rc.row_hashes(got) != fx[nm + "_final_hash"])
    if bad.size:
        rec = oracle.bounce(scs[nm], rays[bad[:64]], seeds[bad[:64]])
        want = rc.final_state(rc.canonical(rec.reshape(-1, rc.REC_WORDS), rc.REC_TYPES).reshape(rec.shape))
        words = sorted({WORDS[k] for k in np.nonzero(got[bad[:64]] != want)[1]})
        by = dict(zip(*np.unique(np.asarray(rc.OUTCOMES)[fx[nm + "_outcome"][bad]], return_counts=True)))
        i = bad[0]
        raise AssertionError(
            f"{nm}: {bad.size} of {len(rays)} rays differ from the reference ({by}) in {words}; ray {i} "
            f"{rays[i].tolist()} seed {int(seeds[i])}: got {got[i].tolist()} = {got[i, 1:13].view(F).tolist()}, "
            f"oracle {want[0].tolist()} = {want[0, 1:13].view(F).tolist()}")
    # the record covers what it is meant to: all three results, and paths that stored a non-finite attenuation
    assert {0, 1, 2} <= set(got[:, 0].tolist())
    assert np.isfinite(rays).all()


def test_device_bounce_meets_a_nonfinite_attenuation(device, oracle, fx, scs):
    """cornell1's glass sphere overlaps the tall box, so hit points lie inside the light sphere: the flag is set
    for some ray of that scene, and the reference's attenuation of it is NaN or infinite."""
    rays, seeds = rc.bounce_rays("cornell1", scs["cornell1"])
    try:
        set_scene_from_oracle(device, scs["cornell1"])
        got = device.debug_bounce(rays, seeds)
    finally:
        device.set_cornell_box(0)
    flagged = got[:, 14] == 1
    assert flagged.any()
    assert (~np.isfinite(got[flagged, 4:7].view(F))).any(1).all() and (got[flagged, 0] == 0).all()


@pytest.mark.parametrize("nm", ["hit_quads", "hit_spheres", "hit_spheres_far"])
def test_device_closest_hit_equals_the_reference_hits(device, oracle, fx, scs, nm):
    sc, rays, z = rc.hit_scenes(oracle, scs)[nm]
    kept, pairs = S.kept_quads(z), z.classify()
    scene_index = np.array([kept[q] for q in S.scan_order([pairs[q] for q in kept])], dtype=U)  # of a table position
    assert rc.digest(np.concatenate([rc.scene_words(sc), rays.view(U).reshape(-1)])) == fx["meta"]["cases_sha256"][nm]
    want = fx[nm]
    try:
        set_scene_from_oracle(device, sc)
        # 256 spheres are walked through the BVH; the far origins' 8 are scanned (the BVH is exact within two
        # diagonals of the scene only: include/rtp.h; 127 of the 256 far rays differed on it)
        assert (device.sphere_walk() == "scan") == (nm != "hit_spheres")
        got = device.debug_closest_hit(rays)
    finally:
        device.set_cornell_box(0)
    for what, cols in (("exact scan", got[:, 3:6].copy()), ("prefiltered", got[:, 0:3].copy())):
        quad = cols[:, 1] == 0
        assert (cols[quad, 2] < len(scene_index)).all()
        cols[quad, 2] = scene_index[cols[quad, 2]]
        bad = np.flatnonzero((cols != want).any(1))
        assert bad.size == 0, (
            f"{nm}, {what}: {bad.size} of {len(rays)} rays differ; ray {bad[0]} {rays[bad[0]].tolist()}: got (t "
            f"{cols[bad[0], 0:1].view(F)[0]!r}, kind {int(cols[bad[0], 1].astype(np.int32))}, index {int(cols[bad[0], 2])}), "
            f"reference (t {want[bad[0], 0:1].view(F)[0]!r}, kind {int(want[bad[0], 1].astype(np.int32))}, index "
            f"{int(want[bad[0], 2])})")
    kinds = set(want[:, 1].astype(np.int32).tolist())
    assert kinds >= {0, 1, -1}, kinds
    assert (want[:, 1] == 1).sum() >= rc.MIN_COVER


# ------------------------------------------------- ray generation and whole frames --
@pytest.fixture(scope="module")
def ffx():
    z = np.load(rc.FRAMES_FIXTURE, allow_pickle=False)
    g = {k: z[k] for k in z.files}
    g["meta"] = json.loads(str(g["meta"]))
    return g


def _camera(words):
    """The package's Camera from a case's first ten words (position, look-at, up, fov)."""
    import raytracingtherestofyourlife_amd as rtp

    cam = rtp.Camera()
    cam.SetPosition(words[0:3].view(F))
    cam.SetLookAt(words[3:6].view(F))
    cam.SetViewUp(words[6:9].view(F))
    cam.SetFieldOfView(float(words[9:10].view(F)[0]))
    return cam


def test_device_camera_constants_equal_the_reference(device, ffx):
    """Python Camera -> rtp_camera -> the host's camera_setup, for every case camera on every canvas: the eye is the
    position given, nlook, delta_x and delta_y are RayGen's constructor's, the signs of zeros included."""
    cases = rc.camera_cases()
    assert rc.digest(cases) == ffx["meta"]["cases_sha256"]["camera"]
    device.set_cornell_box(0)
    got = np.stack([device.debug_raygen(_camera(c), int(c[10]), int(c[11]), [], [])[0] for c in cases]).view(U)
    assert np.array_equal(got[:, :3], cases[:, :3])
    con = rc.canonical(got[:, 3:], "f" * 9)
    bad = np.flatnonzero((con != ffx["camera_out"]).any(1))
    assert bad.size == 0, (
        f"{bad.size} of {len(cases)} cameras differ; case {bad[0]} {cases[bad[0], :10].view(F).tolist()} on "
        f"{cases[bad[0], 10:12].tolist()}: got {con[bad[0]].view(F).tolist()}, reference "
        f"{ffx['camera_out'][bad[0]].view(F).tolist()}")


def test_device_raygen_equals_the_reference(device, ffx):
    """All 2048 rays of the render kernels' camera_ray, the seeds after its two draws and the pixel indices."""
    cases = rc.raygen_cases()
    assert rc.digest(cases) == ffx["meta"]["cases_sha256"]["raygen"]
    device.set_cornell_box(0)
    got = np.zeros((len(cases), 5), dtype=U)
    _, inv = np.unique(cases[:, :12], axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    for g in range(inv.max() + 1):  # one launch per (camera, canvas)
        rows = np.flatnonzero(inv == g)
        c = cases[rows[0]]
        got[rows] = device.debug_raygen(_camera(c), int(c[10]), int(c[11]), cases[rows, 12].astype(np.int64),
                                        cases[rows, 13])[1]
    got, want = rc.canonical(got, "fffui"), ffx["raygen_out"]
    bad = np.flatnonzero((got != want).any(1))
    nud = rc.raygen_nudged(cases, ffx["camera_out"])
    assert bad.size == 0, (
        f"{bad.size} of {len(cases)} rays differ ({int(nud[bad].any(1).sum())} of them nudged); case {bad[0]}: camera "
        f"{cases[bad[0], :10].view(F).tolist()} canvas {cases[bad[0], 10:12].tolist()} pixel {int(cases[bad[0], 12])} "
        f"seed {int(cases[bad[0], 13])}: got {got[bad[0], :3].view(F).tolist()} {got[bad[0], 3:].tolist()}, reference "
        f"{want[bad[0], :3].view(F).tolist()} {want[bad[0], 3:].tolist()}")
    assert (nud.sum(0) >= rc.MIN_COVER).all()


def _compare_frame(nm, ffx, rgba, seeds, live, how):
    rgb = rc.canonical(np.ascontiguousarray(rgba[:, :3], dtype=F).view(U), "fff")
    seeds, live = np.asarray(seeds).view(U), np.asarray(live).view(U)
    bad = np.flatnonzero((rgb != ffx[nm + "_rgb"]).any(1) | (seeds != ffx[nm + "_seed"]) | (live != ffx[nm + "_live"]))
    assert bad.size == 0, (
        f"{nm} through {how}: {bad.size} of {len(rgb)} pixels differ from the reference, first {bad[:4].tolist()}: rgb "
        f"{rgb[bad[0]].view(F).tolist()} seed {seeds[bad[0]]} live {live[bad[0]]}, reference "
        f"{ffx[nm + '_rgb'][bad[0]].view(F).tolist()} {ffx[nm + '_seed'][bad[0]]} {ffx[nm + '_live'][bad[0]]}")


@pytest.mark.parametrize("nm", list(rc.FRAMES))
def test_device_frame_equals_the_reference(device, ffx, scs, nm):
    """Every pixel of every recorded frame (1 x 1, depth 1, depth 2 and depth 50 among them) through
    rtp_render_pixels: rgb sums (NaN equals NaN), final seeds, live counts."""
    scn, cam, nx, ny, spp, depth = rc.FRAMES[nm]
    assert (rc.digest(np.concatenate([rc.scene_words(scs[scn]), rc.frame_case(nm)[0]]))
            == ffx["meta"]["cases_sha256"]["frame_" + nm])
    try:
        set_scene_from_oracle(device, scs[scn])
        rgba, seeds, live, _ = device.render_pixels(_camera(rc.frame_case(nm)[0]), nx, ny, spp, depth, np.arange(nx * ny))
    finally:
        device.set_cornell_box(0)
    _compare_frame(nm, ffx, rgba, seeds, live, "render_pixels")


@pytest.mark.parametrize("nm", ["cornell1", "cornell1_deep"])
def test_device_whole_canvas_launch_equals_the_reference(device, ffx, scs, nm):
    """The same through the whole-canvas launches: rtp_render into host memory (rgb) and rtp_render_device with the
    final seeds and live counts.  cornell1 has NaN pixels in the reference's own frame."""
    import torch

    scn, cam, nx, ny, spp, depth = rc.FRAMES[nm]
    n = nx * ny
    camera = _camera(rc.frame_case(nm)[0])
    out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    seeds = torch.zeros(n, dtype=torch.int32, device="cuda")
    live = torch.zeros(n, dtype=torch.int32, device="cuda")
    try:
        set_scene_from_oracle(device, scs[scn])
        host, _ = device.render(camera, nx, ny, spp, depth)
        device.render_device(camera, nx, ny, spp, depth, out.data_ptr(), seed_ptr=seeds.data_ptr(),
                             live_ptr=live.data_ptr())
        torch.cuda.synchronize()
    finally:
        device.set_cornell_box(0)
    _compare_frame(nm, ffx, out.cpu().numpy(), seeds.cpu().numpy(), live.cpu().numpy(), "render_device")
    _compare_frame(nm, ffx, host, ffx[nm + "_seed"], ffx[nm + "_live"], "render")
    assert np.isnan(ffx[nm + "_rgb"].view(F)).any()
