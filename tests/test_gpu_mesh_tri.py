"""Triangle cells of a mesh scene on the GPU (include/rtp_mesh.h: a cell whose
v11 and v01 compare equal, in particular (a, b, c, c)), on the scenes of
tests/_trimeshes.py: the walk (in a -DRTP_MESH_TRI_TEST=1 build with its
first-triangle test of a marked cell; the results are the same either way)
against the device's brute-force scan ray by ray; scan and walk against the
oracle's rtpo_bounce in all 15 words; small frames against the live oracle;
the device build against the host build -- pads, boxes, records, guarantee,
counts, pixels, bit for bit; the stealing and the resuming pool instances; a
65 536-cell triangle terrain beyond the oracle; and the mapper.

The checks are those of tests/test_gpu_mesh.py and tests/test_gpu_mesh_device.py
(the same promise, the same 1% cap outside the grazing part), called on the new
scenes, which tests/_trimeshes.py registers in _meshes.SCENES."""
from __future__ import annotations


import numpy as np
import pytest

import _meshes
import _scenes
import _trimeshes as T
import test_gpu_mesh as tgm
import test_gpu_mesh_device as tgd
from _adaptive_ref import active_ref, noise_ref
from _util import assert_render_equal

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
SCENES = ("hills_tri", "mixed", "slivers")
NX, NY, SPP, DEPTH = 24, 16, 4, 8
KIND_TRI = -1  # rtp_layout.hpp kMeshKindTri
DEVQUAD = np.dtype([("vv", F, 6), ("e01", F, 3), ("e03", F, 3), ("key_lo", U), ("para", np.int32), ("orig", np.int32),
                    ("kind", np.int32), ("e21", F, 3), ("e23", F, 3), ("n", F, 3), ("alb", F, 3), ("mt", np.int32),
                    ("pad", np.int32, 3)])
assert DEVQUAD.itemsize == 128


@pytest.fixture(scope="module")
def rtp():
    import raytracingtherestofyourlife_amd as rtp

    return rtp


@pytest.fixture(autouse=True)
def _leave_the_cornell_box(device):
    yield
    device.set_cornell_box(0)


def _records(device, nq):
    """rtp_debug_mesh_records: the stored DevQuads, sorted by the caller's index."""
    rec = np.zeros(nq, dtype=DEVQUAD)
    assert device._L.rtp_debug_mesh_records(device.handle, nq, rec.ctypes.data) == 0, device._L.rtp_last_error()
    assert np.array_equal(np.sort(rec["orig"]), np.arange(nq))
    return rec[np.argsort(rec["orig"])]


# 7 ------------------------------------- walk against scan, both against the oracle --
@pytest.mark.parametrize("name", SCENES)
def test_walk_equals_device_scan(device, name):
    out, _ = tgm._walk_equals_scan(device, name, _meshes.N_RAYS)
    kinds = set(out[:, 4].view(np.int32).tolist())
    assert kinds == {-1, 0, 1}, "misses, quad hits and sphere hits all occur"
    # triangle cells win hits, and so do the scene's quads
    m = tgm._mesh(name)
    win = tgm._scan_winner(out)
    tri = T.is_triangle(m)[np.maximum(win, 0)] & (win >= 0)
    assert tri.sum() > 4096 and ((win >= 0) & ~tri).sum() > 4096


@pytest.mark.parametrize("name", SCENES)
def test_bounce_equals_oracle(device, oracle, monkeypatch, name):
    tgm.test_bounce_equals_oracle(device, oracle, monkeypatch, name)


# 8 ------------------------------------------- renders against the live oracle --
@pytest.mark.parametrize("cam", tgm.CAMS)
@pytest.mark.parametrize("name", SCENES)
def test_render_equals_oracle(device, oracle, rtp, name, cam):
    tgm.test_render_equals_oracle(device, oracle, rtp, name, cam)


# 9 ----------------------------------------------- device build against host build --
@pytest.mark.parametrize("name", SCENES)
def test_device_build_equals_host_build(device, rtp, name):
    m = tgm._mesh(name)
    nq = len(m.quads)
    want = _meshes.build_host(m)
    tri = T.is_triangle(m)
    counts = (nq, int(tri.sum()), int((want["pads"] == T.HUGE).sum()))
    cam = m.camera(rtp)
    pix = np.arange(NX * NY, dtype=np.int64)
    # the host build
    g_host = tgd._set_host(device, m)
    assert device.mesh_counts() == counts
    rb_host, rec_host = tgd._readback(device, nq), _records(device, nq)
    px_host = device.render_pixels(cam, NX, NY, SPP, DEPTH, pix)[:3]
    # the device build
    g_dev = tgd._set_dev(device, m)
    assert device.mesh_counts() == counts
    rb_dev, rec_dev = tgd._readback(device, nq), _records(device, nq)
    px_dev = device.render_pixels(cam, NX, NY, SPP, DEPTH, pix)[:3]
    bits = tgd._bits
    assert bits(F(g_dev)).tolist() == bits(F(g_host)).tolist() == bits(F((want["cos_min"], want["reach"]))).tolist()
    for got in (rb_host, rb_dev):
        bad = np.flatnonzero(bits(got["pads"]) != bits(want["pads"]))
        assert bad.size == 0, f"{name}: {bad.size} pads differ, first {bad[:4].tolist()}: {got['pads'][bad[:4]]} " \
                              f"against {want['pads'][bad[:4]]}"
        bad = np.flatnonzero((bits(got["boxes"]) != bits(want["boxes"])).any(1))
        assert bad.size == 0, f"{name}: {bad.size} boxes differ, first {bad[:4].tolist()}"
    # the records, whole: the same 128 bytes per cell from both builders, a triangle cell marked, e23 == 0 kept
    bad = np.flatnonzero((rec_host.view(np.uint8).reshape(nq, 128) != rec_dev.view(np.uint8).reshape(nq, 128)).any(1))
    assert bad.size == 0, f"{name}: {bad.size} records differ, first {bad[:4].tolist()}: {rec_host[bad[:1]]} {rec_dev[bad[:1]]}"
    assert np.array_equal(rec_dev["kind"] == KIND_TRI, tri)
    assert (rec_dev["e23"][tri] == 0).all() and (rec_dev["key_lo"] == np.arange(nq)).all()
    assert_render_equal(px_dev, px_host, f"{name}: device build against host build")
    if name == "hills_tri":
        assert counts == (1805, 1800, 0)
    if name == "slivers":
        assert counts[2] == int((T.sliver_sines() < T.MIN_SINE).sum()) > 4
    tgd._check_structure(device, m, tgd._leaf_size(device))


def test_three_ids_a_row_give_the_same_scene(device, rtp):
    import torch

    m = T.hills_tri()
    tri = T.is_triangle(m)
    only = _meshes.Mesh(m.points, m.quads[tri], m.quad_mat[tri], m.quad_tex[tri], m.spheres, m.mat_type, m.tex_type,
                        m.tex, m.light, m.light_sphere_point, m.ior, m.cam)
    nq = len(only.quads)
    cam = only.camera(rtp)
    pix = np.arange(NX * NY, dtype=np.int64)
    tgd._set_dev(device, only)
    want = (tgd._readback(device, nq), _records(device, nq), device.render_pixels(cam, NX, NY, SPP, DEPTH, pix)[:3])
    assert device.mesh_counts() == (1800, 1800, 0)
    # [N, 3] tensors, expanded on the device
    pts, cells, mat, tex = tgd._tensors(only)
    three = cells[:, :3].contiguous()
    assert three.shape == (1800, 3) and three.is_cuda
    for stream in (None, torch.cuda.Stream()):
        device.set_cornell_box(0)
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        device.set_scene_mesh_device(pts, three, mat, tex, *only.set_args()[4:], stream=stream)
        assert device.mesh_counts() == (1800, 1800, 0)
        assert tgd._same_arrays(tgd._readback(device, nq), want[0])
        assert np.array_equal(_records(device, nq).view(np.uint8), want[1].view(np.uint8))
        assert_render_equal(device.render_pixels(cam, NX, NY, SPP, DEPTH, pix)[:3], want[2], "[N, 3] tensors")
    # and [N, 3] host arrays through set_scene_mesh
    args = list(only.set_args())
    args[1] = only.quads[:, :3]
    device.set_scene_mesh(*args)
    assert device.mesh_counts() == (1800, 1800, 0)
    assert_render_equal(device.render_pixels(cam, NX, NY, SPP, DEPTH, pix)[:3], want[2], "[N, 3] host arrays")
    # a context without a mesh scene has no counts
    device.set_cornell_box(0)
    with pytest.raises(rtp.RtpError):
        device.mesh_counts()


# 10 --------------------------------------------------- the other pool instances --
def test_stealing_frame(device, oracle, rtp, monkeypatch):
    m = T.hills_tri()
    tgm._set(device, m)
    nx, ny, spp, depth = 1024, 768, 1, 4  # 786 432 entries: more than the 655 360 resident slots
    cam = rtp.default_camera()
    monkeypatch.delenv("RTP_STEAL", raising=False)
    stolen, _ = device.render(cam, nx, ny, spp, depth)
    monkeypatch.setenv("RTP_STEAL", "0")
    plain, _ = device.render(cam, nx, ny, spp, depth)
    monkeypatch.delenv("RTP_STEAL")
    assert_render_equal((stolen, None, None), (plain, None, None), "stealing against RTP_STEAL=0")
    pix = np.sort(np.random.default_rng(3).choice(nx * ny, 4096, replace=False)).astype(np.int64)
    want = oracle.render_pixels(m.scene(oracle), oracle.camera_setup(nx, ny), nx, ny, spp, depth, pix)
    assert_render_equal((stolen[pix], None, None), (want[0], None, None), "the stolen frame against the oracle")


def test_resume_and_refine(device, rtp):
    m = T.mixed()
    tgm._set(device, m)
    cam = m.camera(rtp)
    nx, ny, depth = 48, 40, 8
    r = rtp.ProgressiveRender(device, cam, nx, ny, depth)
    r.step(2)
    r.step(2)
    s = r.state()
    pix = np.arange(nx * ny, dtype=np.int64)
    assert_render_equal((s["sums"], s["seed"], s["live"]), device.render_pixels(cam, nx, ny, 4, depth, pix)[:3],
                        "two passes of 2 against one of 4")
    threshold = float(np.median(noise_ref(s["sums"], s["m2"], s["count"])))
    ids = np.flatnonzero(active_ref(s["sums"], s["m2"], s["count"], 2, threshold, 16)).astype(np.int64)
    assert 0.05 < ids.size / (nx * ny) < 0.95
    assert r.refine_device(2, threshold, 16) == ids.size
    t = r.state()
    assert np.array_equal(t["count"][ids], s["count"][ids] + 2)
    rest = np.setdiff1d(pix, ids)
    assert np.array_equal(t["sums"][rest].view(U), s["sums"][rest].view(U)) and np.array_equal(t["seed"][rest], s["seed"][rest])
    assert_render_equal((t["sums"][ids], t["seed"][ids], t["live"][ids]),
                        device.render_pixels(cam, nx, ny, 6, depth, ids)[:3], "the refined pixels against 6 spp")


# 11 ------------------------------------------------------ beyond the oracle --
def test_walk_equals_scan_render_on_65536_triangles(device, rtp, monkeypatch):
    m = T.hills(32768, True)
    assert len(m.quads) == 65536 + T.N_ROOM
    cam = m.camera(rtp)
    pix = np.arange(32 * 32, dtype=np.int64)
    monkeypatch.delenv("RTP_MESH_SCAN", raising=False)
    tgm._set(device, m)
    assert device.mesh_counts() == (65536 + T.N_ROOM, 65536, 0)
    walk = device.render_pixels(cam, 32, 32, 2, 6, pix)[:3]
    monkeypatch.setenv("RTP_MESH_SCAN", "1")
    tgm._set(device, m)
    scan = device.render_pixels(cam, 32, 32, 2, 6, pix)[:3]
    assert_render_equal(walk, scan, "walk against RTP_MESH_SCAN=1 on 65 536 triangle cells")
    assert walk[2].sum() > 32 * 32 * 2  # (paths go on past the first hit)


# 12 ------------------------------------------------------------------ mapper --
def test_mapper_takes_triangle_cells(device, rtp):
    m = T.hills_tri()
    tgm._set(device, m)
    cam = rtp.default_camera()
    want, _ = device.render(cam, NX, NY, SPP, DEPTH)
    device.set_cornell_box(0)
    sp = m.spheres
    assert (m.quads[T.N_ROOM:, 2] == m.quads[T.N_ROOM:, 3]).all()  # rows (a, b, c, c) pass through RenderCells
    cells = rtp.CellSet(m.quads, np.array([s[0] for s in sp], dtype=np.int32),
                        sphere_radius=np.array([s[1] for s in sp], dtype=F))
    mapper = rtp.MapperPathTracer(SPP, DEPTH, (m.quad_mat, np.array([s[2] for s in sp], dtype=np.int32)),
                                  (m.quad_tex, np.array([s[3] for s in sp], dtype=np.int32)),
                                  np.array(m.mat_type, dtype=np.int32), np.array(m.tex_type, dtype=np.int32), m.tex,
                                  device=device)
    canvas = rtp.CanvasRayTracer(NX, NY)
    mapper.SetCanvas(canvas)
    mapper.RenderCells(cells, m.points, None, None, cam, None, m.light, m.light_sphere_point, m.ior)
    assert device.mesh_counts() == (1805, 1800, 0)  # (the mapper set a mesh scene, its triangles bounded)
    assert_render_equal((canvas.GetColorBuffer(), None, None), (want, None, None), "RenderCells against set_scene_mesh")
