"""Triangle cells of a mesh scene without a GPU (include/rtp_mesh.h: a cell
whose v11 and v01 compare equal, in particular (a, b, c, c)): the host
builder's pads and boxes against the formula restated in float64, the pad's
soundness by tests/test_mesh_host.py's float64 check on the scenes of
tests/_trimeshes.py, the host scan against the oracle's quad test, the trees,
and the Python and C interfaces (the [N, 3] connectivity, rtp.triangulate,
rtp.unbounded_cells, rtp_mesh_counts)."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import _meshes
import _trimeshes as T
import test_mesh_host as tmh

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hills_tri", "mixed", "slivers")


def _spheres(m):
    return [s[0] for s in m.spheres], [s[1] for s in m.spheres]


# 1 -------------------------------------------------------- counts and pads --
def test_no_triangle_of_the_hills_is_unbounded():
    m, b = T.hills_tri(), tmh.built("hills_tri")
    tri = T.is_triangle(m)
    assert int(tri.sum()) == 1800 and len(m.quads) == 1805
    assert int((b["pads"][tri] == T.HUGE).sum()) == 0
    assert int((b["pads"] == T.HUGE).sum()) == 0


@pytest.mark.parametrize("name", NEW)
def test_triangle_pads_and_boxes_equal_the_formula(name):
    m, b = tmh.scene(name), tmh.built(name)
    tri = T.is_triangle(m)
    assert tri.sum() > 32
    pad, mn, mx = T.tri_pad_formula(m, b["reach"], b["cos_min"])
    got = b["pads"][tri].astype(np.float64)
    fin = np.isfinite(pad[tri])
    assert (got[~fin] == float(T.HUGE)).all() and (got[fin] < 2.0 ** 99).all()
    # the builder's double arithmetic, rounded to float32 and stepped one ulp up
    want = np.nextafter(pad[tri][fin].astype(F), F(np.inf)).astype(np.float64)
    assert np.abs(got[fin] - want).max() <= np.spacing(want.astype(F)).max(), "the pad is the formula's"
    assert (np.abs(got[fin] / pad[tri][fin] - 1) < 4 * 2.0 ** -24).all()
    # the box: the three vertices -+ pad, one ulp outward
    p32 = b["pads"][tri][fin]
    lo = np.nextafter((mn[tri][fin].astype(F) - p32[:, None]).astype(F), F(-np.inf))
    hi = np.nextafter((mx[tri][fin].astype(F) + p32[:, None]).astype(F), F(np.inf))
    box = b["boxes"][tri][fin]
    assert np.array_equal(box[:, :3].view(np.uint32), lo.view(np.uint32))
    assert np.array_equal(box[:, 3:].view(np.uint32), hi.view(np.uint32))
    unb = b["boxes"][tri][~fin]
    assert (unb[:, :3] <= -2.0 ** 99).all() and (unb[:, 3:] >= 2.0 ** 99).all()
    # the quads of the scene keep the quad's pad (tests/test_mesh_host.py pad_formula)
    qpad, _ = tmh.pad_formula(m, b["reach"], b["cos_min"])
    q = ~tri
    assert np.array_equal(np.isfinite(qpad[q]), b["pads"][q] < 2.0 ** 99)
    f = np.isfinite(qpad[q])
    assert (np.abs(b["pads"][q][f] / qpad[q][f] - 1) < 4 * 2.0 ** -24).all()


def test_slivers_cover_both_sides_of_the_sine_limit():
    m, b = T.slivers(), tmh.built("slivers")
    s = T.sliver_sines()
    pads = b["pads"][T.N_ROOM:T.N_ROOM + T.N_SLIVERS]
    assert (s >= T.MIN_SINE).sum() > 8 and (s < T.MIN_SINE).sum() > 4
    assert (pads[s < T.MIN_SINE] == T.HUGE).all(), "a corner flatter than kMeshMinSine: the unbounded box"
    wide = s > 2 * T.MIN_SINE
    assert (pads[wide] < 2.0 ** 99).all()
    # the 1 / s term: the pad less the slab grows as the sine falls
    slab = 1e-5 + 2.0 ** -16 + 2.0 ** -18 * b["reach"]
    ratio = (pads[wide].astype(np.float64) - slab) * s[wide]
    assert ratio.max() / ratio.min() < 1.02 and pads[wide][-1] > 100 * pads[wide][0]
    # equal by value, not by id (the last with +0 against -0): triangle cells like the others
    tail = slice(T.N_ROOM + T.N_SLIVERS, None)
    assert (m.quads[tail, 2] != m.quads[tail, 3]).all() and T.is_triangle(m)[tail].all()
    pad, _, _ = T.tri_pad_formula(m, b["reach"], b["cos_min"])
    assert (b["pads"][tail] < 2.0 ** 99).all() and (np.abs(b["pads"][tail] / pad[tail] - 1) < 4 * 2.0 ** -24).all()


def test_bent_quads_are_unbounded_and_bounded_once_split():
    import raytracingtherestofyourlife_amd as rtp

    q = T.hills_quads()
    b = tmh.built("hills_quads")
    terrain = slice(T.N_ROOM, None)
    assert (b["pads"][terrain] == T.HUGE).mean() > 0.5, "a curved terrain of quads is mostly unbounded"
    which = rtp.unbounded_cells(q.points, q.quads, *_spheres(q))
    assert np.array_equal(which, b["pads"] == T.HUGE)
    cells, mat, tex, parent = rtp.triangulate(q.quads, q.quad_mat, q.quad_tex, which)
    assert len(cells) == len(q.quads) + int(which.sum())
    assert not rtp.unbounded_cells(q.points, cells, *_spheres(q)).any(), "the whole terrain is bounded again"
    assert np.array_equal(mat, q.quad_mat[parent]) and np.array_equal(tex, q.quad_tex[parent])


# 2, 3 ---------------------------------------- the pad is sound; the oracle --
@pytest.mark.parametrize("name", NEW)
def test_pad_holds_every_accepted_hit_inside_the_promise(name, oracle):
    """tests/test_mesh_host.py's check, on the new scenes: every winner's t is the oracle's rtpo_stage_quad_hit
    bit for bit; at most 1% of a part outside the promise; the accepted point inside the padded box."""
    tmh.test_pad_holds_every_accepted_hit_inside_the_promise(name, oracle)


@pytest.mark.parametrize("name", NEW)
def test_no_triangle_accepts_a_hit_beyond_its_third_edge(name):
    m = tmh.scene(name)
    ray, tbits, win, inside = tmh.scanned(name)
    tri = T.is_triangle(m)
    use = np.flatnonzero((win >= 0) & tri[np.maximum(win, 0)])  # every triangle winner, inside the promise or not
    assert use.size > 4096
    V = m.verts().astype(np.float64)[win[use]]
    r = ray[use].astype(np.float64)
    p = r[:, :3] + tbits[use].view(F).astype(np.float64)[:, None] * r[:, 3:]
    e01, e03, w = V[:, 1] - V[:, 0], V[:, 3] - V[:, 0], p - V[:, 0]
    # barycentric coordinates of the accepted point on the triangle's plane (least squares)
    a11, a12, a22 = (e01 * e01).sum(1), (e01 * e03).sum(1), (e03 * e03).sum(1)
    b1, b2 = (w * e01).sum(1), (w * e03).sum(1)
    det = a11 * a22 - a12 * a12
    alpha, beta = (b1 * a22 - b2 * a12) / det, (b2 * a11 - b1 * a12) / det
    print(f"{name}: {use.size} triangle winners, max alpha + beta {float((alpha + beta).max()):.7f}")
    assert ((alpha + beta) <= 1 + 1e-4).all()


# 4 ------------------------------------------------------------------ trees --
@pytest.mark.parametrize("name", NEW + ("hills_quads",))
def test_builder_tree(name):
    tmh.test_builder_tree(name)  # every cell once, children inside parents, leaf boxes around their cells; 8 octants


def test_quad_scenes_keep_their_pads():
    """A quad cell is not touched: on a scene without triangle cells every pad is the quad formula's."""
    m, b = tmh.scene("hills_quads"), tmh.built("hills_quads")
    assert not T.is_triangle(m).any()
    qpad, _ = tmh.pad_formula(m, b["reach"], b["cos_min"])
    assert np.array_equal(np.isfinite(qpad), b["pads"] < 2.0 ** 99)


# 5 -------------------------------------------------------------------- API --
def test_three_ids_a_row_equal_the_repeated_id():
    from raytracingtherestofyourlife_amd.device import mesh_scene_desc, scene_desc

    m = T.hills_tri()
    tri = T.is_triangle(m)
    only = _meshes.Mesh(m.points, m.quads[tri], m.quad_mat[tri], m.quad_tex[tri], m.spheres, m.mat_type, m.tex_type,
                        m.tex, m.light, m.light_sphere_point, m.ior)
    args = list(only.set_args())
    four, keep4 = scene_desc(*args)
    args[1] = only.quads[:, :3]
    assert args[1].shape == (1800, 3)
    three, keep3 = mesh_scene_desc(*args)
    assert three.n_quads == four.n_quads == 1800
    assert all(np.array_equal(keep3[k], keep4[k]) and keep3[k].dtype == keep4[k].dtype for k in keep4)
    for name, _ in type(four)._fields_:
        if name not in keep4:  # (the pointers: the arrays above, byte for byte; the rest: the descriptor's own bytes)
            f = getattr(type(four), name)
            assert ctypes.string_at(ctypes.addressof(three) + f.offset, f.size) == \
                ctypes.string_at(ctypes.addressof(four) + f.offset, f.size), name
    # and the builder's outputs, through the descriptors themselves
    from raytracingtherestofyourlife_amd._lib import ptr

    L = tmh._lib()
    outs = []
    for desc in (three, four):
        nodes = np.zeros(2 * 1800, dtype=_meshes.NODE)
        order, boxes, pads = np.zeros(1800, np.int32), np.zeros((1800, 6), F), np.zeros(1800, F)
        nn = ctypes.c_int32(0)
        assert L.rtp_mesh_build_host(desc, 3, len(nodes), nn, nodes.ctypes.data, ptr(order), ptr(boxes), ptr(pads),
                                     None) == 0
        outs.append((nodes[: nn.value].tobytes(), order.tobytes(), boxes.tobytes(), pads.tobytes()))
    assert outs[0] == outs[1]


def test_triangulate_on_numpy_and_torch():
    import torch

    import raytracingtherestofyourlife_amd as rtp

    q, t = T.hills_quads(), T.hills_tri()
    terrain = np.arange(len(q.quads)) >= T.N_ROOM
    cells, mat, tex, parent = rtp.triangulate(q.quads, q.quad_mat, q.quad_tex, terrain)
    assert isinstance(cells, np.ndarray) and cells.dtype == np.int32
    assert np.array_equal(cells, t.quads) and np.array_equal(mat, t.quad_mat) and np.array_equal(tex, t.quad_tex)
    assert np.array_equal(parent, np.r_[np.arange(T.N_ROOM), np.repeat(np.arange(T.N_ROOM, len(q.quads)), 2)])
    # a list of indices selects like the mask; None splits every quad
    by_index = rtp.triangulate(q.quads, q.quad_mat, q.quad_tex, np.flatnonzero(terrain))
    assert all(np.array_equal(a, b) for a, b in zip(by_index, (cells, mat, tex, parent)))
    every = rtp.triangulate(q.quads, q.quad_mat, q.quad_tex)
    assert len(every[0]) == 2 * len(q.quads) and np.array_equal(every[0][2 * T.N_ROOM:], t.quads[T.N_ROOM:])
    # both halves: the quad's orientation (the normal of (v00, v10, v11) on the same side), together its area
    V = q.verts().astype(np.float64)[T.N_ROOM:]
    H = t.points[t.quads[T.N_ROOM:]].astype(np.float64).reshape(-1, 2, 4, 3)
    nq = np.cross(V[:, 1] - V[:, 0], V[:, 3] - V[:, 0])
    for half in (0, 1):
        nh = np.cross(H[:, half, 1] - H[:, half, 0], H[:, half, 2] - H[:, half, 0])
        assert ((nh * nq).sum(1) > 0).all()
    # torch tensors stay tensors
    tq, tm, tt = (torch.from_numpy(np.ascontiguousarray(a)) for a in (q.quads, q.quad_mat, q.quad_tex))
    for which in (torch.from_numpy(terrain), terrain, torch.from_numpy(np.flatnonzero(terrain))):
        got = rtp.triangulate(tq, tm, tt, which)
        assert all(isinstance(g, torch.Tensor) for g in got) and got[0].dtype == torch.int32
        assert all(np.array_equal(g.numpy(), w) for g, w in zip(got, (cells, mat, tex, parent)))
    with pytest.raises(ValueError):
        rtp.triangulate(q.quads, q.quad_mat, q.quad_tex, terrain[:-1])
    # a row that is a triangle cell already stays whole: no (c, c, b, b) cell without area, nothing new unbounded
    x = T.mixed()
    cells, mat, tex, parent = rtp.triangulate(x.quads, x.quad_mat, x.quad_tex)
    was_tri = x.quads[:, 2] == x.quads[:, 3]
    assert len(cells) == int(was_tri.sum()) + 2 * int((~was_tri).sum())
    assert (cells[:, 2] == cells[:, 3]).all() and (cells[:, 0] != cells[:, 1]).all()
    assert np.array_equal(cells[np.isin(parent, np.flatnonzero(was_tri))], x.quads[was_tri])
    sp = [s[0] for s in x.spheres], [s[1] for s in x.spheres]
    assert not rtp.unbounded_cells(x.points, cells, *sp).any()
    got = rtp.triangulate(torch.from_numpy(x.quads), torch.from_numpy(x.quad_mat), torch.from_numpy(x.quad_tex))
    assert np.array_equal(got[0].numpy(), cells) and np.array_equal(got[3].numpy(), parent)


def test_mesh_counts_is_in_the_header_the_table_and_the_library():
    from raytracingtherestofyourlife_amd import Device
    from raytracingtherestofyourlife_amd import _lib as lib

    mesh = lib.SIGNATURES["include/rtp_mesh.h"]
    assert mesh["rtp_mesh_counts"] == (ctypes.c_int32, [lib.vp, lib.i32p, lib.i32p, lib.i32p])
    assert "rtp_mesh_counts" not in lib.SIGNATURES["include/rtp.h"] and "rtp_mesh_counts" not in lib.EXPORTED_SYMBOLS
    assert "rtp_mesh_counts" not in open(os.path.join(ROOT, "include", "rtp.h")).read()
    hdr = open(os.path.join(ROOT, "include", "rtp_mesh.h")).read()
    assert ("rtp_status rtp_mesh_counts(rtp_context* ctx, int32_t* n_cells, int32_t* n_triangles, "
            "int32_t* n_unbounded);") in hdr
    assert "(a, b, c, c)" in hdr
    L = lib.load()
    assert hasattr(L, "rtp_mesh_counts") and L.rtp_abi_version() == 3
    assert callable(Device.mesh_counts)
    # no context, no mesh scene: refused like rtp_mesh_guarantee
    n = ctypes.c_int32(7)
    assert L.rtp_mesh_counts(None, n, None, None) == lib.RTP_ERR_INVALID_ARGUMENT and n.value == 7


# 6 -------------------------------------------------------------- sanitizer --
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a HIP device is present: sanitized programs do not run there")
def test_triangle_builder_sanitized_without_device():
    import subprocess

    from raytracingtherestofyourlife_amd import build
    from test_asan_mesh import ENV

    exe = {os.path.basename(e): e for e in build.build_asan()}["asan_mesh_tri"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.strip() == "OK"
    assert r.stderr.strip() == "", r.stderr[-4000:]
