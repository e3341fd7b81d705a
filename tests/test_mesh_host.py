"""Mesh scenes (rtp_set_scene_mesh) without a GPU: the new symbols, the
instance table's walk 3, the device-free BVH builder (rtp_mesh_build_host) on
the generated scenes of tests/_meshes.py, the boxes' pad checked in float64
against what the float32 quad test accepts, and the descriptor refusals.

The pad check takes every ray of the populations, the host brute-force scan's
winning quad (rtp_mesh_scan_host: the reference's float32 test; the oracle's
rtpo_stage_quad_hit confirms every accepted t bit for bit), and, for every
winner inside the promise (reach, cos_min), requires the point at the accepted
t to lie inside the quad's padded box with the slab test's rounding to spare
on every axis: 2^-22 (|o| + |box|), the error in space of one v_rcp_f32 ulp
and one rounding of o / d (rtp_trace.hpp mesh_visit).  Every box on the path
from the root to the quad's leaf contains that box (checked on the builder's
output below: child inside parent, leaf boxes around their quads), so the
interval the ray spends in each of them contains the accepted t likewise.
Condition, not measurement: outside the grazing part at most 1% of a part's
rays may be outside the promise and skipped."""
from __future__ import annotations

import ctypes
import functools
import itertools
import os

import numpy as np
import pytest

import _meshes

F = np.float32
MAX_OUTSIDE = 0.01


def _lib():
    import raytracingtherestofyourlife_amd as rtp

    return rtp.load()


build = _meshes.build_host


@functools.lru_cache(maxsize=None)
def built(name, oct=0):
    return build(scene(name), oct)


def scene(name):
    if name == "cornell0":
        return _meshes.cornell(0)
    if name == "cornell2":
        return _meshes.cornell(2)
    if name == "grid65536":
        return _meshes.grid(65536)
    return _meshes.SCENES[name]()


ALL = ("cornell0", "cornell2", "tess", "facets", "bent", "grid65536")


# ------------------------------------------------------------------- ABI --
def test_new_symbols_are_in_the_signature_table():
    from raytracingtherestofyourlife_amd import _lib as lib

    i32, vp = ctypes.c_int32, ctypes.c_void_p
    mesh = lib.SIGNATURES["include/rtp_mesh.h"]
    assert mesh["rtp_set_scene_mesh"] == (i32, [vp, ctypes.POINTER(lib.RtpSceneDesc)])
    assert mesh["rtp_mesh_guarantee"] == (i32, [vp, lib.f32p, lib.f32p])
    assert not set(mesh) & set(lib.SIGNATURES["include/rtp.h"]) and not set(mesh) & set(lib.EXPORTED_SYMBOLS)
    rtp_h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtp.h")).read()
    assert not any(name in rtp_h for name in mesh)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtp_mesh.h")).read()
    assert "rtp_status rtp_set_scene_mesh(rtp_context* ctx, const rtp_scene_desc* scene);" in hdr
    assert "rtp_status rtp_mesh_guarantee(rtp_context* ctx, float* cos_min, float* reach);" in hdr
    L = lib.load()
    for name in ("rtp_set_scene_mesh", "rtp_mesh_guarantee", "rtp_mesh_build_host", "rtp_mesh_scan_host"):
        assert hasattr(L, name), name
    assert L.rtp_abi_version() == 3
    from raytracingtherestofyourlife_amd import Device

    assert callable(Device.set_scene_mesh) and callable(Device.mesh_guarantee)


def test_walk_3_names_exactly_the_four_mesh_instances():
    L = _lib()
    pool = "rtp_render_pool<false, false, false, false, %s, false, %s, true>"
    want = {(0, 0): pool % ("false", "false"), (1, 0): pool % ("true", "false"), (0, 1): pool % ("false", "true"),
            (1, 1): pool % ("true", "true")}
    found = 0
    for stats, tiles, plan, steal, views, resume in itertools.product((0, 1), repeat=6):
        got = L.rtp_instance_name(2, stats, 3, tiles, plan, steal, views, resume)
        if stats or tiles or plan or views:
            assert got is None, (stats, tiles, plan, steal, views, resume, got)
        else:
            assert got is not None and got.decode() == want[(steal, resume)]
            found += 1
    assert found == 4
    for mode in itertools.product((0, 1), repeat=6):
        assert L.rtp_instance_name(1, mode[0], 3, *mode[1:]) is None  # (no lockstep kernel on a mesh scene)
    assert 1 <= L.rtp_mesh_leaf_size() <= 7


# --------------------------------------------------------------- builder --
@pytest.mark.parametrize("name", ALL)
def test_builder_tree(name):
    m = scene(name)
    nq = len(m.quads)
    leaf_max = _lib().rtp_mesh_leaf_size()
    seen_order = None
    for oct in range(8):
        b = build(m, oct) if oct else built(name)
        nodes, order, boxes = b["nodes"], b["order"], b["boxes"]
        nn = len(nodes)
        assert sorted(order.tolist()) == list(range(nq)), "every quad once in the leaf order"
        if seen_order is not None:
            assert (order == seen_order).all(), "one leaf order for all octants"
        seen_order = order
        skip = nodes["skip"].astype(np.int64)
        leaf = nodes["leaf"] != 0
        first, count = nodes["leaf"] >> 3, nodes["leaf"] & 7
        assert (count[leaf] >= 1).all() and (count[leaf] <= leaf_max).all()
        # every quad in exactly one leaf
        cover = np.zeros(nq + 1, dtype=np.int64)
        np.add.at(cover, first[leaf], 1)
        np.add.at(cover, first[leaf] + count[leaf], -1)
        assert (np.cumsum(cover)[:nq] == 1).all()
        # the threaded order: a leaf goes on at i + 1, an inner node's skip is beyond it, none beyond nn
        idx = np.arange(nn)
        assert (skip > idx).all() and (skip <= nn).all() and (skip[leaf] == idx[leaf] + 1).all()
        # each node's parent: the nearest earlier inner node whose skip lies beyond it
        parent = np.full(nn, -1, dtype=np.int64)
        sk, lf, stack = skip.tolist(), leaf.tolist(), []
        for j in range(nn):
            while stack and sk[stack[-1]] <= j:
                stack.pop()
            if stack:
                parent[j] = stack[-1]
            if not lf[j]:
                stack.append(j)
        has = parent >= 0
        par = parent[has]
        assert int((~has).sum()) == 1 and not has[0], "one root: node 0"
        # subtrees nest: a child's skip ends inside its parent's, the last child's exactly at it, and an inner
        # node has at least two nodes below it
        assert (skip[has] <= skip[par]).all()
        last_child = np.zeros(nn, dtype=np.int64)
        np.maximum.at(last_child, par, skip[has])
        inner = ~leaf
        assert (last_child[inner] == skip[inner]).all()
        assert (np.bincount(par, minlength=nn)[inner] == 2).all(), "binary: two children per inner node"
        # the two walks the threading allows at the extremes: every box hit (i + 1 throughout) visits every
        # leaf once and ends at nn; every box missed leaves by the root's skip
        assert int(leaf.sum()) == len(np.unique(first[leaf])) and skip[nn - 1] == nn and leaf[nn - 1]
        assert skip[0] == nn
        # a random hit / miss pattern: the walk rises strictly and ends exactly at nn
        rng = np.random.default_rng(oct)
        hit = rng.random(nn) < 0.7
        i, steps = 0, 0
        while i < nn:
            i = i + 1 if (hit[i] or lf[i]) else sk[i]
            steps += 1
        assert i == nn and steps <= nn
        # child boxes inside their parent's
        assert (nodes["lo"][has] >= nodes["lo"][par]).all() and (nodes["hi"][has] <= nodes["hi"][par]).all()
        # a leaf's box holds its quads' boxes
        owner = np.repeat(np.flatnonzero(leaf), count[leaf])
        pos = np.concatenate([np.arange(f, f + c) for f, c in zip(first[leaf].tolist(), count[leaf].tolist())])
        q = order[pos]
        assert (boxes[q, :3] >= nodes["lo"][owner]).all() and (boxes[q, 3:] <= nodes["hi"][owner]).all()


def test_compact_nodes_round_outward():
    """mesh_compact (the walk's 16-byte nodes): every half-precision box holds its BvhNode's box, an
    unbounded box becomes +-inf, NaN becomes the infinity on its side, and skip / leaf words carry over."""
    from raytracingtherestofyourlife_amd._lib import ptr

    L = _lib()
    nodes = np.concatenate([built("bent")["nodes"], built("grid65536")["nodes"][:4096]]).copy()
    extra = np.zeros(6, dtype=_meshes.NODE)
    vals = [0.0, -0.0, 65504.0, 65505.0, 1e-8, -1e-8, 2.0 ** -24, 1 + 2.0 ** -11, np.nan, 2.0 ** 100, -2.0 ** 100,
            0.1, -0.1, 3.4e38, -3.4e38, 1e-30, 6.1e-5, -6.1e-5]
    for k in range(6):
        extra["lo"][k] = vals[3 * k:3 * k + 3]
        extra["hi"][k] = vals[3 * k:3 * k + 3]
        extra["skip"][k] = 7 + k
    nodes = np.concatenate([nodes, extra])
    out = np.zeros((len(nodes), 4), dtype=np.uint32)
    L.rtp_mesh_compact_host(nodes.ctypes.data, len(nodes), ptr(out))
    h = np.ascontiguousarray(out[:, :3]).view(np.uint16).reshape(-1, 6).view(np.float16).astype(np.float64)
    lo, hi = h[:, :3], h[:, 3:]  # (lo.x, lo.y, lo.z, hi.x, hi.y, hi.z: rtp_layout.hpp kCBvhLeafBit)
    nlo, nhi = nodes["lo"].astype(np.float64), nodes["hi"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        assert ((lo <= nlo) | np.isnan(nlo)).all() and ((hi >= nhi) | np.isnan(nhi)).all()
    assert (lo[np.isnan(nlo)] == -np.inf).all() and (hi[np.isnan(nhi)] == np.inf).all()
    assert (lo[nlo <= -2.0 ** 99] == -np.inf).all() and (hi[nhi >= 2.0 ** 99] == np.inf).all()
    # tight: the next half inward is on the wrong side (finite halves)
    f16 = lambda a: a.astype(np.float16)
    with np.errstate(over="ignore"):  # (a step from the largest half is inf: still on the wrong side)
        fin = np.isfinite(lo) & np.isfinite(nlo)
        assert (np.nextafter(f16(lo[fin]), np.float16(np.inf)).astype(np.float64) > nlo[fin]).all()
        fin = np.isfinite(hi) & np.isfinite(nhi)
        assert (np.nextafter(f16(hi[fin]), np.float16(-np.inf)).astype(np.float64) < nhi[fin]).all()
    leaf = nodes["leaf"] != 0
    assert (out[~leaf, 3] == nodes["skip"][~leaf].astype(np.uint32)).all()
    assert (out[leaf, 3] == (nodes["leaf"][leaf].astype(np.uint32) | 0x40000000)).all()


def test_mildly_bent_quads_keep_bounded_boxes_with_an_h_term():
    """bent()'s last N_MILD quads are lifted by 0.02% to 0.10% of the edge: under the fold limit, so their
    boxes are bounded and the pad's h / cos_min term is several times the planar pad; the pad test and the
    GPU walk-against-scan test cull them like any other quad."""
    m, b = scene("bent"), built("bent")
    mild = slice(len(m.quads) - _meshes.N_MILD, len(m.quads))
    pads = b["pads"]
    assert (pads[mild] < 2.0 ** 99).all()
    V = m.verts().astype(np.float64)[mild]
    n1 = np.cross(V[:, 1] - V[:, 0], V[:, 3] - V[:, 0])
    h = np.abs(((V[:, 2] - V[:, 0]) * n1).sum(1)) / np.linalg.norm(n1, axis=1)
    assert (h > 1e-5).all()
    planar = float(np.median(built("facets")["pads"]))
    assert (pads[mild] >= planar * 0.99 + h / b["cos_min"]).all() and (h / b["cos_min"] > planar).all()
    strong = slice(mild.start - 64, mild.start)
    assert (pads[strong] >= 2.0 ** 99).all()


def pad_formula(m, reach, cos_min):
    """The pad of rtp_layout.hpp in float64, per quad (inf: the unbounded box)."""
    V = m.verts().astype(np.float64)
    e01, e03, e21, e23 = V[:, 1] - V[:, 0], V[:, 3] - V[:, 0], V[:, 1] - V[:, 2], V[:, 3] - V[:, 2]
    n1 = np.cross(e01, e03)
    A1, A2 = np.linalg.norm(n1, axis=1), np.linalg.norm(np.cross(e21, e23), axis=1)
    ln = lambda e: np.linalg.norm(e, axis=1)
    with np.errstate(all="ignore"):
        sine = np.minimum(A1 / (ln(e01) * ln(e03)), A2 / (ln(e21) * ln(e23)))
        h = np.abs(((V[:, 2] - V[:, 0]) * n1).sum(1)) / A1
        u1 = np.cross(n1, V[:, 3] - V[:, 1])
        side = np.where(((V[:, 0] - V[:, 1]) * u1).sum(1) < 0, 1.0, -1.0)
        w = side * ((V[:, 2] - V[:, 1]) * u1).sum(1) / ln(u1)
        far = V[:, 0].astype(F) + (V[:, 1].astype(F) - V[:, 0].astype(F)) + (V[:, 3].astype(F) - V[:, 0].astype(F))
        amax = np.maximum(np.abs(V).max((1, 2)), np.abs(far).max(1))
        pad = ((2.0 ** -18) * reach / sine + h) / cos_min + 1e-5 + 2.0 ** -16 * amax + 2.0 ** -18 * reach
        huge = ~(sine >= 2.0 ** -10) | ((h > 0) & (~(w > 0) | ~(h / w < 0.5 * cos_min))) | ~(pad < reach)
    return np.where(huge, np.inf, pad), far


@pytest.mark.parametrize("name", ALL)
def test_builder_boxes_hold_the_quads_and_the_pad(name):
    m, b = scene(name), built(name)
    lo, hi = m.bounds()
    assert b["cos_min"] == 2.0 ** -8
    assert b["reach"] == pytest.approx(2 * np.linalg.norm(hi - lo), rel=1e-5)
    pad, far = pad_formula(m, b["reach"], b["cos_min"])
    V = m.verts().astype(np.float64)
    mn = np.minimum(V.min(1), far)
    mx = np.maximum(V.max(1), far)
    need = np.where(np.isinf(pad), 2.0 ** 99, pad * (1 - 1e-6))[:, None]
    assert (b["boxes"][:, :3] <= mn - need).all() and (b["boxes"][:, 3:] >= mx + need).all()
    finite = np.isfinite(pad)
    assert (b["pads"][finite] < 2.0 ** 99).all() and (b["pads"][~finite] >= 2.0 ** 99).all()
    if name.startswith("cornell"):  # well under 1% of the scene's diagonal
        assert b["pads"][finite].max() < 0.005 * np.linalg.norm(hi - lo)
    if name in ("tess", "facets", "grid65536"):
        assert finite.mean() > 0.95, "planar facets get bounded boxes"


# ------------------------------------------------------------------- pad --
@functools.lru_cache(maxsize=None)
def scanned(name):
    """The rays of a scene, the host scan's (t bits, winner) and the promise mask."""
    m, b = scene(name), built(name)
    finite = b["pads"][b["pads"] < 2.0 ** 99]
    ray = _meshes.rays(name, b["cos_min"], float(np.median(finite)))
    tbits, win = _meshes.host_scan(m, ray)
    return ray, tbits, win, _meshes.inside_promise(m, ray, win, b["cos_min"], b["reach"])


@pytest.mark.parametrize("name", ("tess", "facets", "bent"))
def test_pad_holds_every_accepted_hit_inside_the_promise(name, oracle):
    m, b = scene(name), built(name)
    ray, tbits, win, inside = scanned(name)
    assert len(ray) == _meshes.N_RAYS
    hit = win >= 0
    # the oracle's own test accepts each winner with the same t, bit for bit
    V = m.verts()
    rows = np.flatnonzero(hit)
    cases = np.zeros((len(rows), 20), dtype=np.uint32)
    cases[:, :6] = ray[rows].view(np.uint32)
    cases[:, 6:18] = V[win[rows]].reshape(-1, 12).view(np.uint32)
    cases[:, 18] = F(0.001).view(np.uint32)
    cases[:, 19] = F(3.40282347e+38).view(np.uint32)
    got = oracle.stage("quad_hit", None, cases)
    assert (got[:, 0] == 1).all() and (got[:, 3] == tbits[rows]).all()
    # at most 1% of a part outside the promise (the grazing part is built at its edge)
    for part in range(_meshes.N_PARTS):
        s = slice(part * _meshes.PART, (part + 1) * _meshes.PART)
        out = float((~inside[s]).mean())
        print(f"{name} {_meshes.PART_NAMES[part]}: {int(hit[s].sum())} quad hits, {out:.4f} outside the promise")
        if part != _meshes.GRAZING:
            assert out <= MAX_OUTSIDE, (name, _meshes.PART_NAMES[part], out)
    assert (hit & inside)[_meshes.GRAZING * _meshes.PART:(_meshes.GRAZING + 1) * _meshes.PART].sum() > 1000
    if name == "bent":  # the mildly bent quads win rays inside the promise, grazing ones among them
        mild = win >= len(m.quads) - _meshes.N_MILD
        graz = np.zeros(len(ray), bool)
        graz[_meshes.GRAZING * _meshes.PART:(_meshes.GRAZING + 1) * _meshes.PART] = True
        print(f"bent: {int((mild & inside).sum())} winners on mildly bent quads inside the promise, "
              f"{int((mild & inside & graz).sum())} of them grazing")
        assert (mild & inside).sum() > 2000 and (mild & inside & graz).sum() > 500
    # the accepted point, in float64, inside the winner's box with the slab test's rounding to spare
    use = np.flatnonzero(hit & inside)
    r = ray[use].astype(np.float64)
    t = tbits[use].view(F).astype(np.float64)
    p = r[:, :3] + t[:, None] * r[:, 3:]
    box = b["boxes"][win[use]].astype(np.float64)
    spare = 2.0 ** -22 * (np.abs(r[:, :3]).max(1) + np.abs(box).max(1))[:, None]
    spare = np.where(np.isfinite(spare), spare, 0.0)
    ok = ((p >= box[:, :3] + spare) & (p <= box[:, 3:] - spare)).all(1)
    bad = use[~ok]
    assert bad.size == 0, (name, bad[:8].tolist(), ray[bad[:2]].tolist(), win[bad[:8]].tolist())


# -------------------------------------------------------------- refusals --
def _refused(m, **edit):
    L = _lib()
    desc, keep = m.desc()
    for k, v in edit.items():
        setattr(desc, k, v)
    rc = L.rtp_mesh_build_host(desc, 0, 0, None, None, None, None, None, None)
    return rc, L.rtp_last_error().decode()


def test_descriptor_refusals():
    from raytracingtherestofyourlife_amd._lib import RTP_ERR_INVALID_ARGUMENT as BAD

    m = _meshes.cornell(0)
    assert _refused(m)[0] == 0
    rc, msg = _refused(m, n_quads=0)
    assert rc == BAD and "1 to 4194304 quads" in msg
    # nine spheres
    z9 = _meshes.Mesh(m.points, m.quads, m.quad_mat, m.quad_tex, [m.spheres[0]] * 9, m.mat_type, m.tex_type, m.tex,
                      m.light, m.light_sphere_point, m.ior)
    rc, msg = _refused(z9)
    assert rc == BAD and "at most 8 spheres" in msg
    eight = _meshes.Mesh(m.points, m.quads, m.quad_mat, m.quad_tex, [m.spheres[0]] * 8, m.mat_type, m.tex_type,
                         m.tex, m.light, m.light_sphere_point, m.ior)
    assert _refused(eight)[0] == 0
    # ids out of range, with rtp_set_scene's messages
    q = m.quads.copy()
    q[3, 2] = len(m.points)
    bad_q = _meshes.Mesh(m.points, q, m.quad_mat, m.quad_tex, m.spheres, m.mat_type, m.tex_type, m.tex, m.light,
                         m.light_sphere_point, m.ior)
    rc, msg = _refused(bad_q)
    assert rc == BAD and msg == "rtp_set_scene: quad point id out of range"
    mats = m.quad_mat.copy()
    mats[1] = len(m.mat_type)
    bad_m = _meshes.Mesh(m.points, m.quads, mats, m.quad_tex, m.spheres, m.mat_type, m.tex_type, m.tex, m.light,
                         m.light_sphere_point, m.ior)
    rc, msg = _refused(bad_m)
    assert rc == BAD and msg == "rtp_set_scene: quad material/texture index out of range"
    pts = m.points.copy()
    pts[m.quads[5, 1], 2] = np.inf
    bad_p = _meshes.Mesh(pts, m.quads, m.quad_mat, m.quad_tex, m.spheres, m.mat_type, m.tex_type, m.tex, m.light,
                         m.light_sphere_point, m.ior)
    rc, msg = _refused(bad_p)
    assert rc == BAD and msg == "rtp_set_scene_mesh: a quad vertex is not finite"
    rc, msg = _refused(m, light_sphere_point=-1)
    assert rc == BAD and msg == "rtp_set_scene: light sphere point id out of range"
    bad_l = _meshes.Mesh(m.points, m.quads, m.quad_mat, m.quad_tex, m.spheres, m.mat_type, m.tex_type, m.tex,
                         (8, 9, 10, len(m.points)), m.light_sphere_point, m.ior)
    rc, msg = _refused(bad_l)
    assert rc == BAD and msg == "rtp_set_scene: light quad point id out of range"


def test_mapper_picks_the_mesh_entry_above_256_distinct_quads():
    from raytracingtherestofyourlife_amd import mapper

    t = _meshes.tess()
    assert mapper._distinct_quads(t.points, t.quads, t.quad_mat, t.quad_tex) > 256
    c = _meshes.cornell(0)
    assert mapper._distinct_quads(c.points, c.quads, c.quad_mat, c.quad_tex) <= 256
