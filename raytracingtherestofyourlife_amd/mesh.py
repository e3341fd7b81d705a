"""Mesh scenes: helpers for cell sets that hold triangle cells
(include/rtp_mesh.h, DESIGN.md 4.11 "Triangle cells").

A triangle cell is a cell (a, b, c, c): the reference's quad test makes of it
exactly its first triangle, and the mesh BVH always bounds it tightly.  A
bent quad -- a quad of a curved surface -- gets an unbounded box that every
ray tests; split in two triangles it renders at the walk's speed.

    which = rtp.unbounded_cells(coords, cells, sphere_points, sphere_radius)
    cells, mat, tex, parent = rtp.triangulate(cells, mat, tex, which)
    device.set_scene_mesh(coords, cells, mat, tex, ...)
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

HUGE = np.float32(2.0 ** 100)  # csrc/rtp_layout.hpp kMeshHuge: the pad of an unbounded box


def cell_rows(quad_points):
    """Connectivity for a mesh scene: rows (a, b, c) of an [N, 3] array or
    tensor become the triangle cells (a, b, c, c), on the device the tensor
    lives on; anything else is returned as it is."""
    shape = getattr(quad_points, "shape", None)
    if shape is None:
        quad_points = np.asarray(quad_points)
        shape = quad_points.shape
    if len(shape) == 2 and shape[1] == 3:
        return quad_points[:, [0, 1, 2, 2]]
    return quad_points


def _is_tensor(a) -> bool:
    return type(a).__module__.split(".")[0] == "torch"


def triangulate(quad_points, quad_mat, quad_tex, which=None):
    """Split quads in two triangle cells: (cells [N', 4], mat [N'], tex [N'],
    parent [N']), parent the index of the quad a cell came from.

    Every selected quad (v00, v10, v11, v01) is replaced, in its place, by
    (v00, v10, v01, v01) and (v11, v01, v10, v10); both keep the quad's
    orientation, material and texture.  ``which``: a boolean mask over the
    quads or a list of quad indices (None: every quad) -- unbounded_cells()
    gives the natural one.  A selected row that is a triangle cell already,
    (a, b, c, c) by id, is kept as it is.  Indexing and concatenation only:
    numpy arrays give numpy arrays, torch tensors give tensors on the same
    device.

    The two halves are not the reference's bent quad.  The reference reports
    every hit of a quad at t on its first triangle's plane and accepts a bent
    one beyond its edges, arbitrarily far away for grazing rays; each half
    reports t on its own plane and accepts nothing beyond its edges.  That is
    the point of splitting: a planar quad renders as before wherever the two
    agree, a bent one becomes the surface it was meant to be."""
    if _is_tensor(quad_points):
        import torch

        qp = quad_points.reshape(-1, 4)
        n = qp.shape[0]
        idx = torch.arange(n, device=qp.device)
        if which is None:
            sel = torch.ones(n, dtype=torch.bool, device=qp.device)
        else:
            w = torch.as_tensor(which, device=qp.device)
            sel = w if w.dtype == torch.bool else torch.zeros(n, dtype=torch.bool, device=qp.device).index_fill_(
                0, w.to(torch.int64), True)
        cat = torch.cat
    else:
        qp = np.asarray(quad_points).reshape(-1, 4)
        n = qp.shape[0]
        idx = np.arange(n)
        if which is None:
            sel = np.ones(n, dtype=bool)
        else:
            w = np.asarray(which)
            sel = w if w.dtype == bool else np.isin(idx, w)
        quad_mat, quad_tex = np.asarray(quad_mat), np.asarray(quad_tex)
        cat = np.concatenate
    if sel.shape[0] != n:
        raise ValueError(f"triangulate: a mask of {sel.shape[0]} entries for {n} quads")
    # a row that names one point as third and fourth id is a triangle cell already: its second half would be
    # (c, c, b, b), a cell without area that every ray tests; it stays as it is, selected or not
    sel = sel & (qp[:, 2] != qp[:, 3])
    # per quad three candidate rows -- the quad, its two triangles -- of which the mask keeps one or two
    rows = cat([qp[:, None, :], qp[:, [0, 1, 3, 3]][:, None, :], qp[:, [2, 3, 1, 1]][:, None, :]], 1).reshape(-1, 4)
    keep = cat([~sel[:, None], sel[:, None], sel[:, None]], 1).reshape(-1)
    parent = cat([idx[:, None], idx[:, None], idx[:, None]], 1).reshape(-1)[keep]
    return rows[keep], quad_mat[parent], quad_tex[parent], parent


def _host(a, dtype):
    if _is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def mesh_pads(coords, cells, sphere_points=(), sphere_radius=()):
    """The pad of every cell's box as the host builder of rtp_set_scene_mesh
    computes it (float32 [N]; HUGE: the unbounded box).  The pads depend on the
    cells and, through the scene's bounding box, on the spheres; materials and
    lights play no part.  No device is touched."""
    from .device import scene_desc

    pts = _host(coords, np.float32).reshape(-1, 3)
    rows = _host(cell_rows(cells), np.int32).reshape(-1, 4)  # ([N, 3]: triangle cells)
    n = len(rows)
    sp, sr = _host(sphere_points, np.int32).reshape(-1), _host(sphere_radius, np.float32).reshape(-1)
    if sp.size == 0:
        # the descriptor needs one sphere: a vertex of the mesh with a radius
        # that vanishes beside any float32 coordinate leaves the bounds alone
        first = int(rows[0, 0]) if n and 0 <= rows[0, 0] < len(pts) else 0
        sp, sr = np.array([first], dtype=np.int32), np.array([1e-30], dtype=np.float32)
    zeros = np.zeros(n, dtype=np.int32)
    none = np.zeros(len(sp), np.int32)
    desc, keep = scene_desc(pts, rows, zeros, zeros, sp, sr, none, none, [0], [0], np.zeros((1, 3), np.float32),
                            (int(sp[0]),) * 4, int(sp[0]), 1.5)
    pads = np.zeros(n, dtype=np.float32)
    # (byref: what both a typed and a void* parameter take, should a caller have retyped the shared library's hook)
    _lib.check(_lib.load().rtp_mesh_build_host(ctypes.byref(desc), 0, 0, None, None, None, None, _lib.ptr(pads), None))
    del keep
    return pads


def unbounded_cells(coords, cells, sphere_points=(), sphere_radius=()):
    """Boolean mask [N] of the cells that rtp_set_scene_mesh gives an unbounded
    box (every ray tests them): the bent quads of a curved surface.  It is the
    natural ``which`` of triangulate(); Device.mesh_counts() reports how many
    the current scene holds."""
    return mesh_pads(coords, cells, sphere_points, sphere_radius) == HUGE
