"""Mesh scenes with triangle cells (include/rtp_mesh.h: a cell whose v11 and
v01 compare equal, in particular (a, b, c, c)), for the triangle-cell tests.
Plain numpy, fixed seeds, no GPU; every scene fits the oracle (2048 cells,
8192 points).  The scenes are registered in _meshes.SCENES at import, so
_meshes.rays() and the helpers of _meshes serve them like its own."""
from __future__ import annotations

import functools

import numpy as np

import _meshes
import _scenes
from _scenes import GLASS, GREEN, RED, WHITE

F = np.float32
HUGE = F(2.0 ** 100)  # rtp_layout.hpp kMeshHuge
N_ROOM = 5            # _meshes._room: the cells in front of every terrain
MIN_SINE = 2.0 ** -10
N_SLIVERS, N_BY_VALUE = 64, 5


def hill_height(x, z):
    return 0.08 * (0.5 + 0.5 * np.sin(7 * x + 1) * np.cos(5 * z)) + 0.02


def _hill_grid(z, nx, nz):
    """(nx + 1) x (nz + 1) shared vertices over [0, 1]^2 at hill_height; returns
    the terrain's quads (v00, v10, v11, v01) as point ids, [nx * nz, 4], and
    their (material, texture) pairs: a checkerboard."""
    xs, zs = np.linspace(0, 1, nx + 1), np.linspace(0, 1, nz + 1)
    X, Z = np.meshgrid(xs, zs, indexing="ij")
    base = z.add_points(np.stack([X, hill_height(X, Z), Z], -1).reshape(-1, 3))
    i, j = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    a = base + i * (nz + 1) + j
    ids = np.stack([a, a + (nz + 1), a + (nz + 1) + 1, a + 1], -1).reshape(-1, 4)
    mt = [WHITE if (k // nz + k % nz) % 2 else GREEN for k in range(nx * nz)]
    return ids, mt


def _add_cells(z, ids, mt, split):
    for q, m in zip(ids.tolist(), mt):
        if split:  # (v00, v10, v01, v01) and (v11, v01, v10, v10)
            z.quads.append([(q[0], q[1], q[3], q[3]), *m])
            z.quads.append([(q[2], q[3], q[1], q[1]), *m])
        else:
            z.quads.append([tuple(q), *m])


def _lit_room():
    z = _scenes.Zoo()
    _meshes._room(z)
    z.add_sphere((0.6, 0.45, 0.5), 0.125, GLASS)
    z.light_sphere_point = z.spheres[0][0]
    return z


@functools.lru_cache(maxsize=None)
def hills(n, split=True):
    """The lit room over the curved terrain of n cells (n a power of two, or a
    square), each a bent quad (split=False) or two triangle cells."""
    nx = 1 << ((n.bit_length() - 1) // 2) if n & (n - 1) == 0 else int(round(n ** 0.5))
    nz = n // nx
    assert nx * nz == n
    z = _lit_room()
    _add_cells(z, *_hill_grid(z, nx, nz), split)
    return _meshes.Mesh.from_zoo(z)


def hills_tri():
    """30 x 30 terrain cells as 1800 triangle cells: 1805 cells."""
    m = hills(900, True)
    assert len(m.quads) == 1805 and len(m.points) <= 8192
    return m


def hills_quads():
    """The same terrain as 900 bent quads."""
    m = hills(900, False)
    assert len(m.quads) == 905
    return m


@functools.lru_cache(maxsize=None)
def mixed():
    """Planar quads and triangle cells side by side: the tilted cone frustum
    of _meshes.facets() (96 planar trapezoids) closed by a fan of 32 triangle
    cells over an apex, and a 16 x 16 curved terrain of 512 triangle cells."""
    z = _scenes.Zoo()
    _meshes._room(z)
    R = _scenes._rotation((1, 0.3, 0.2), 20.0)
    rings, seg = 3, 32
    shift = np.array([0.35, 0.2, 0.6])
    ang = np.linspace(0, 2 * np.pi, seg + 1)[:-1]
    ring = lambda r, y: np.stack([r * np.cos(ang), np.full(seg, y), r * np.sin(ang)], -1) @ R.T + shift
    base = z.add_points(np.concatenate([ring(0.18 - 0.04 * k, 0.12 * k) for k in range(rings + 1)]))
    apex = z.add_points(np.array([0.0, 0.12 * rings + 0.07, 0.0]) @ R.T + shift)
    for k in range(rings):
        for s in range(seg):
            s1 = (s + 1) % seg
            z.quads.append([(base + k * seg + s, base + k * seg + s1, base + (k + 1) * seg + s1, base + (k + 1) * seg + s),
                            *(RED, WHITE, GREEN)[k % 3]])
    top = base + rings * seg
    for s in range(seg):
        z.quads.append([(top + s, top + (s + 1) % seg, apex, apex), *(WHITE, RED)[s % 2]])
    z.add_sphere((0.72, 0.3, 0.35), 0.15625, GLASS)
    z.light_sphere_point = z.spheres[0][0]
    _add_cells(z, *_hill_grid(z, 16, 16), True)
    m = _meshes.Mesh.from_zoo(z)
    assert len(m.quads) == N_ROOM + 96 + 32 + 512
    return m


def sliver_sines():
    """The sine of the corner at v00 of slivers()' first N_SLIVERS cells: from
    1 down to 2^-12, through rtp_layout.hpp kMeshMinSine = 2^-10."""
    return 2.0 ** (-12.0 * np.arange(N_SLIVERS) / (N_SLIVERS - 1))


@functools.lru_cache(maxsize=None)
def slivers():
    """The lit room with 64 triangle cells whose corner at v00 narrows from a
    right angle to a sine of 2^-12 (each with points of its own, v11 and v01
    one id), then N_BY_VALUE triangle cells whose v11 and v01 are two points
    with equal coordinates -- the last with +0 against -0."""
    z = _lit_room()
    rng = np.random.default_rng(41)
    e = 0.1
    for k, s in enumerate(sliver_sines()):
        o = np.array([0.08 + 0.105 * (k % 8), 0.1 + 0.06 * (k // 8 % 3), 0.08 + 0.105 * (k // 8)])
        Rk = _scenes._rotation(rng.normal(size=3), rng.uniform(0, 30))
        a, b = Rk @ np.array([e, 0, 0]), Rk @ np.array([e * np.sqrt(1 - s * s), 0, e * s])
        base = z.add_points([o, o + a, o + b])
        z.quads.append([(base, base + 1, base + 2, base + 2), *(WHITE, RED, GREEN)[k % 3]])
    for k in range(N_BY_VALUE):
        o = np.array([0.15 + 0.15 * k, 0.55, 0.3 + 0.1 * k])
        Rk = _scenes._rotation(rng.normal(size=3), rng.uniform(0, 40))
        c = o + Rk @ np.array([0, 0, 0.12])
        if k == N_BY_VALUE - 1:  # on the wall x = 0: v11.x = +0, v01.x = -0
            o, c = np.array([0.3, 0.6, 0.5]), np.array([0.0, 0.65, 0.55])
        z.add_quad([o, o + Rk @ np.array([0.12, 0, 0]), c, c], (GREEN, WHITE)[k % 2])
        if k == N_BY_VALUE - 1:
            z.points[-1, 0] = F(-0.0)
    m = _meshes.Mesh.from_zoo(z)
    assert len(m.quads) == N_ROOM + N_SLIVERS + N_BY_VALUE
    last = m.quads[-1]
    assert last[2] != last[3] and (m.points[last[2]] == m.points[last[3]]).all() and np.signbit(m.points[last[3], 0])
    return m


TRI_SCENES = {"hills_tri": hills_tri, "hills_quads": hills_quads, "mixed": mixed, "slivers": slivers}
_meshes.SCENES.update(TRI_SCENES)


def is_triangle(m):
    """Per cell: v11 and v01 compare equal in all three coordinates."""
    V = m.verts()
    return (V[:, 2] == V[:, 3]).all(1)


def tri_pad_formula(m, reach, cos_min):
    """The triangle cell's pad restated in float64, per cell (inf: unbounded):
    (2^-18 reach / s) / cos_min + slab, s the sine of the corner at v00, over
    the three vertices; and the three-vertex box (mn, mx)."""
    V = m.verts().astype(np.float64)
    e01, e03 = V[:, 1] - V[:, 0], V[:, 3] - V[:, 0]
    A1 = np.linalg.norm(np.cross(e01, e03), axis=1)
    T = V[:, [0, 1, 3]]
    mn, mx = T.min(1), T.max(1)
    with np.errstate(all="ignore"):
        s = A1 / (np.linalg.norm(e01, axis=1) * np.linalg.norm(e03, axis=1))
        amax = np.maximum(np.abs(mn), np.abs(mx)).max(1)
        pad = (2.0 ** -18 * reach / s) / cos_min + 1e-5 + 2.0 ** -16 * amax + 2.0 ** -18 * reach
        huge = ~(A1 > 0) | ~np.isfinite(A1) | ~(s >= MIN_SINE) | ~(pad < reach)
    return np.where(huge, np.inf, pad), mn, mx
