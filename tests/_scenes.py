"""Generated scenes for the parity tests: a room that holds every reachable
(kind, exact-parallelogram) pair of the renderer's quad classification, and
small variants of it that sit on each side of the host's scene-setup gates
(the closest-hit prefilter's conditions, the 256-quad limit, kept and dropped
duplicates).  Plain numpy and ctypes over oracle_ctypes.Scene: no GPU.

classify() restates the classification from its definition (rtp_layout.hpp
kQuadKind, rtp_mesh_cell.hpp mesh_cell_record); nothing here is imported from the library,
so the tests can hold the library's own tally against it."""
from __future__ import annotations

import numpy as np

F = np.float32

# --------------------------------------------------------- classification --
# Masks of the exact non-zero components (bit k: component k) of the edges
# e01 = v10 - v00, e03 = v01 - v00, e21 = v10 - v11, e23 = v01 - v11, in
# float32.  Kinds 1..6: axis-plane rectangles (e01 along one axis, e03 along
# another); 7..9: faces of a box turned about y; 10: general first triangle,
# second triangle flat in y; anything else is kind 0.
KIND_OF_MASKS = {
    (1, 2, 2, 1): 1, (1, 4, 4, 1): 2, (2, 1, 1, 2): 3, (2, 4, 4, 2): 4, (4, 1, 1, 4): 5, (4, 2, 2, 4): 6,
    (5, 2, 2, 5): 7, (2, 5, 5, 2): 8, (5, 5, 5, 5): 9,
    (7, 7, 5, 5): 10,
}
N_KINDS = 11
MAX_QUADS = 256   # distinct quads a scene may hold
MAX_PRE = 32      # axis-plane quads the closest-hit prefilter takes
PRE_LIM = 16.0    # ... and the largest |vertex coordinate| of them

# Every (kind, para) pair a quad can have.  Kinds 1..8 are always exact
# parallelograms, so (1..8, False) cannot exist and is not chased: an exact
# zero of a float32 difference means equal coordinates, and the masks then
# leave v11 no freedom.  For kind 7 (e01, e23 without y; e03, e21 along y):
# v11 = (v10.x, v01.y, v10.z), v01 = (v00.x, ., v00.z) and v10.y = v00.y, hence
# e21.y = v00.y - v01.y = -e03.y and e23.xz = v00.xz - v10.xz = -e01.xz bit
# for bit; kinds 1..6 and 8 alike.  Kind 9 can be either.  Kind 10 has e01.y
# non-zero and e23.y zero: never a parallelogram.
REACHABLE = ([(k, True) for k in range(1, 9)] + [(9, False), (9, True), (0, False), (0, True), (10, False)])


def _mask(e):
    return int((e[..., 0] != 0) * 1 + (e[..., 1] != 0) * 2 + (e[..., 2] != 0) * 4)


def classify(points, quads):
    """[(kind, para)] per quad; points float32 [n, 3], quads int [nq, 4] as
    (v00, v10, v11, v01)."""
    P = np.ascontiguousarray(points, dtype=F).reshape(-1, 3)
    out = []
    for i0, i1, i2, i3 in np.asarray(quads).reshape(-1, 4):
        v00, v10, v11, v01 = P[i0], P[i1], P[i2], P[i3]
        e01, e03, e21, e23 = v10 - v00, v01 - v00, v10 - v11, v01 - v11  # float32
        kind = KIND_OF_MASKS.get((_mask(e01), _mask(e03), _mask(e21), _mask(e23)), 0)
        para = bool(np.all(-e01 == e23) and np.all(-e03 == e21))
        out.append((kind, para))
    return out


def tally(pairs):
    """{(kind, para): count}."""
    t = {}
    for p in pairs:
        t[p] = t.get(p, 0) + 1
    return t


def scan_order(pairs):
    """The device's quad order: grouped by kind in the order 1..10, 0, each
    group in scene order (rtp_layout.hpp DevScene::kind_begin).  Returns the
    scene index of each scan position."""
    return sorted(range(len(pairs)), key=lambda q: ((pairs[q][0] - 1) % N_KINDS, q))


# ------------------------------------------------------------------ scene --
RED, WHITE, GREEN, LIGHT, GLASS = (0, 0), (1, 1), (2, 2), (3, 3), (4, 0)  # (material, texture) as the Cornell box
MAT_TYPE = [0, 0, 0, 1, 2]  # Lambertian x3, emissive, dielectric
TEX_TYPE = [0, 1, 2, 3, 0]
TEX = [[0.65, 0.05, 0.05], [0.73, 0.73, 0.73], [0.12, 0.45, 0.15], [15, 15, 15]]


class Zoo:
    """A scene under construction: float32 points, quads as four point ids."""

    def __init__(self):
        self.points = np.zeros((0, 3), dtype=F)
        self.quads = []    # [(i0, i1, i2, i3), material, texture]
        self.spheres = []  # [point id, radius (float32), material, texture]
        self.light = (8, 9, 10, 11)
        self.light_sphere_point = -1
        self.ior = 1.5
        self.scale = 1.0
        # the reference's camera (main.cc:616-622)
        self.cam = dict(position=np.array([278 / 555.0, 278 / 555.0, -800 / 555.0], dtype=F),
                        look_at=np.array([278 / 555.0, 278 / 555.0, 278 / 555.0], dtype=F),
                        view_up=np.array([0, 1, 0], dtype=F), fov_y=40.0)

    def add_points(self, p):
        base = len(self.points)
        self.points = np.concatenate([self.points, np.asarray(p, dtype=np.float64).reshape(-1, 3).astype(F)], 0)
        return base

    def add_quad(self, verts, mt, at=None):
        """verts: (v00, v10, v11, v01), rounded to float32 here.  at: index in
        the quad list (default: the end); the points always go to the end."""
        base = self.add_points(verts)
        q = [(base, base + 1, base + 2, base + 3), mt[0], mt[1]]
        self.quads.insert(len(self.quads) if at is None else at, q)

    def add_sphere(self, centre, radius, mt):
        self.spheres.append([self.add_points(centre), F(radius), mt[0], mt[1]])

    # views ------------------------------------------------------------
    def quad_points(self):
        return np.array([q[0] for q in self.quads], dtype=np.int32).reshape(-1, 4)

    def verts(self):
        """(nq, 4, 3) float32."""
        return self.points[self.quad_points()]

    def classify(self):
        return classify(self.points, self.quad_points())

    def camera(self, rtp):
        cam = rtp.Camera()
        cam.SetPosition(self.cam["position"])
        cam.SetLookAt(self.cam["look_at"])
        cam.SetViewUp(self.cam["view_up"])
        cam.SetFieldOfView(self.cam["fov_y"])
        cam.SetClippingRange(0.1 * float(self.scale), 5.0 * float(self.scale))
        return cam

    def oracle_camera(self, oracle, nx, ny):
        return oracle.camera_setup(nx, ny, **self.cam)

    def scene(self, oracle):
        """The oracle's Scene (what set_scene_from_oracle uploads)."""
        sc = oracle.Scene()
        n = len(self.points)
        sc.n_points = n
        np.ctypeslib.as_array(sc.points)[:n] = self.points
        sc.n_quads = len(self.quads)
        for q, (ids, m, t) in enumerate(self.quads):
            sc.quad_ids[q][0] = q  # the cell id: a field index (-direct mode's scalar)
            for k in range(4):
                sc.quad_ids[q][1 + k] = ids[k]
            sc.quad_mat[q], sc.quad_tex[q] = m, t
        sc.n_spheres = len(self.spheres)
        for k, (p, r, m, t) in enumerate(self.spheres):
            sc.sphere_point[k], sc.sphere_radius[k], sc.sphere_mat[k], sc.sphere_tex[k] = p, r, m, t
        sc.n_mat = sc.n_tex_type = 5
        for i in range(5):
            sc.mat_type[i], sc.tex_type[i] = MAT_TYPE[i], TEX_TYPE[i]
        sc.n_tex = 4
        np.ctypeslib.as_array(sc.tex)[:4] = np.asarray(TEX, dtype=F)
        sc.light_box_pointids[0] = 0
        for k in range(4):
            sc.light_box_pointids[1 + k] = self.light[k]
        sc.light_sphere_point = self.light_sphere_point
        sc.ior = self.ior
        # per-point values for the -direct mode's colour AOV (any spread will do)
        sc.n_field = n
        np.ctypeslib.as_array(sc.field)[:n] = ((np.arange(n) * 37) % 101).astype(F) / F(101)
        return sc


def _rect(o, a, b):
    """v00 = o, e01 = a, e03 = b: an exact parallelogram when the sums are exact."""
    o, a, b = (np.asarray(v, dtype=np.float64) for v in (o, a, b))
    return [o, o + a, o + a + b, o + b]


def _rotation(axis, deg):
    """Rodrigues' rotation matrix, float64."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.deg2rad(deg)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def _box_faces(size, R, shift):
    """The six faces of [0, size] turned by R (float64) and moved by shift:
    four sides (vertex orders alternate, so a box turned about y gives kinds 7
    and 8 twice each), top, bottom."""
    sx, sy, sz = size
    c = lambda x, y, z: R @ np.array([x, y, z], dtype=np.float64) + np.asarray(shift, dtype=np.float64)
    return [
        [c(0, 0, 0), c(sx, 0, 0), c(sx, sy, 0), c(0, sy, 0)],      # e01 across, e03 up
        [c(sx, 0, 0), c(sx, sy, 0), c(sx, sy, sz), c(sx, 0, sz)],  # e01 up, e03 across
        [c(sx, 0, sz), c(0, 0, sz), c(0, sy, sz), c(sx, sy, sz)],  # e01 across, e03 up
        [c(0, 0, sz), c(0, sy, sz), c(0, sy, 0), c(0, 0, 0)],      # e01 up, e03 across
        [c(0, sy, 0), c(sx, sy, 0), c(sx, sy, sz), c(0, sy, sz)],  # top
        [c(0, 0, 0), c(sx, 0, 0), c(sx, 0, sz), c(0, 0, sz)],      # bottom
    ]


def zoo(scale=1.0):
    """A room in [0, 1]^3, open toward the camera like the Cornell box, times
    ``scale`` in float32.  Light coupling as the reference's: the light quad is
    points 8..11 in a plane y = const, the light sphere is sphere 0."""
    z = Zoo()
    # the room: one vertex order per axis-plane kind
    z.add_quad([(1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)], GREEN)  # right wall: e01 || y, e03 || z (kind 4)
    z.add_quad([(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)], RED)    # left wall: e01 || z, e03 || y (6)
    ly = 511 / 512
    z.add_quad([(0.375, ly, 0.375), (0.625, ly, 0.375), (0.625, ly, 0.625), (0.375, ly, 0.625)], LIGHT)  # (2)
    z.add_quad([(0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)], WHITE)  # ceiling: e01 || z, e03 || x (5)
    z.add_quad([(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)], WHITE)  # floor: e01 || x, e03 || z (2)
    z.add_quad([(0, 0, 1), (1, 0, 1), (1, 0.5, 1), (0, 0.5, 1)], WHITE)  # back wall, lower: e01 || x, e03 || y (1)
    z.add_quad([(0, 0.5, 1), (0, 1, 1), (1, 1, 1), (1, 0.5, 1)], WHITE)  # back wall, upper: e01 || y, e03 || x (3)
    # a tall box turned about y (in double, rounded to float32): sides (7, T) and (8, T), top and bottom (9, F)
    for f in _box_faces((0.3, 0.6, 0.3), _rotation((0, 1, 0), 15.0), (0.12, 0.0, 0.6)):
        z.add_quad(f, WHITE)
    # (9, T): a rhombus in a y-plane with dyadic edges
    z.add_quad(_rect((0.125, 0.625, 0.25), (0.25, 0, 0.0625), (0.0625, 0, 0.1875)), GREEN)
    # (0, T): a dyadic general parallelogram
    z.add_quad(_rect((0.5, 0.25, 0.25), (0.25, 0.125, 0.0625), (-0.0625, 0.25, 0.125)), RED)
    # (0, F): a small box turned about a general axis, a non-planar quad and a trapezoid inside a z-plane
    for f in _box_faces((0.16, 0.16, 0.16), _rotation((1, 2, 3), 35.0), (0.62, 0.55, 0.7)):
        z.add_quad(f, GREEN)
    z.add_quad([(0.55, 0.05, 0.6), (0.8, 0.02, 0.65), (0.85, 0.25, 0.8), (0.6, 0.2, 0.7)], WHITE)
    z.add_quad([(0.55, 0.1, 0.95), (0.9, 0.1, 0.95), (0.8, 0.4, 0.95), (0.55, 0.4, 0.95)], RED)
    # (10, F): v10, v11, v01 share one y, v00 is raised (the reference's small box top has such a vertex)
    R = _rotation((0, 1, 0), 30.0)
    k10 = [R @ np.array(v, dtype=np.float64) + np.array([0.3, 0.8, 0.4]) for v in
           [(-0.1, 0.03, -0.1), (0.1, 0, -0.1), (0.1, 0, 0.1), (-0.1, 0, 0.1)]]
    z.add_quad(k10, WHITE)
    # a glass pane in an x-plane
    z.add_quad([(0.9375, 0.25, 0.25), (0.9375, 0.25, 0.75), (0.9375, 0.75, 0.75), (0.9375, 0.75, 0.25)], GLASS)
    # three spheres (below the sphere-BVH threshold): glass, Lambertian, a small emissive one
    z.add_sphere((0.7, 0.15625, 0.35), 0.15625, GLASS)
    # (sphere 1 is the larger: with the light sphere's point at its centre and sphere 0's radius, no
    # surface point lies inside that light sphere, whose pdf is NaN from inside)
    z.add_sphere((0.3, 0.1875, 0.25), 0.1875, GREEN)
    z.add_sphere((0.85, 0.8, 0.7), 0.03125, LIGHT)
    z.light_sphere_point = z.spheres[0][0]
    if scale != 1.0:
        s = F(scale)
        z.scale = float(scale)
        z.points = (z.points * s).astype(F)
        for sp in z.spheres:
            sp[1] = F(sp[1] * s)
        z.cam["position"] = (z.cam["position"] * s).astype(F)
        z.cam["look_at"] = (z.cam["look_at"] * s).astype(F)
    return z


# ------------------------------------------- a float64 closest hit --
def pixel_centre_rays(cam, nx, ny):
    """camera_ray_at with both jitter draws 0.5f, in float32 (rtp_kernels.hip)."""
    eye, nlook, dx, dy = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    pix = np.arange(nx * ny)
    pi, pj = (pix % nx).astype(F), (pix // nx).astype(F)
    a = (F(2) * (pi + (F(1) - F(0.5))) - F(nx)) / F(2)
    b = (F(2) * (pj + F(0.5)) - F(ny)) / F(2)
    rd = (nlook[None, :] + dx[None, :] * a[:, None]) + dy[None, :] * b[:, None]
    rd = np.where(rd == 0, rd + F(0.0000001), rd).astype(F)
    mag = np.sqrt((rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1]) + rd[:, 2] * rd[:, 2])
    d = (rd / mag[:, None]).astype(F)
    return np.broadcast_to(eye, d.shape).astype(np.float64), d.astype(np.float64)


def hits_f64(z, o, d):
    """t per (primitive, ray) in float64, inf where missed: the quads in scene
    order by the Lagae-Dutre test as test_gpu_guides.quad_hits_f64 states it
    (t and (alpha, beta) in the plane of v00, v10, v01; past alpha + beta = 1
    the corner at v11 decides), then the spheres (the nearer root beyond
    0.001, else the farther)."""
    V = z.verts().astype(np.float64)
    rows = []

    def moller_trumbore(a, b, c):
        e1, e2 = b - a, c - a
        pv = np.cross(d, e2)
        det = pv @ e1
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            tv = o - a
            u = (tv * pv).sum(1) * inv
            qv = np.cross(tv, e1)
            return np.abs(det) > 1e-14, u, (d * qv).sum(1) * inv, (qv @ e2) * inv

    for v00, v10, v11, v01 in V:
        ok, al, be, t = moller_trumbore(v00, v10, v01)
        ok2, ap, bp, _ = moller_trumbore(v11, v01, v10)
        with np.errstate(all="ignore"):
            hit = ok & (al >= 0) & (be >= 0) & (t > 0.001)
            hit &= (al + be <= 1) | (ok2 & (ap >= 0) & (bp >= 0))
        rows.append(np.where(hit, t, np.inf))
    for p, r, _, _ in z.spheres:
        oc = o - z.points[p].astype(np.float64)
        bq, aq = (oc * d).sum(1), (d * d).sum(1)
        disc = bq * bq - aq * ((oc * oc).sum(1) - float(r) ** 2)
        root = np.sqrt(np.maximum(disc, 0.0))
        t1, t2 = (-bq - root) / aq, (-bq + root) / aq
        t = np.where(t1 > 0.001, t1, t2)
        rows.append(np.where((disc > 0) & (t > 0.001), t, np.inf))
    return np.array(rows)


# A second camera, above the room's opening looking down: it sees the tops
# (the default camera, level with the room's middle, sees kind 9 edge-on).
HIGH_CAM = dict(position=np.array([0.5, 0.93, -1.0], dtype=F), look_at=np.array([0.5, 0.35, 0.5], dtype=F),
                view_up=np.array([0, 1, 0], dtype=F), fov_y=45.0)


def clear_first_hits(z, cam12, nx, ny, rel=1e-4):
    """Float64 first hits of the pixel-centre rays of a camera (the oracle's 12
    camera constants): (T [primitive, ray], first [ray], t [ray], clear
    [ray]); clear: a hit whose runner-up is farther than a relative ``rel``
    in t.  Primitive rows: the quads in scene order, then the spheres; equal t
    goes to the lower row, as in the reference's scan."""
    o, d = pixel_centre_rays(cam12, nx, ny)
    T = hits_f64(z, o, d)
    cols = np.arange(T.shape[1])
    first = T.argmin(axis=0)
    t = T[first, cols]
    rest = T.copy()
    rest[first, cols] = np.inf
    clear = np.isfinite(t) & (rest.min(axis=0) > t * (1 + rel))
    return T, first, t, clear


# --------------------------------------------------------------- variants --
def scaled(s):
    """555: the reference's native units; 16 and 17: the two sides of the
    prefilter's coordinate limit.  Radii and camera scale too."""
    return zoo(scale=s)


def _floor_tile(i, j, y):
    """An axis-plane tile (kind 2) of the 8 x 8 grid over the floor."""
    return _rect((i / 8 + 1 / 64, y, j / 8 + 1 / 64), (3 / 32, 0, 0), (0, 0, 3 / 32))


def many_axis():
    """36 more axis-plane quads just above the floor: more than the prefilter takes."""
    z = zoo()
    for i in range(6):
        for j in range(6):
            z.add_quad(_floor_tile(i + 1, j + 1, 1 / 1024), WHITE if (i + j) % 2 else RED)
    return z


def _rhombus_tile(k):
    """Tile k of a 16 x 16 grid of small dyadic rhombi (kind 9, exact
    parallelograms: no axis-plane quad is added) just above the floor."""
    i, j = k % 16, k // 16
    return _rect((i / 16 + 1 / 256, 1 / 512, j / 16), (7 / 128, 0, 1 / 256), (1 / 256, 0, 7 / 128))


def _tiled(n_distinct):
    z = zoo()
    k = 0
    while len(z.quads) < n_distinct:
        z.add_quad(_rhombus_tile(k), (WHITE, RED, GREEN)[k % 3])
        k += 1
    return z


def full():
    """Exactly 256 distinct quads, and three bit-identical copies of earlier
    quads (same vertices, material and texture: dropped by the host) at low
    indices, so that most kept quads change index: 259 quads go in."""
    z = _tiled(MAX_QUADS)
    for src, at in ((0, 2), (4, 6), (9, 11)):  # (source index, where its copy goes: after the source)
        ids, m, t = z.quads[src]
        z.add_quad(z.points[list(ids)], (m, t), at=at)
    assert len(z.quads) == MAX_QUADS + 3
    return z


def overfull():
    """257 distinct quads: one too many."""
    return _tiled(MAX_QUADS + 1)


def dups():
    """Three repeats that the host must keep: the red left wall again in white
    at a higher index; the white floor again in red (the same pair the other
    way round); the general parallelogram with its vertex order rotated by
    one, in green.  Equal t goes to the lower index."""
    z = zoo()
    z.add_quad(z.points[list(z.quads[1][0])], WHITE)
    z.add_quad(z.points[list(z.quads[4][0])], RED)
    ids = z.quads[14][0]
    z.add_quad(z.points[[ids[1], ids[2], ids[3], ids[0]]], GREEN)
    return z


def turned(deg):
    """Every point turned about the vertical axis through the room's centre,
    in double then float32: no axis-plane quad is left."""
    z = zoo()
    c = np.array([0.5, 0.0, 0.5])
    z.points = ((z.points.astype(np.float64) - c) @ _rotation((0, 1, 0), deg).T + c).astype(F)
    return z


def ior(n):
    z = zoo()
    z.ior = n
    return z


def light_sphere_elsewhere():
    """The light sphere's point is sphere 1's centre; its radius stays sphere 0's."""
    z = zoo()
    z.light_sphere_point = z.spheres[1][0]
    return z


# every variant a scene is accepted for (overfull() is not)
VARIANTS = {
    "zoo": zoo,
    "scaled555": lambda: scaled(555),
    "scaled16": lambda: scaled(16),
    "scaled17": lambda: scaled(17),
    "many_axis": many_axis,
    "full": full,
    "dups": dups,
    "turned1": lambda: turned(1.0),
    "turned2": lambda: turned(2.0),
    "turned3": lambda: turned(3.0),
    "ior133": lambda: ior(1.33),
    "light_sphere_elsewhere": light_sphere_elsewhere,
}


def kept_quads(z):
    """Scene indices of the quads the host keeps: a quad that repeats an
    earlier one bit for bit (vertices in order, material, texture) is dropped
    (rtp_scene_host.cpp scene_quads)."""
    V = z.verts()
    seen, kept = set(), []
    for q in range(len(z.quads)):
        key = (V[q].tobytes(), z.quads[q][1], z.quads[q][2])
        if key not in seen:
            seen.add(key)
            kept.append(q)
    return kept


def prefilter_expected(z):
    """Whether the closest-hit prefilter is on for z, from the gates'
    definition (rtp_scene_host.cpp setup_prefilter): between 1 and MAX_PRE
    axis-plane quads among the kept ones, none of their vertex coordinates
    beyond PRE_LIM."""
    pairs = z.classify()
    axis = [q for q in kept_quads(z) if 1 <= pairs[q][0] <= 6]
    if not 1 <= len(axis) <= MAX_PRE:
        return False
    return bool(np.abs(z.verts()[axis]).max() <= PRE_LIM)
