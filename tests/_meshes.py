"""Generated mesh scenes and ray populations for the mesh-scene tests
(rtp_set_scene_mesh), from fixed seeds.  Plain numpy and ctypes: no GPU.

Scenes are Mesh objects (float32 points, quads as four point ids in the order
v00, v10, v11, v01); all but grid(n) fit the oracle (2048 quads, 8192 points)
and convert with Mesh.scene(oracle).  The light coupling is the reference's:
the light quad is points 8..11, the light sphere's radius is sphere 0's."""
from __future__ import annotations

import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _scenes
from _scenes import GLASS, GREEN, LIGHT, RED, WHITE, MAT_TYPE, TEX, TEX_TYPE

F = np.float32
N_RAYS = 1 << 17
N_PARTS = 8
PART = N_RAYS // N_PARTS
PART_NAMES = ("inside", "vertices", "on_quads", "grazing", "far", "axis", "miss", "sphere")
GRAZING = 3  # the part built outside or at the edge of the promise on purpose
N_MILD = 64  # bent(): the mildly bent quads at the end of its list


class Mesh:
    def __init__(self, points, quads, quad_mat, quad_tex, spheres, mat_type, tex_type, tex, light, light_sphere_point,
                 ior=1.5, cam=None):
        self.points = np.ascontiguousarray(points, dtype=F).reshape(-1, 3)
        self.quads = np.ascontiguousarray(quads, dtype=np.int32).reshape(-1, 4)
        self.quad_mat = np.ascontiguousarray(quad_mat, dtype=np.int32)
        self.quad_tex = np.ascontiguousarray(quad_tex, dtype=np.int32)
        self.spheres = list(spheres)  # (point id, radius, material, texture)
        self.mat_type, self.tex_type = list(mat_type), list(tex_type)
        self.tex = np.asarray(tex, dtype=F).reshape(-1, 3)
        self.light, self.light_sphere_point, self.ior = tuple(int(v) for v in light), int(light_sphere_point), ior
        self.cam = cam or _scenes.Zoo().cam

    @classmethod
    def from_zoo(cls, z):
        return cls(z.points, z.quad_points(), [q[1] for q in z.quads], [q[2] for q in z.quads], z.spheres, MAT_TYPE,
                   TEX_TYPE, TEX, z.light, z.light_sphere_point, z.ior, z.cam)

    @classmethod
    def from_oracle(cls, sc):
        arr = np.ctypeslib.as_array
        nq, ns = sc.n_quads, sc.n_spheres
        sph = [(int(sc.sphere_point[k]), F(sc.sphere_radius[k]), int(sc.sphere_mat[k]), int(sc.sphere_tex[k]))
               for k in range(ns)]
        return cls(sc.points_np(), sc.quad_ids_np()[:, 1:], arr(sc.quad_mat)[:nq].copy(), arr(sc.quad_tex)[:nq].copy(),
                   sph, list(sc.mat_type[: sc.n_mat]), list(sc.tex_type[: sc.n_tex_type]),
                   arr(sc.tex)[: sc.n_tex].copy(), tuple(sc.light_box_pointids[1:5]), sc.light_sphere_point, sc.ior)

    # ------------------------------------------------------------ views --
    def verts(self):
        return self.points[self.quads]  # (nq, 4, 3)

    def set_args(self):
        """Device.set_scene / set_scene_mesh / device.scene_desc arguments."""
        sp = self.spheres
        return (self.points, self.quads, self.quad_mat, self.quad_tex, [s[0] for s in sp], [s[1] for s in sp],
                [s[2] for s in sp], [s[3] for s in sp], self.mat_type, self.tex_type, self.tex, self.light,
                self.light_sphere_point, self.ior)

    def desc(self):
        from raytracingtherestofyourlife_amd.device import scene_desc
        return scene_desc(*self.set_args())

    def scene(self, oracle):
        sc = oracle.Scene()
        n, nq = len(self.points), len(self.quads)
        assert n <= oracle.MAX_POINTS and nq <= oracle.MAX_QUADS, (n, nq)
        sc.n_points = n
        np.ctypeslib.as_array(sc.points)[:n] = self.points
        sc.n_quads = nq
        ids = np.ctypeslib.as_array(sc.quad_ids)
        ids[:nq, 0] = np.arange(nq)
        ids[:nq, 1:] = self.quads
        np.ctypeslib.as_array(sc.quad_mat)[:nq] = self.quad_mat
        np.ctypeslib.as_array(sc.quad_tex)[:nq] = self.quad_tex
        sc.n_spheres = len(self.spheres)
        for k, (p, r, m, t) in enumerate(self.spheres):
            sc.sphere_point[k], sc.sphere_radius[k], sc.sphere_mat[k], sc.sphere_tex[k] = p, r, m, t
        sc.n_mat, sc.n_tex_type, sc.n_tex = len(self.mat_type), len(self.tex_type), len(self.tex)
        for i, v in enumerate(self.mat_type):
            sc.mat_type[i] = v
        for i, v in enumerate(self.tex_type):
            sc.tex_type[i] = v
        np.ctypeslib.as_array(sc.tex)[: len(self.tex)] = self.tex
        sc.light_box_pointids[0] = 0
        for k in range(4):
            sc.light_box_pointids[1 + k] = self.light[k]
        sc.light_sphere_point = self.light_sphere_point
        sc.ior = self.ior
        sc.n_field = n
        return sc

    def camera(self, rtp, cam=None):
        c = cam or self.cam
        out = rtp.Camera()
        out.SetPosition(c["position"])
        out.SetLookAt(c["look_at"])
        out.SetViewUp(c["view_up"])
        out.SetFieldOfView(c["fov_y"])
        return out

    def bounds(self):
        lo, hi = self.points[self.quads].reshape(-1, 3).min(0), self.points[self.quads].reshape(-1, 3).max(0)
        for p, r, _, _ in self.spheres:
            lo, hi = np.minimum(lo, self.points[p] - r), np.maximum(hi, self.points[p] + r)
        return lo.astype(np.float64), hi.astype(np.float64)


# ------------------------------------------------------------------ scenes --
@functools.lru_cache(maxsize=None)
def cornell(variant):
    import oracle_ctypes as oracle
    return Mesh.from_oracle(oracle.cornell_box(variant))


def _split(V, n):
    """The n x n bilinear sub-quads of one quad (float64 in, each (4, 3))."""
    v00, v10, v11, v01 = V
    at = lambda a, b: (1 - a) * (1 - b) * v00 + a * (1 - b) * v10 + a * b * v11 + (1 - a) * b * v01
    g = np.linspace(0.0, 1.0, n + 1)
    return [np.array([at(g[i], g[j]), at(g[i + 1], g[j]), at(g[i + 1], g[j + 1]), at(g[i], g[j + 1])])
            for j in range(n) for i in range(n)]


@functools.lru_cache(maxsize=None)
def tess():
    """Cornell variant 2 with every wall split 8 x 8 and every box face 4 x 4
    (the light quad whole): shared edges and vertices, near and exact t ties.
    The box's points stay in front, so the light's ids are unchanged."""
    base = cornell(2)
    V = base.verts().astype(np.float64)
    area = np.linalg.norm(np.cross(V[:, 1] - V[:, 0], V[:, 3] - V[:, 0]), axis=1)
    pts, quads, mats, texs = [base.points], [], [], []
    n_pts = len(base.points)
    for q in range(len(base.quads)):
        if tuple(base.quads[q]) == base.light:
            quads.append(base.quads[q])
            mats.append(base.quad_mat[q]), texs.append(base.quad_tex[q])
            continue
        for sub in _split(V[q], 8 if area[q] > 0.5 * area.max() else 4):
            pts.append(sub.astype(F))
            quads.append(np.arange(n_pts, n_pts + 4))
            n_pts += 4
            mats.append(base.quad_mat[q]), texs.append(base.quad_tex[q])
    return Mesh(np.concatenate(pts), np.array(quads), mats, texs, base.spheres, base.mat_type, base.tex_type, base.tex,
                base.light, base.light_sphere_point, base.ior)


def _room(z):
    """The zoo's room without its floor (quad 2 is the light: points 8..11)."""
    z.add_quad([(1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)], GREEN)
    z.add_quad([(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)], RED)
    ly = 511 / 512
    z.add_quad([(0.375, ly, 0.375), (0.625, ly, 0.375), (0.625, ly, 0.625), (0.375, ly, 0.625)], LIGHT)
    z.add_quad([(0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)], WHITE)
    z.add_quad([(0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], WHITE)


def _terrain(z, nx, nz, amp=0.06, y0=0.0, rng=None):
    """A ridged floor over [0, 1]^2: nx x nz quads on shared vertices whose
    height varies along x only, so every quad is a planar parallelogram."""
    rng = rng or np.random.default_rng(11)
    hx = y0 + amp * (0.5 + 0.5 * np.sin(np.linspace(0, 9.0, nx + 1))) * rng.uniform(0.5, 1.0, nx + 1)
    xs, zs = np.linspace(0, 1, nx + 1), np.linspace(0, 1, nz + 1)
    X, Z = np.meshgrid(xs, zs, indexing="ij")
    base = z.add_points(np.stack([X, np.broadcast_to(hx[:, None], X.shape), Z], -1).reshape(-1, 3))
    i, j = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    a = base + i * (nz + 1) + j
    ids = np.stack([a, a + (nz + 1), a + (nz + 1) + 1, a + 1], -1).reshape(-1, 4)
    for k, q in enumerate(ids):
        z.quads.append([tuple(int(v) for v in q), *(WHITE if (k // nz + k % nz) % 2 else GREEN)])


@functools.lru_cache(maxsize=None)
def facets():
    """A room with a ridged floor, a tilted cone frustum of planar trapezoids
    in general orientation and a glass sphere: exactly 2048 quads."""
    z = _scenes.Zoo()
    _room(z)
    R = _scenes._rotation((1, 0.3, 0.2), 20.0)
    rings, seg = 3, 32
    ang = np.linspace(0, 2 * np.pi, seg + 1)[:-1]
    ring = lambda r, y: np.stack([r * np.cos(ang), np.full(seg, y), r * np.sin(ang)], -1) @ R.T + np.array([0.35, 0.2, 0.6])
    rows = [ring(0.18 - 0.04 * k, 0.12 * k) for k in range(rings + 1)]
    base = z.add_points(np.concatenate(rows))
    for k in range(rings):
        for s in range(seg):
            s1 = (s + 1) % seg
            z.quads.append([(base + k * seg + s, base + k * seg + s1, base + (k + 1) * seg + s1, base + (k + 1) * seg + s),
                            *(RED, WHITE, GREEN)[k % 3]])
    z.add_sphere((0.72, 0.3, 0.35), 0.15625, GLASS)
    z.light_sphere_point = z.spheres[0][0]
    extra = 2048 - len(z.quads) - 44 * 44
    assert 0 <= extra < 64
    for k in range(extra):  # planar steps against the back wall
        y = 0.3 + 0.02 * k
        z.add_quad(_scenes._rect((0.05 + 0.01 * k, y, 0.9), (0.1, 0, 0), (0, 0.01, 0.05)), WHITE)
    _terrain(z, 44, 44)
    assert len(z.quads) == 2048 and len(z.points) <= 8192
    return Mesh.from_zoo(z)


@functools.lru_cache(maxsize=None)
def bent():
    """The zoo's room plus 64 quads whose v11 is lifted off the first
    triangle's plane by 1% to 10% of the edge length."""
    z = _scenes.zoo()
    rng = np.random.default_rng(23)
    for k in range(64):
        o = np.array([0.08 + 0.11 * (k % 8), 0.3 + 0.05 * (k // 8 % 2), 0.08 + 0.11 * (k // 8)])
        e = 0.08
        a = _scenes._rotation(rng.normal(size=3), rng.uniform(0, 40)) @ np.array([e, 0, 0])
        b = _scenes._rotation(rng.normal(size=3), rng.uniform(0, 40)) @ np.array([0, 0, e])
        n = np.cross(a, b)
        lift = e * (0.01 + 0.09 * k / 63) * n / np.linalg.norm(n)
        z.add_quad([o, o + a, o + a + b + lift, o + b], (WHITE, RED, GREEN)[k % 3])
    # and 64 mildly bent ones, lifts of 0.02% to 0.10% of the edge: their fold stays under cos_min / 2, so they
    # keep a bounded box whose pad carries a real h / cos_min term (N_MILD, the scene's last quads)
    for k in range(N_MILD):
        o = np.array([0.06 + 0.11 * (k % 8), 0.62 + 0.03 * (k // 8 % 2), 0.06 + 0.11 * (k // 8)])
        e = 0.08
        Rk = _scenes._rotation(rng.normal(size=3), rng.uniform(0, 40))
        a, b = Rk @ np.array([e, 0, 0]), Rk @ np.array([0, 0, e])
        n = np.cross(a, b)
        lift = e * (0.0002 + 0.0008 * k / (N_MILD - 1)) * n / np.linalg.norm(n)
        z.add_quad([o, o + a, o + a + b + lift, o + b], (WHITE, RED, GREEN)[k % 3])
    return Mesh.from_zoo(z)


@functools.lru_cache(maxsize=None)
def grid(n):
    """A lit room over a planar-facet terrain of n quads (n a power of two)."""
    nx = 1 << ((n.bit_length() - 1) // 2)
    nz = n // nx
    assert nx * nz == n
    z = _scenes.Zoo()
    _room(z)
    z.add_sphere((0.6, 0.4, 0.5), 0.125, GLASS)
    z.light_sphere_point = z.spheres[0][0]
    _terrain(z, nx, nz)
    m = Mesh.from_zoo(z)
    assert len(m.quads) == n + 5
    return m


SCENES = {"tess": tess, "facets": facets, "bent": bent}


# ----------------------------------------------------------- populations --
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _ulps(x, k):
    """float32 array moved by k ulps (k int array, same shape)."""
    b = np.ascontiguousarray(x, dtype=F).view(np.int32).astype(np.int64)
    key = np.where(b < 0, -(b & 0x7FFFFFFF), b) + k  # ordered integers
    out = np.where(key < 0, (-key) | 0x80000000, key).astype(np.uint32)
    return out.view(F)


@functools.lru_cache(maxsize=None)
def rays(name, cos_min, pad, n=N_RAYS, seed=101):
    """(n, 6) float32 rays of scene `name` in eight equal parts (PART_NAMES).
    cos_min and pad (a typical box pad of the scene) shape the grazing part."""
    m = SCENES[name]() if isinstance(name, str) else grid(name)
    rng = np.random.default_rng(seed)
    V = m.verts().astype(np.float64)
    nq, p = len(V), n // N_PARTS
    lo, hi = m.bounds()
    diag, ctr = np.linalg.norm(hi - lo), 0.5 * (lo + hi)
    inside = lambda k: lo + (hi - lo) * rng.uniform(0.02, 0.98, size=(k, 3))
    on_quad = lambda q, a, b: ((1 - a) * (1 - b))[:, None] * V[q, 0] + (a * (1 - b))[:, None] * V[q, 1] + \
        (a * b)[:, None] * V[q, 2] + ((1 - a) * b)[:, None] * V[q, 3]
    normal = lambda q: np.cross(V[q, 1] - V[q, 0], V[q, 3] - V[q, 0])
    parts = []
    # 0: from inside the room at random
    parts.append(np.concatenate([inside(p), _unit(rng, p)], 1))
    # 1: aimed at quad vertices and edge midpoints, displaced by 0, +-1, +-16 ulps
    q, c = rng.integers(nq, size=p), rng.integers(4, size=p)
    tgt = np.where(rng.integers(2, size=p)[:, None] == 0, V[q, c], 0.5 * (V[q, c] + V[q, (c + 1) % 4]))
    o = inside(p).astype(F)
    d = (tgt.astype(F) - o).astype(F)
    d = _ulps(d, rng.choice([0, 1, -1, 16, -16], size=(p, 3)))
    parts.append(np.concatenate([o, d], 1))
    # 2: origins on quads (hit points: the t > 0.001 self-hit rule), cosine-distributed directions
    q = rng.integers(nq, size=p)
    o = on_quad(q, rng.uniform(0, 1, p), rng.uniform(0, 1, p))
    nrm = normal(q)
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True) * rng.choice([-1.0, 1.0], size=(p, 1))
    u = _unit(rng, p)
    tang = np.cross(nrm, u)
    tang /= np.linalg.norm(tang, axis=1, keepdims=True)
    r2, phi = rng.uniform(0, 1, p), rng.uniform(0, 2 * np.pi, p)
    d = (np.sqrt(r2) * np.cos(phi))[:, None] * tang + (np.sqrt(r2) * np.sin(phi))[:, None] * np.cross(nrm, tang) + \
        np.sqrt(1 - r2)[:, None] * nrm
    parts.append(np.concatenate([o, d], 1))
    # 3: meeting a chosen quad at |cos| in [1, 4] cos_min, aimed within one pad of its edges
    q, c = rng.integers(nq, size=p), rng.integers(4, size=p)
    edge_pt = V[q, c] + rng.uniform(0, 1, p)[:, None] * (V[q, (c + 1) % 4] - V[q, c])
    nrm = normal(q)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    inpl = np.cross(nrm, _unit(rng, p))
    inpl /= np.linalg.norm(inpl, axis=1, keepdims=True)
    inpl2 = np.cross(nrm, inpl)
    tgt = edge_pt + (rng.uniform(-1, 1, p) * pad)[:, None] * inpl2
    cs = cos_min * rng.uniform(1.0, 4.0, p) * rng.choice([-1.0, 1.0], size=p)
    d = np.sqrt(1 - cs * cs)[:, None] * inpl + cs[:, None] * nrm
    o = tgt - d * (diag * rng.uniform(0.05, 0.5, p))[:, None]
    parts.append(np.concatenate([o, d], 1))
    # 4: origins far out, aimed at the scene: 1 to 1.45 diagonals from its centre, so between 0.5 and 2 (just
    # under the reach) from whatever quad they hit
    o = ctr + _unit(rng, p) * (diag * rng.uniform(1.0, 1.45, p))[:, None]
    parts.append(np.concatenate([o, inside(p) - o], 1))
    # 5: axis-parallel rays (two zero direction components: the slab_rcp clamp) along axis-parallel quad edges,
    # so each lies in the planes of the quads that share the edge; through quad vertices where a scene has no
    # such edge
    E = V[:, [1, 2, 3, 0]] - V  # (nq, 4, 3): the edge leaving each corner, float32 values
    par = np.argwhere((E != 0).sum(2) == 1)
    d = np.zeros((p, 3))
    if len(par):
        pick = par[rng.integers(len(par), size=p)]
        q, c = pick[:, 0], pick[:, 1]
        ax = np.argmax(E[q, c] != 0, axis=1)
        base = V[q, c] + rng.uniform(0, 1, p)[:, None] * E[q, c]
    else:
        q, c, ax = rng.integers(nq, size=p), rng.integers(4, size=p), rng.integers(3, size=p)
        base = V[q, c]
    d[np.arange(p), ax] = rng.choice([-1.0, 1.0], size=p)
    o = base - d * (diag * rng.uniform(0.05, 0.4, p))[:, None]
    parts.append(np.concatenate([o, d], 1))
    # 6: rays that miss everything (from outside, pointing away)
    u = _unit(rng, p)
    parts.append(np.concatenate([ctr + u * diag * 1.2, u], 1))
    # 7: rays that start next to a sphere and go for its centre
    sp = [m.spheres[k] for k in rng.integers(len(m.spheres), size=p)]
    cen = np.array([m.points[s[0]] for s in sp], dtype=np.float64)
    rad = np.array([float(s[1]) for s in sp])
    u = _unit(rng, p)
    o = cen + u * (rad * rng.uniform(1.05, 1.5, p))[:, None]
    parts.append(np.concatenate([o, cen + 0.5 * rad[:, None] * _unit(rng, p) - o], 1))
    out = np.concatenate(parts).astype(F)
    assert out.shape == (n, 6)
    return out


# ------------------------------------------------------------ host builder --
NODE = np.dtype([("lo", F, 3), ("skip", np.int32), ("hi", F, 3), ("leaf", np.int32)])


def build_host(m, oct=0):
    """rtp_mesh_build_host: dict(nodes, order, boxes, pads, cos_min, reach)."""
    import raytracingtherestofyourlife_amd as rtp

    L, ptr = rtp.load(), rtp._lib.ptr
    desc, keep = m.desc()
    nq = len(m.quads)
    nodes = np.zeros(2 * nq, dtype=NODE)
    order = np.zeros(nq, dtype=np.int32)
    boxes = np.zeros((nq, 6), dtype=F)
    pads = np.zeros(nq, dtype=F)
    g = np.zeros(2, dtype=F)
    nn = ctypes.c_int32(0)
    rc = L.rtp_mesh_build_host(desc, oct, len(nodes), nn, nodes.ctypes.data, ptr(order), ptr(boxes), ptr(pads), ptr(g))
    assert rc == 0, L.rtp_last_error()
    del keep
    return dict(nodes=nodes[: nn.value], order=order, boxes=boxes, pads=pads, cos_min=float(g[0]), reach=float(g[1]))


# ------------------------------------------------------- host brute force --
def host_scan(m, ray, threads=8):
    """rtp_mesh_scan_host over the rays in parallel slices: (t bits uint32 [n],
    winner int32 [n], -1: no quad)."""
    import raytracingtherestofyourlife_amd as rtp
    fn, ptr = rtp.load().rtp_mesh_scan_host, rtp._lib.ptr
    desc, keep = m.desc()
    ray = np.ascontiguousarray(ray, dtype=F)
    out = np.zeros((len(ray), 2), dtype=np.uint32)
    cuts = np.linspace(0, len(ray), threads + 1).astype(int)

    def run(k):
        a, b = cuts[k], cuts[k + 1]
        return fn(desc, ptr(ray[a:b]), b - a, ptr(out[a:b]))

    with ThreadPoolExecutor(threads) as ex:
        assert all(rc == 0 for rc in ex.map(run, range(threads)))
    del keep
    return out[:, 0].copy(), out[:, 1].astype(np.int32)


def inside_promise(m, ray, winner, cos_min, reach):
    """Per ray, in float64: the winning quad (winner >= 0) is inside the
    promise -- every vertex within reach of the origin, and the ray meets the
    first triangle's plane with |cos| >= cos_min.  Rays without a winning quad
    are inside (nothing is promised about them that could fail)."""
    V = m.verts().astype(np.float64)
    r = np.asarray(ray, dtype=np.float64)
    o, d = r[:, :3], r[:, 3:]
    w = np.maximum(winner, 0)
    n = np.cross(V[w, 1] - V[w, 0], V[w, 3] - V[w, 0])
    with np.errstate(all="ignore"):
        cs = np.abs((n * d).sum(1)) / (np.linalg.norm(n, axis=1) * np.linalg.norm(d, axis=1))
    dist = np.linalg.norm(V[w] - o[:, None, :], axis=2).max(1)
    return (winner < 0) | ((cs >= cos_min) & (dist <= reach))
