"""Generated sphere sets for the sphere-BVH parity tests, their rays and their
references.  Built on _scenes.Zoo: a room of plain walls plus the light quad,
sphere 0 the light-sphere target.  Plain numpy (and the oracle's camera
constants): no GPU.

Everything the library computes is restated here from its definition, never
imported: the float32 sphere root (rtp_kernels.hip sphere_root, the oracle's
sphere_hit), the pad of a sphere's box (rtp_scene_host.cpp scene_sphere_bvh,
rtp_bvh_gpu.hip k_boxes; the pad before the soundness bound is kept as
pad_old for the guard that shows what that bound is for) and the outward
rounding to half precision (rtp_mesh_cell.hpp half_outward).

Walk orders.  Both builders keep spheres with equal keys in index order (the
host's stable partition and its sort by index, the device's stable radix sort
with ties split by position), so bit-identical spheres sit in ascending index
order in every tree; the octant copies of negative directions visit them in
descending order.  Rays of every octant therefore meet an exact tie both
ways round, and the groups' indices are spread so that other spheres lie
between them in index order."""
from __future__ import annotations

import numpy as np

import _scenes as S
from _scenes import F, GLASS, GREEN, LIGHT, RED, WHITE, Zoo

TMIN = F(0.001)
U = 2.0 ** -24          # float32 unit roundoff
REACH_FACTOR = 2.0      # the boxes' reach: this many diagonals of the scene's bounding box (include/rtp.h)
DISC_ERR = 24.0         # sphere_root's discriminant error bound, in units of 2^-24 |o-c|^2 |d|^2
GRAZE_ERR = 8.0         # the error the grazing rays are sized for (what float32 shows in practice)
LAMBERT = (RED, WHITE, GREEN)


# ------------------------------------------------------------------ rooms --
def room():
    """Five walls and the light quad (points 8..11) of the unit room, open
    toward the camera."""
    z = Zoo()
    z.add_quad([(1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)], GREEN)
    z.add_quad([(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)], RED)
    ly = 511 / 512
    z.add_quad([(0.375, ly, 0.375), (0.625, ly, 0.375), (0.625, ly, 0.625), (0.375, ly, 0.625)], LIGHT)
    z.add_quad([(0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)], WHITE)
    z.add_quad([(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)], WHITE)
    z.add_quad([(0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], WHITE)
    z.cams = [dict(z.cam), dict(S.HIGH_CAM)]
    return z


def _done(z, scale=1.0):
    z.light_sphere_point = z.spheres[0][0]
    if scale != 1.0:
        s = F(scale)
        z.scale = float(scale)
        z.points = (z.points * s).astype(F)
        for sp in z.spheres:
            sp[1] = F(sp[1] * s)
        for c in z.cams:
            c["position"] = (np.asarray(c["position"], F) * s).astype(F)
            c["look_at"] = (np.asarray(c["look_at"], F) * s).astype(F)
    z.cam = z.cams[0]
    return z


def _aim(z, target, fov0, fov1):
    """Both cameras turned to a small cloud at ``target``."""
    for c, fov in zip(z.cams, (fov0, fov1)):
        c["look_at"] = np.asarray(target, dtype=F)
        c["fov_y"] = float(F(fov))


def _mat(rng):
    return GLASS if rng.uniform() < 0.2 else LAMBERT[int(rng.integers(0, 3))]


def centres(z):
    return z.points[[s[0] for s in z.spheres]]


def radii(z):
    return np.array([s[1] for s in z.spheres], dtype=F)


# --------------------------------------------------------------- variants --
def uniform(n, seed, rlo=3.0, rhi=15.0):
    """Sphere 0 the glass sphere at (190, 90, 190) / 555 of radius 90 / 555;
    the rest uniformly inside the room, radius rlo..rhi (/555)."""
    z = room()
    rng = np.random.default_rng(seed)
    r = rng.uniform(rlo, rhi, n) / 555.0
    c = r[:, None] + (1 - 2 * r[:, None]) * rng.uniform(0, 1, (n, 3))
    z.add_sphere((190 / 555, 90 / 555, 190 / 555), 90 / 555, GLASS)
    for k in range(1, n):
        z.add_sphere(c[k], r[k], _mat(rng))
    return _done(z)


def count(n):
    """8: the scan; 9: the smallest BVH; 10; 300: more than the inline array
    of 256; 2000: near the oracle's limit of 2048.  (The few spheres of the
    small counts are large, so that the cameras see them.)"""
    return uniform(n, 100 + n, *((30.0, 70.0) if n <= 10 else (3.0, 15.0)))


def pad_old(c, r):
    """The pad of a sphere's box before the soundness bound, float32:
    0.002 r + 1e-5 + 2^-16 (max|c| + r)."""
    c, r = np.asarray(c, dtype=F), np.asarray(r, dtype=F)
    return ((F(0.002) * r + F(1e-5)) + F(2.0 ** -16) * (np.abs(c).max(axis=-1) + r)).astype(F)


def bounds(z):
    """The scene's bounding box, float32: every quad vertex, every sphere's
    c -+ r."""
    V = z.verts().reshape(-1, 3)
    c, r = centres(z), radii(z)
    lo = np.minimum(V.min(axis=0), (c - r[:, None]).min(axis=0)).astype(F)
    hi = np.maximum(V.max(axis=0), (c + r[:, None]).max(axis=0)).astype(F)
    return lo, hi


def reach(z):
    """The largest |o - c| the boxes are sound for: REACH_FACTOR diagonals of
    bounds(z), float32."""
    lo, hi = bounds(z)
    e = (hi - lo).astype(F)
    return F(REACH_FACTOR) * np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2], dtype=F)


def pad_new(z):
    """The pad with the soundness bound, per sphere, float32: pad_old +
    (sqrt(r^2 + E) - r) + 16 2^-24 reach, E = DISC_ERR 2^-24 reach^2."""
    return _pad_new(centres(z), radii(z), reach(z))


def _pad_new(c, r, rc):
    E = F(DISC_ERR * U) * rc * rc
    return ((pad_old(c, r) + (np.sqrt(r * r + E, dtype=F) - r)) + F(16 * U) * rc).astype(F)


def boxes(z, pad):
    """(lo, hi) float32 [n, 3] of the spheres' padded boxes."""
    c, r = centres(z), radii(z)
    pad = np.asarray(pad, dtype=F)
    return ((c - r[:, None]) - pad[:, None]).astype(F), ((c + r[:, None]) + pad[:, None]).astype(F)


def half_outward(x, up):
    """float32 -> the nearest half-precision value on the outer side (an
    infinity beyond the finite range), as float32."""
    x = np.asarray(x, dtype=F)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    v = h.astype(F)
    bad = (v < x) if up else (v > x)
    with np.errstate(over="ignore"):
        h = np.where(bad, np.nextafter(h, np.float16(np.inf if up else -np.inf)), h).astype(np.float16)
    return h.astype(F)


def _on_half_grid(c, r, axis, up, pad_of):
    """c with c[axis] moved (by less than 1e-3) so that the box face on that
    side lies within 2e-6 inside a half-precision grid point: rounding the
    face outward then adds next to nothing."""
    c = np.asarray(c, dtype=F).copy()
    bits = int(c[axis:axis + 1].view(np.int32)[0])
    cand = (bits + np.arange(-40000, 40001)).astype(np.int32).view(F)
    cs = np.repeat(c[None, :], cand.size, axis=0)
    cs[:, axis] = cand
    pad = pad_of(cs, F(r))
    face = ((cs[:, axis] + F(r)) + pad).astype(F) if up else ((cs[:, axis] - F(r)) - pad).astype(F)
    gap = np.abs(half_outward(face, up).astype(np.float64) - face.astype(np.float64))
    ok = np.flatnonzero((gap > 0) & (gap <= 2e-6))
    assert ok.size, "no such centre"
    c[axis] = cand[ok[np.abs(ok - 40000).argmin()]]
    return c


def extreme(new_pad=False):
    """64 spheres of radius 1/555 and 0.25/555 in a cube of side 0.03 about
    the room's centre.  Six of them are the cloud's extremes, one per axis
    and side (z.extreme: (index, axis, up)), each placed so that its box face
    on that side lies within 2e-6 inside a half-precision grid point; every
    other sphere lies strictly inside those six.  new_pad: placed for the pad
    with the soundness bound instead of the one before it."""
    rng = np.random.default_rng(7)
    n, mid, half = 64, 0.5, 0.015
    rad = np.where(np.arange(n) % 2 == 0, 1.0, 0.25) / 555.0
    rad[rng.permutation(n)[:8]] = 1.0 / 555.0
    c = mid + rng.uniform(-0.011, 0.011, (n, 3))
    where = [5, 17, 23, 38, 44, 59]
    sides = [(a, up) for a in range(3) for up in (False, True)]
    for k, (a, up) in zip(where, sides):
        c[k] = mid + rng.uniform(-0.008, 0.008, 3)
        c[k, a] = mid + (half if up else -half)

    def build(cc):
        z = room()
        for k in range(n):
            z.add_sphere(cc[k], rad[k], GLASS if k % 7 == 3 else LAMBERT[k % 3])
        return z

    c = c.astype(F)
    if new_pad:  # the pad depends on the scene's bounds: the room's here, whatever the cloud
        rc = reach(build(c))
        pad_of = lambda cs, r: _pad_new(cs, r, rc)
    else:
        pad_of = pad_old
    for k, (a, up) in zip(where, sides):
        c[k] = _on_half_grid(c[k], rad[k], a, up, pad_of)
    z = build(c)
    z.extreme = [(k, a, up) for k, (a, up) in zip(where, sides)]
    _aim(z, (mid, mid, mid), 1.2, 1.5)
    return _done(z)


def _spread(rng, n):
    """Centres in the room, clear of the walls by 0.12."""
    return 0.12 + 0.76 * rng.uniform(0, 1, (n, 3))


def duplicates():
    """40 spheres: 10 groups of 3 bit-identical ones (centre and radius; the
    materials differ, so a render shows which index won), 4 mirror pairs --
    equal spheres at x = m +- h with m, h dyadic, the lower index at the
    larger x: a ray in the plane x = m with d.x = +-0 meets both at the same
    float32 t (z.mirror: (lower index, higher index, m, y, z)) -- and two
    single ones, of which sphere 0 is the light-sphere target that nothing
    overlaps.  The other indices are dealt by a fixed permutation in which no
    group has two adjacent ones."""
    rng = np.random.default_rng(11)
    c0, r0 = np.array([0.2, 0.12, 0.2]), 0.1
    gr = rng.uniform(0.05, 0.09, 10)
    gc = []
    while len(gc) < 10:
        c = _spread(rng, 1)[0]
        if np.linalg.norm(c - c0) > r0 + gr[len(gc)] + 0.01:
            gc.append(c)
    items = []
    for g in range(10):
        for k in range(3):
            items.append((gc[g], gr[g], (RED, GREEN, GLASS)[(g + k) % 3] if k else WHITE))
    planes = [(0.25, 0.3, 0.75), (0.5, 0.7, 0.6), (0.75, 0.25, 0.3), (0.375, 0.8, 0.25)]
    for m, y, zz in planes:
        for k in range(2):  # k = 0 gets the lower index: the larger x
            items.append(((m + (0.0625 if k == 0 else -0.0625), y, zz), 0.078125, (WHITE, RED)[k]))
    items.append(((0.8, 0.6, 0.8), 0.07, GREEN))
    for _ in range(1000):
        perm = rng.permutation(39)
        at = lambda i: 1 + int(np.flatnonzero(perm == i)[0])  # the index of item i
        groups = [sorted(at(3 * g + k) for k in range(3)) for g in range(10)]
        mirror = [[at(30 + 2 * p + k) for k in range(2)] for p in range(4)]
        if all(b - a > 1 and c - b > 1 for a, b, c in groups) and all(lo < hi for lo, hi in mirror):
            break
    else:
        raise AssertionError("no such permutation")
    z = room()
    z.add_sphere(c0, r0, GLASS)
    for i in perm:  # index 1 + j holds item perm[j]
        z.add_sphere(*items[i])
    z.groups = groups
    z.mirror = [(lo, hi) + planes[p] for p, (lo, hi) in enumerate(mirror)]
    return _done(z)


def all_equal():
    """16 bit-identical spheres: zero extent on every axis, the median split
    by index, equal Morton codes; sphere 0 wins every hit."""
    z = room()
    for k in range(16):
        z.add_sphere((0.5, 0.35, 0.5), 0.3, (GLASS, WHITE, RED, GREEN)[k % 4])
    return _done(z)


def concentric():
    """16 spheres about one centre, radii 0.03..0.4 in no order."""
    z = room()
    rr = np.random.default_rng(13).permutation(np.linspace(0.03, 0.4, 16))
    for k in range(16):
        z.add_sphere((0.5, 0.45, 0.5), rr[k], GLASS if k % 2 else LAMBERT[k % 3])
    return _done(z)


def concentric9():
    """9 spheres (the smallest set behind the BVH) about one centre, radii
    increasing with the index: every Morton code is equal, so the device
    builder's radix tree splits by position alone."""
    z = room()
    for k, r in enumerate(np.linspace(0.05, 0.33, 9)):
        z.add_sphere((0.5, 0.45, 0.5), r, GLASS if k % 2 else LAMBERT[k % 3])
    return _done(z)


def near_ties():
    """32 pairs (k, k + 32) of equal-radius spheres whose centres differ by
    1e-5..1e-4 along one axis (z, toward the camera, for two pairs in three);
    the higher index is the nearer one (lower coordinate) for every other pair."""
    rng = np.random.default_rng(17)
    c, r = _spread(rng, 32), rng.uniform(0.03, 0.07, 32)
    z = room()
    second = []
    for k in range(32):
        delta = rng.uniform(1e-5, 1e-4) * (-1 if k % 2 else 1)
        e = np.zeros(3)
        e[2 if k % 3 else (k // 3) % 2] = delta
        second.append(c[k] + e)
    for k in range(32):
        z.add_sphere(c[k], r[k], GLASS if k % 5 == 0 else LAMBERT[k % 3])
    for k in range(32):
        z.add_sphere(second[k], r[k], LAMBERT[(k + 1) % 3])
    return _done(z)


def line():
    """24 spheres whose centres differ in x only (overlapping in chains)."""
    rng = np.random.default_rng(19)
    z = room()
    for x in rng.permutation(np.linspace(0.08, 0.92, 24)):
        z.add_sphere((x, 0.4, 0.5), rng.uniform(0.07, 0.12), _mat(rng))
    return _done(z)


def plane():
    """40 spheres with y constant."""
    rng = np.random.default_rng(23)
    z = room()
    for c in _spread(rng, 40):
        z.add_sphere((c[0], 0.3, c[2]), rng.uniform(0.04, 0.08), _mat(rng))
    return _done(z)


def cluster():
    """498 spheres of radius 0.2/555 inside a cube of side 2^-11 at the
    room's centre, and two spheres far from it (sphere 0, the glass sphere of
    uniform(), and one near the far top corner): the centres' bounding box is
    then about half the room, one 10-bit cell of it is about 2^-11 wide, and
    nearly all 30-bit Morton codes are equal."""
    rng = np.random.default_rng(29)
    z = room()
    z.add_sphere((190 / 555, 90 / 555, 190 / 555), 90 / 555, GLASS)
    z.add_sphere((0.85, 0.85, 0.8), 0.05, WHITE)
    for c in 0.5 + rng.uniform(0, 2.0 ** -11, (498, 3)):
        z.add_sphere(c, 0.2 / 555, _mat(rng))
    m = 0.5 + 2.0 ** -12
    _aim(z, (m, m, m), 0.053, 0.066)
    return _done(z)


def nested():
    """A glass sphere of radius 0.6 about the room's centre around the whole
    cloud (ray origins in the room are inside it), two chains of overlapping
    spheres, and a glass sphere around the default camera's position."""
    rng = np.random.default_rng(31)
    z = room()
    z.add_sphere((0.35, 0.2, 0.4), 0.1, GLASS)
    for k in range(12):  # each overlaps the next
        a = k / 11
        z.add_sphere((0.15 + 0.7 * a, 0.55 + 0.2 * np.sin(5 * a), 0.7 - 0.3 * a), 0.065, _mat(rng))
    z.add_sphere((0.5, 0.5, 0.5), 0.6, GLASS)
    for k in range(10):
        a = k / 9
        z.add_sphere((0.75 - 0.4 * a, 0.2 + 0.1 * a, 0.25 + 0.5 * a), 0.045, _mat(rng))
    z.add_sphere(np.asarray(z.cam["position"], dtype=np.float64) + (0.02, 0.01, 0.03), 0.1, GLASS)
    return _done(z)


FAR = [(-70500.0, 300.0, -2000.0), (72000.0, 200.0, -3000.0), (-81000.0, 250.0, -2500.0)]


def far(beyond_half=False):
    """The room and a cloud of 64 spheres in the reference's units (times
    555).  beyond_half: three more spheres centred beyond +-70000 in x, out of
    half precision's finite range, behind the camera and beside every ray's
    way: they only shape the boxes."""
    z = uniform(64, 37, 10.0, 40.0)
    z = _done(z, 555.0)
    if beyond_half:
        for c in FAR:
            z.add_sphere(c, 20.0, WHITE)
    return z


VARIANTS = {
    "count8": lambda: count(8),
    "count9": lambda: count(9),
    "count10": lambda: count(10),
    "count300": lambda: count(300),
    "count2000": lambda: count(2000),
    "extreme": extreme,
    "extreme_new_pad": lambda: extreme(True),
    "duplicates": duplicates,
    "all_equal": all_equal,
    "concentric": concentric,
    "concentric9": concentric9,
    "near_ties": near_ties,
    "line": line,
    "plane": plane,
    "cluster": cluster,
    "nested": nested,
    "far": far,
    "far_beyond_half": lambda: far(True),
}

_variants = {}


def variant(name):
    """VARIANTS[name](), built once."""
    if name not in _variants:
        _variants[name] = VARIANTS[name]()
    return _variants[name]


def parked(z):
    """The same quads with exactly one sphere, far below the floor where no
    test ray reaches it: closest hits on it are the quads' part of z's, on the
    scan path."""
    p = Zoo()
    p.points, p.quads, p.light, p.ior, p.scale = z.points.copy(), [list(q) for q in z.quads], z.light, z.ior, z.scale
    p.add_sphere((0.5 * z.scale, -1000.0 * z.scale, 0.5 * z.scale), 0.001 * z.scale, WHITE)
    p.light_sphere_point = p.spheres[0][0]
    return p


# ------------------------------------------------------------------- rays --
def _pack(o, d):
    """Built in float64, rounded once."""
    return np.concatenate([np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)], axis=1).astype(F)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _camera_rays(z, n):
    import oracle_ctypes

    nx = max(int(np.sqrt(n / 2)), 1)
    out = []
    for c in z.cams:
        o, d = S.pixel_centre_rays(oracle_ctypes.camera_setup(nx, nx, **c), nx, nx)
        out.append(_pack(o, d))
    return np.concatenate(out)


def _inside_rays(z, n, rng):
    return _pack(rng.uniform(0, 1, (n, 3)) * z.scale, _unit(rng.normal(size=(n, 3))))


def _close_rays(z, n, rng):
    """From 1.5 to 25 radii off a sphere's centre toward it: the only rays
    for which a small sphere is more than a silhouette."""
    c, r = centres(z).astype(np.float64), radii(z).astype(np.float64)
    k = rng.integers(0, len(r), n)
    o = c[k] + _unit(rng.normal(size=(n, 3))) * (r[k] * rng.uniform(1.5, 25.0, n))[:, None]
    return _pack(o, _unit((c[k] + r[k, None] * rng.uniform(-1.5, 1.5, (n, 3))) - o))


def _axis_rays(z, n, rng):
    """One or two direction components exactly +0.0 or -0.0, aimed at a
    sphere; every other ray starts exactly on a coordinate that is a face of
    that sphere's box (the float32 face, or that face rounded outward to half
    precision), and every other one of those travels in that face's plane."""
    c, r = centres(z).astype(np.float64), radii(z).astype(np.float64)
    lo, hi = boxes(z, pad_new(z))
    k = rng.integers(0, len(r), n)
    o = rng.uniform(0, 1, (n, 3)) * z.scale
    a = rng.integers(0, 3, n)
    up = rng.uniform(size=n) < 0.5
    face = np.where(up, hi[k, a], lo[k, a])
    face = np.where(rng.uniform(size=n) < 0.5, face, np.where(up, half_outward(face, True), half_outward(face, False)))
    on = np.arange(n) % 2 == 0
    rows = np.arange(n)
    o[rows[on], a[on]] = face[on].astype(np.float64)
    d = (c[k] + r[k, None] * rng.uniform(-1.2, 1.2, (n, 3))) - np.where(np.isfinite(o), o, 0.0)
    zero = np.where(on & (np.arange(n) % 4 == 0), a, rng.integers(0, 3, n))
    d[rows, zero] = 0.0
    two = rng.uniform(size=n) < 0.3
    d[rows[two], (zero[two] + 1) % 3] = 0.0
    norm = np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where(norm > 0, d / np.where(norm > 0, norm, 1.0), d)
    neg = rng.uniform(size=(n, 3)) < 0.5
    d = np.where((d == 0) & neg, -0.0, d)
    o = np.where(np.isfinite(o), o, 0.5 * z.scale)  # (a face at an infinity)
    return _pack(o, d)


def graze_band(r, D):
    """How far beyond r float32 can still accept a ray from distance D, for
    a discriminant error of GRAZE_ERR 2^-24 D^2."""
    return np.sqrt(r * r + GRAZE_ERR * U * D * D) - r


def _graze_rays(z, n, rng):
    """Rays passing a sphere at r + u from its centre, u in [-1e-5,
    graze_band(r, D) + 1e-5], from distance D in [0.5 (scene units), reach],
    travelling in the plane of the box side they pass (that direction
    component is +-0): past the cloud's six extremes on their outer sides
    where the variant has them (z.extreme), past random spheres otherwise."""
    c, r = centres(z).astype(np.float64), radii(z).astype(np.float64)
    if hasattr(z, "extreme"):
        pick = rng.integers(0, len(z.extreme), n)
        k = np.array([e[0] for e in z.extreme])[pick]
        a = np.array([e[1] for e in z.extreme])[pick]
        sgn = np.where(np.array([e[2] for e in z.extreme])[pick], 1.0, -1.0)
    else:
        k, a, sgn = rng.integers(0, len(r), n), rng.integers(0, 3, n), np.where(rng.uniform(size=n) < 0.5, 1.0, -1.0)
    D = rng.uniform(0.5 * z.scale, float(reach(z)), n)
    u = rng.uniform(-1e-5 * z.scale, graze_band(r[k], D) + 1e-5 * z.scale)
    phi = rng.uniform(0, 2 * np.pi, n)
    rows = np.arange(n)
    o, d = c[k].copy(), np.zeros((n, 3))
    o[rows, a] += sgn * (r[k] + u)
    o[rows, (a + 1) % 3] += D * np.cos(phi)
    o[rows, (a + 2) % 3] += D * np.sin(phi)
    d[rows, (a + 1) % 3] = -np.cos(phi)
    d[rows, (a + 2) % 3] = -np.sin(phi)
    d[rows, a] = np.where(rng.uniform(size=n) < 0.5, 0.0, -0.0)
    return _pack(o, d)


def _mirror_rays(z, n, rng):
    """In the mirror plane of a pair (z.mirror), d.x = +-0, toward the
    lens the two spheres share."""
    if not hasattr(z, "mirror"):
        return np.zeros((0, 6), dtype=F)
    p = rng.integers(0, len(z.mirror), n)
    m = np.array([e[2:5] for e in z.mirror])[p]
    o = rng.uniform(0, 1, (n, 3))
    o[:, 0] = m[:, 0]
    d = (m + 0.03 * rng.uniform(-1, 1, (n, 3))) - o
    d[:, 0] = np.where(rng.uniform(size=n) < 0.5, 0.0, -0.0)
    nrm = np.linalg.norm(d, axis=1, keepdims=True)
    return _pack(o, np.where(d == 0, d, d / nrm))


def _nan_rays(z, n, rng):
    r = _inside_rays(z, n, rng)
    bad = [np.nan, np.inf, -np.inf]
    for i in range(n):
        r[i, (i * 5) % 6] = bad[i % 3]
    return r


_KINDS = {"inside": _inside_rays, "close": _close_rays, "axis": _axis_rays, "graze": _graze_rays,
          "mirror": _mirror_rays, "nan": _nan_rays}
KINDS = ("camera", "inside", "close", "axis", "graze", "mirror", "nan")


def rays(z, kind, n, seed):
    """(about n, 6) float32 rays (o, d) of one kind for a variant."""
    if kind == "camera":
        return _camera_rays(z, n)
    return _KINDS[kind](z, n, np.random.default_rng([seed, KINDS.index(kind)]))


def ray_sets(z, seed=1):
    """{kind: rays}: the sets the ray-level tests take, sized so that
    spheres x rays stays near 2^24 (at most 2^14 rays, at least 2^13)."""
    n = int(np.clip((1 << 24) // max(len(z.spheres), 1), 1 << 13, 1 << 14))
    sizes = {"camera": n // 4, "inside": n // 4, "close": n // 4, "axis": n // 4, "graze": n // 2, "mirror": n // 8,
             "nan": 24}
    return {k: rays(z, k, sizes[k], seed) for k in KINDS}


# ------------------------------------------------------------- references --
def sphere_roots_f32(z, o, d, first=0, last=None):
    """sphere_root in float32, operation by operation, for spheres
    first..last: t [sphere, ray], inf where not accepted.  dot(x, y) =
    (x0 y0 + x1 y1) + x2 y2; disc = b b - a cc; correctly rounded sqrt and
    divisions; r1 > tmin ? r1 : r2, accepted if > tmin."""
    o, d = np.ascontiguousarray(o, dtype=F), np.ascontiguousarray(d, dtype=F)
    c = centres(z)[first:last]
    rad = radii(z)[first:last]
    rr = (rad * rad).astype(F)[:, None]
    with np.errstate(all="ignore"):
        ocx, ocy, ocz = (o[None, :, k] - c[:, None, k] for k in range(3))
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        a = (dx * dx + dy * dy) + dz * dz
        b = (ocx * dx + ocy * dy) + ocz * dz
        cc = ((ocx * ocx + ocy * ocy) + ocz * ocz) - rr
        disc = b * b - a * cc
        sq = np.sqrt(disc)
        r1 = (-b - sq) / a
        t = np.where(r1 > TMIN, r1, (-b + sq) / a)
        ok = (disc > 0) & (t > TMIN)
    assert t.dtype == F
    return np.where(ok, t, F(np.inf))


def sphere_hits_f32(z, o, d, chunk=32):
    """The brute-force scan over sphere_roots_f32 in index order with a
    strict '<': (t float32 [ray], index [ray]); inf and -1 where no sphere is
    hit.  No tree in it."""
    n = len(o)
    best_t, best_i = np.full(n, np.inf, dtype=F), np.full(n, -1, dtype=np.int64)
    cols = np.arange(n)
    for s0 in range(0, len(z.spheres), chunk):
        t = sphere_roots_f32(z, o, d, s0, s0 + chunk)
        k = t.argmin(axis=0)  # the first of equal minima
        tk = t[k, cols]
        upd = tk < best_t
        best_t[upd], best_i[upd] = tk[upd], s0 + k[upd]
    return best_t, best_i


def expected_hits(quad_cols, t_s, i_s):
    """The combined closest hit as three uint32 words (t bits, kind, index):
    the sphere's if and only if its t is strictly less than the quads' t (a
    miss carries the largest float), else the quads' words as they are."""
    quad_cols = np.asarray(quad_cols, dtype=np.uint32)
    tq = quad_cols[:, 0].copy().view(F)
    take = t_s < tq
    sph = np.stack([t_s.view(np.uint32), np.ones_like(i_s, dtype=np.uint32), i_s.astype(np.uint32)], axis=1)
    return np.where(take[:, None], sph, quad_cols)


def same_hits(got, want):
    """Rows equal word for word, or both t NaN."""
    got, want = np.asarray(got, dtype=np.uint32), np.asarray(want, dtype=np.uint32)
    both_nan = np.isnan(got[:, 0].copy().view(F)) & np.isnan(want[:, 0].copy().view(F))
    return (got == want).all(axis=1) | both_nan


def slab_misses(lo, hi, o, d):
    """Exact (float64) slab test of rays against one box each: True where the
    line misses the box or the box lies wholly behind the origin."""
    lo, hi, o, d = (np.asarray(v, dtype=np.float64) for v in (lo, hi, o, d))
    with np.errstate(all="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    par = d == 0
    inside = (lo <= o) & (o <= hi)
    tn = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1)).max(axis=1)
    tf = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t0, t1)).min(axis=1)
    return (tn > tf) | (tf < 0)
