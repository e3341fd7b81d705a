"""Cases, word layouts and file formats of the reference stage fixture
(tests/golden/ref_stages.npz), shared by tools/make_ref_stage_golden.py, which
records what the reference's own worklet headers compute (oracle/_ref/ref_stages,
built from tests/cpp/ref_stage_driver.cpp), and by the tests that hold the oracle
and the HIP bounce to those records.

Cases are rows of 32-bit words.  They are generated here from fixed seeds, with
numpy's frozen RandomState streams and float32 arithmetic of exactly rounded
operations only, so that the tool and the tests build the same rows; the
fixture stores a digest of every case array, and the cases that can only be
found by running the reference (the dielectric's reflect_prob thresholds)."""
from __future__ import annotations

import hashlib
import os
import subprocess
import tempfile

import numpy as np

F = np.float32
U = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_STAGES = os.path.join(ROOT, "oracle", "_ref", "ref_stages")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_stages.npz")
MAGIC = 0x47545352
N_STAGE = 2048
N_BOUNCE = 4096
FLT_MAX = np.finfo(F).max

# name: (driver mode, words per case, result word types, oracle entry takes the scene)
# result word types: f float32 bits (NaN equals NaN), i int32, u uint32
STAGES = {
    "rng": (0, 1, "ufu", False),                            # wang32(seed); getRandF(seed), seed after
    "which": (1, 1, "iu", False),                           # which, seed after
    "onb": (2, 6, "f" * 12, False),                         # n, a -> u, v, w, local(a)
    "quad_hit": (3, 20, "ifffi" + "f" * 7, False),          # o, d, v00, v10, v11, v01, tmin, tmax -> hit, u, v, t; intersect, T, N, P
    "sphere_hit": (4, 12, "i" + "f" * 7, False),            # o, d, centre, radius, tmin, tmax -> hit, T, N, P
    "material": (5, 20, "u" + "f" * 12 + "u", True),        # kind, fin, o, d, hrec[9], hid M, T, seed -> fin, srec[9], emitted, seed
    "dielectric_scatter": (6, 12, "f" * 9, False),          # d, n, p, _rand (double: lo, hi), ref_idx -> srec[9]
    "generator": (7, 9, "fffu", True),                      # kind, which, n, p, seed -> generated, seed
    "light_pdf": (8, 10, "fu", True),                       # kind, fin, p, generated, sum_value, seed -> sum_value, seed
    "scatter": (9, 26, "u" + "f" * 9, True),                # fin, o, d, n, p, srec[9], sum_value, generated -> fin, o, d, attenuation
    "collect": (10, 1, "u" + "f" * 6, True),                # status -> status, emitted, attenuation (7: left alone)
}
BOUNCE_MODE = 11
PASSES = ("quad traversal", "sphere traversal", "CollectIntersecttWorklet", "LambertianWorklet", "DiffuseLightWorklet",
          "DielectricWorklet", "WorketletGenerateDir", "CosineWorketletGenerateDir", "QuadWorkletGenerateDir",
          "SphereWorkletGenerateDir", "QuadPDFWorklet", "SpherePDFWorklet", "PDFCosineWorklet")
# one ray's state after a pass (rtp_oracle.h rtpo_bounce): word offsets
REC_TYPES = "u" + "f" * 7 + "ii" + "f" * 9 + "i" + "f" * 16 + "u"
REC = dict(status=0, T=1, N=2, P=5, M=8, Tx=9, sO=10, sD=13, sA=16, which=19, gen=20, sum=23, E=24, A=27, org=30, dir=33,
           seed=36)
REC_WORDS = len(REC_TYPES)
BOUNCE_SCENES = ("cornell0", "cornell1", "cornell2", "cornell3", "zoo")
STAGE_SCENE = "cornell1"  # the scene of the stages that take one: the glass sphere inside the box
# the least number of cases the fixture must hold of every outcome (counted from the reference's results)
MIN_COVER = 32


def fbits(a):
    return np.ascontiguousarray(a, dtype=F).view(U)


def words(*cols):
    """Stack columns (float arrays of shape (n,) or (n, k) as float32 bits, integer arrays as they are) into rows
    of 32-bit words."""
    out = []
    for c in cols:
        c = np.asarray(c)
        c = fbits(c.astype(F)) if c.dtype.kind == "f" else (c.astype(np.int64) & 0xFFFFFFFF).astype(U)
        out.append(c.reshape(len(c), -1))
    return np.ascontiguousarray(np.concatenate(out, 1))


def canonical(out, types):
    """Results with every NaN of a float column written as 0x7fc00000 (the payload carries no information)."""
    out = np.array(out, dtype=U, copy=True).reshape(-1, len(types))
    fcols = np.array([t == "f" for t in types])
    f = out.view(F)
    nan = np.isnan(f) & fcols[None, :]
    out[nan] = 0x7FC00000
    return out


def digest(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<u4").tobytes()).hexdigest()


def row_hashes(a) -> np.ndarray:
    """One 64-bit hash per row of canonical words."""
    a = np.ascontiguousarray(a, dtype="<u4")
    return np.array([int.from_bytes(hashlib.blake2b(r.tobytes(), digest_size=8).digest(), "little") for r in a],
                    dtype=np.uint64)


# ------------------------------------------------------------------ scenes --
def scenes(oracle) -> dict:
    import _scenes

    sc = {f"cornell{v}": oracle.cornell_box(v) for v in range(4)}
    sc["zoo"] = _scenes.zoo().scene(oracle)
    return sc


def scene_words(sc) -> np.ndarray:
    """The scene section of a case file (ref_stage_driver.cpp Scene::read)."""
    arr = np.ctypeslib.as_array
    nq, ns = sc.n_quads, sc.n_spheres
    i32 = lambda a: np.asarray(a, dtype=np.int32).reshape(-1).view(U)
    f32 = lambda a: fbits(np.asarray(a, dtype=F).reshape(-1))
    parts = [i32([sc.n_points]), f32(arr(sc.points)[: sc.n_points]), i32([nq]), i32(arr(sc.quad_ids)[:nq]),
             i32(arr(sc.quad_mat)[:nq]), i32(arr(sc.quad_tex)[:nq]), i32([ns]), i32(arr(sc.sphere_point)[:ns]),
             f32(arr(sc.sphere_radius)[:ns]), i32(arr(sc.sphere_mat)[:ns]), i32(arr(sc.sphere_tex)[:ns]),
             i32([sc.n_mat]), i32(arr(sc.mat_type)[: sc.n_mat]), i32([sc.n_tex_type]),
             i32(arr(sc.tex_type)[: sc.n_tex_type]), i32([sc.n_tex]), f32(arr(sc.tex)[: sc.n_tex]),
             i32(list(sc.light_box_pointids)), i32([sc.light_sphere_point]), f32([sc.ior])]
    return np.concatenate(parts)


def scene_verts(sc) -> np.ndarray:
    """(nq, 4, 3) float32: v00, v10, v11, v01 of every quad."""
    return sc.points_np()[sc.quad_ids_np()[:, 1:]]


# ----------------------------------------------------------- running things --
def run_driver(mode: int, kout: int, sc, cases: np.ndarray, exe: str = REF_STAGES) -> np.ndarray:
    """The reference's results for the cases: (n, kout) words."""
    cases = np.ascontiguousarray(cases, dtype=U)
    n, kin = cases.shape
    with tempfile.TemporaryDirectory() as td:
        fin, fout = os.path.join(td, "cases.bin"), os.path.join(td, "results.bin")
        with open(fin, "wb") as fh:
            np.array([MAGIC, mode, n, kin], dtype=U).tofile(fh)
            scene_words(sc).tofile(fh)
            cases.tofile(fh)
        subprocess.run([exe, fin, fout], check=True)
        res = np.fromfile(fout, dtype=U)
    assert res[:3].tolist() == [mode, n, kout], res[:3]
    return res[3:].reshape(n, kout)


def driver_stage(name: str, sc, cases, exe: str = REF_STAGES) -> np.ndarray:
    mode, kin, types, _ = STAGES[name]
    assert cases.shape[1] == kin
    return run_driver(mode, len(types), sc, cases, exe)


def driver_bounce(sc, rays, seeds, exe: str = REF_STAGES) -> np.ndarray:
    """(n, 13, 37) words: every ray's state after every worklet of one depth."""
    out = run_driver(BOUNCE_MODE, len(PASSES) * REC_WORDS, sc, words(rays, seeds), exe)
    return out.reshape(len(rays), len(PASSES), REC_WORDS)


# ------------------------------------------------------------ case helpers --
def _rs(tag: str) -> np.random.RandomState:
    return np.random.RandomState(int.from_bytes(hashlib.sha256(tag.encode()).digest()[:4], "little"))


def _uni(rs, lo, hi, shape):
    return (lo + (hi - lo) * rs.random_sample(shape)).astype(F)


def _dirs(rs, n):
    """Directions from the cube (never all zero), lengths 0.05 .. 0.87."""
    d = _uni(rs, -0.5, 0.5, (n, 3))
    d[(np.abs(d) < 0.05).all(1)] = F(0.25)
    return d


def _pow10(e):
    """10**e for integer e in -3 .. 3, from a table (no libm pow)."""
    return np.array([1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3])[np.asarray(e) + 3]


def _pick(rs, n, k):
    return rs.randint(0, k, n)


def _nudge(a, ulps):
    """a moved by `ulps` float32 steps along the number line (0.0 minus one step is the smallest negative number)."""
    i = np.ascontiguousarray(a, dtype=F).view(np.int32).astype(np.int64)
    key = np.where(i >= 0, i, -(i & 0x7FFFFFFF)) + np.asarray(ulps, dtype=np.int64)
    return np.where(key >= 0, key, (-key) | 0x80000000).astype(U).view(F)


def inv_wang32(t):
    """The seed whose hash is t (wangXor.h:30-38 is a bijection of uint32)."""
    x = np.asarray(t, dtype=np.uint64) & 0xFFFFFFFF
    x = x ^ (x >> 15) ^ (x >> 30)
    x = (x * pow(0x27D4EB2D, -1, 1 << 32)) & 0xFFFFFFFF
    x = x ^ (x >> 4) ^ (x >> 8) ^ (x >> 12) ^ (x >> 16) ^ (x >> 20) ^ (x >> 24) ^ (x >> 28)
    x = (x * pow(9, -1, 1 << 32)) & 0xFFFFFFFF
    hi = x >> 16
    return ((hi << 16) | ((x & 0xFFFF) ^ 61 ^ hi)).astype(U)


def which_thresholds():
    import json

    with open(os.path.join(ROOT, "tests", "golden", "kat.json")) as fh:
        return json.load(fh)["which_thresholds"]


def seeds_cases() -> np.ndarray:
    """RNG and which: seeds 0 and 2^32-1, hashes 0 and the lowest and highest that draw 1.0f, hashes around the
    `which` thresholds of kat.json and around the draw's rounding steps, and random seeds."""
    rs = _rs("seeds")
    th = which_thresholds()
    near = np.concatenate([np.arange(t - 160, t + 161, 1, dtype=np.int64) for t in th])
    ones = np.concatenate([np.arange(4294967168 - 40, 4294967168 + 40, dtype=np.int64),
                           np.arange((1 << 32) - 40, 1 << 32, dtype=np.int64), np.arange(0, 40, dtype=np.int64)])
    special = np.concatenate([np.array([0, 0xFFFFFFFF, 61, 1, 639999, 1 << 31], dtype=U), inv_wang32(near),
                              inv_wang32(ones)])
    rnd = rs.randint(0, 1 << 32, N_STAGE - len(special), dtype=np.uint64).astype(U)
    return np.concatenate([special, rnd]).reshape(-1, 1)


def onb_cases() -> np.ndarray:
    rs = _rs("onb")
    n = N_STAGE
    nn = _dirs(rs, n)
    k = n // 8
    ax = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=F)
    nn[:k] = ax[_pick(rs, k, 6)] * _uni(rs, 0.5, 2.0, (k, 1))
    # |w.x| either side of build_from_w's 0.9
    x = _nudge(np.full(k, 0.9, dtype=F), rs.randint(-3, 4, k)) * np.where(rs.random_sample(k) < 0.5, -1, 1).astype(F)
    y = _uni(rs, -1, 1, k)
    y = np.sqrt(np.maximum(F(1) - x * x, F(0))).astype(F) * np.where(y < 0, -1, 1).astype(F)
    nn[k:2 * k] = np.stack([x, y, np.zeros(k, dtype=F)], 1)
    nn[2 * k:2 * k + 8] = 0  # a zero normal: what a dead ray's generator is given
    a = _uni(rs, -2, 2, (n, 3))
    return words(nn, a)


def synthetic_quads(degenerate: bool = True) -> np.ndarray:
    """Quads for the bilinear branches of QuadLeafIntersector::hit (Surface.h:106-158) in each of the three
    normal-dominant orientations and one tilted, all dyadic: v11 = v00 + a e01 + b e03.  The reference takes
    n = Cross(E01, E02), so beta_11 = n_i / n_i is 1 for every quad with a triangle normal: (a, b) = (1, 1) gives
    alpha_11 = 1 (first branch), (1, 1.25), (1.25, 1) and (1.25, 0.75) give alpha_11 != 1 (second branch).  The
    third branch is reached only where n = 0 (v00, v10, v11 on one line: alpha_11 infinite, beta_11 = 0/0), the
    `degenerate` quads (a, b) = (0.5, 0), which come last."""
    out = []
    frames = [((0.25, 0.25, 0.5), (0.5, 0, 0), (0, 0.5, 0)), ((0.5, 0.25, 0.25), (0, 0.5, 0), (0, 0, 0.5)),
              ((0.25, 0.5, 0.25), (0, 0, 0.5), (0.5, 0, 0)), ((0.25, 0.25, 0.25), (0.5, 0.125, 0.0625), (-0.0625, 0.25, 0.5))]
    for ab in (((1, 1), (1, 1.25), (1.25, 1), (1.25, 0.75)), ((0.5, 0.0),) if degenerate else ()):
        for o, e1, e3 in frames:
            o, e1, e3 = (np.array(v, dtype=np.float64) for v in (o, e1, e3))
            for a, b in ab:
                out.append([o, o + e1, o + a * e1 + b * e3, o + e3])
    return np.array(out, dtype=F)


def quad_pool(scs, degenerate: bool = True) -> np.ndarray:
    return np.concatenate([scene_verts(scs["zoo"]), scene_verts(scs["cornell0"]), synthetic_quads(degenerate)], 0)


def quad_hit_cases(scs) -> np.ndarray:
    rs = _rs("quad_hit")
    V = quad_pool(scs)
    n, k = N_STAGE, N_STAGE // 8
    q = np.arange(n) % len(V)  # every quad of the pool, in turn
    q[7 * k:] = len(V) - 1 - np.arange(n - 7 * k) % 4  # and the degenerate ones again
    v00, v10, v11, v01 = (V[q, j] for j in range(4))
    e1, e3 = v10 - v00, v01 - v00
    nrm = np.cross(e1.astype(np.float64), e3.astype(np.float64))
    nrm = (nrm / np.sqrt((nrm * nrm).sum(1, keepdims=True))).astype(F)
    u, v = _uni(rs, -0.1, 1.1, n), _uni(rs, -0.1, 1.1, n)
    o = _uni(rs, -0.2, 1.2, (n, 3))
    tmin = np.full(n, F(0.001))
    tmax = np.full(n, FLT_MAX)
    # 1. through a vertex or a point of an edge, exactly and a few ulps off
    s = slice(k, 2 * k)
    e = _pick(rs, k, 4)
    a, b = V[q[s], e], V[q[s], (e + 1) % 4]
    w = _uni(rs, 0, 1, k)
    w[rs.random_sample(k) < 0.4] = 0
    tgt_edge = _nudge(a + w[:, None] * (b - a), rs.randint(-2, 3, (k, 3)))
    tgt = (v00 + u[:, None] * e1 + v[:, None] * e3).astype(F)
    tgt[s] = tgt_edge
    d = (tgt - o).astype(F)
    # 2. in the quad's plane: origin on the plane, direction a combination of the edges
    s = slice(2 * k, 3 * k)
    o[s] = (v00[s] + _uni(rs, -0.5, 1.5, (k, 1)) * e1[s] + _uni(rs, -0.5, 1.5, (k, 1)) * e3[s]).astype(F)
    d[s] = (_uni(rs, -1, 1, (k, 1)) * e1[s] + _uni(rs, -1, 1, (k, 1)) * e3[s]).astype(F)
    # 3. nearly in the plane: det = -d . (e01 x e03) either side of Epsilon = 1e-5
    s = slice(3 * k, 4 * k)
    cr = np.cross(e1[s].astype(np.float64), e3[s].astype(np.float64))
    inpl = (_uni(rs, -1, 1, (k, 1)) * e1[s] + _uni(rs, -1, 1, (k, 1)) * e3[s]).astype(np.float64)
    want = 1e-5 * (0.5 + 1.0 * rs.random_sample(k)) * np.where(rs.random_sample(k) < 0.5, -1, 1)
    lift = want / (cr * nrm[s]).sum(1)
    o[s] = (tgt[s] - (inpl - lift[:, None] * nrm[s])).astype(F)
    d[s] = (tgt[s] - o[s]).astype(F)
    # 4. t either side of tmin: the origin 0.0005 .. 0.0015 in front of the hit point along a unit-length d
    s = slice(4 * k, 5 * k)
    dd = _dirs(rs, k).astype(np.float64)
    dd /= np.sqrt((dd * dd).sum(1, keepdims=True))
    o[s] = (tgt[s] - dd * (0.0005 + 0.001 * rs.random_sample((k, 1)))).astype(F)
    d[s] = dd.astype(F)
    # 5. t either side of a tmax left by an earlier hit: tmax = t (in double, rounded) nudged by -2 .. 2 ulps
    s = slice(5 * k, 6 * k)
    t64 = ((tgt[s] - o[s]).astype(np.float64) * d[s]).sum(1) / (d[s].astype(np.float64) ** 2).sum(1)
    tmax[s] = _nudge(t64.astype(F), rs.randint(-2, 3, k))
    # 6. unnormalised and reversed directions (t < 0)
    s = slice(6 * k, 7 * k)
    d[s] = (d[s] * _pow10(rs.randint(-3, 4, (k, 1))).astype(F) * np.where(rs.random_sample((k, 1)) < 0.25, -1, 1)).astype(F)
    # 7. rays with a component that is not finite (hit() rejects nothing on a NaN; intersect() does, on T < tmax)
    bad = np.array([np.nan, np.inf, -np.inf], dtype=F)
    j = 7 * k - 48 + np.arange(48)
    d[j[:24], np.arange(24) % 3] = bad[np.arange(24) // 3 % 3]
    o[j[24:], np.arange(24) % 3] = bad[np.arange(24) // 3 % 3]
    return words(o, d, v00, v10, v11, v01, tmin, tmax)


def quad_hit_branches(cases) -> dict:
    """Which branches of Surface.h:58-158 a case takes, restated in float32 for counting only: the reference's
    recorded `hit` decides who reached the bilinear part."""
    c = np.asarray(cases, dtype=U).view(F)
    o, d, v00, v10, v11, v01 = (c[:, 3 * j:3 * j + 3] for j in range(6))
    cross = lambda a, b: np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                                   a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(F)
    dot = lambda a, b: ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(F) + a[:, 2] * b[:, 2]).astype(F)
    with np.errstate(all="ignore"):
        E03, E01, E02 = v01 - v00, v10 - v00, v11 - v00
        P = cross(d, E03)
        det = dot(E01, P)
        inv = (F(1) / det).astype(F)
        T = o - v00
        alpha = (dot(T, P) * inv).astype(F)
        beta = (dot(d, cross(T, E01)) * inv).astype(F)
        nn = np.abs(cross(E01, E02))
        ax = np.where((nn[:, 0] >= nn[:, 1]) & (nn[:, 0] >= nn[:, 2]), 0, np.where((nn[:, 1] >= nn[:, 0]) & (nn[:, 1] >= nn[:, 2]), 1, 2))
        n_ax = np.take_along_axis(cross(E01, E02), ax[:, None], 1)[:, 0]
        a11 = np.where(ax == 0, E02[:, 1] * E03[:, 2] - E02[:, 2] * E03[:, 1],
                       np.where(ax == 1, E02[:, 2] * E03[:, 0] - E02[:, 0] * E03[:, 2], E02[:, 0] * E03[:, 1] - E02[:, 1] * E03[:, 0])).astype(F) / n_ax
        b11 = np.where(ax == 0, E01[:, 1] * E02[:, 2] - E01[:, 2] * E02[:, 1],
                       np.where(ax == 1, E01[:, 2] * E02[:, 0] - E01[:, 0] * E02[:, 2], E01[:, 0] * E02[:, 1] - E01[:, 1] * E02[:, 0])).astype(F) / n_ax
        eps = F(1e-5)
        bil = np.where(np.abs(a11 - F(1)) < eps, 0, np.where(np.abs(b11.astype(np.float64) - 1.0) < eps, 1, 2))
    return dict(det=det, alpha=alpha, beta=beta, axis=ax, bilinear=bil)


def sphere_hit_cases(scs) -> np.ndarray:
    rs = _rs("sphere_hit")
    n, k = N_STAGE, N_STAGE // 8
    c = _uni(rs, 0.1, 0.9, (n, 3))
    r = _uni(rs, 0.02, 0.3, n)
    o = _uni(rs, -0.5, 1.5, (n, 3))
    # aim at a point at 0 .. 1.3 radii from the centre: hits, grazes and misses
    off = _dirs(rs, n).astype(np.float64)
    off /= np.sqrt((off * off).sum(1, keepdims=True))
    frac = 1.3 * rs.random_sample(n)
    frac[:k] = 1.0 + (rs.random_sample(k) - 0.5) * 2e-6  # the discriminant either side of 0
    tgt = c + off * (frac * r)[:, None]
    d = (tgt - o).astype(F)
    # perpendicular offset needs d perpendicular to off: project the origin into the plane through tgt
    oo = o.astype(np.float64)
    oo[:k] -= off[:k] * ((oo[:k] - tgt[:k]) * off[:k]).sum(1, keepdims=True)
    o[:k] = oo[:k].astype(F)
    d[:k] = (tgt[:k] - o[:k]).astype(F)
    tmin, tmax = np.full(n, F(0.001)), np.full(n, FLT_MAX)
    # origins inside the sphere: the second root
    s = slice(k, 2 * k)
    o[s] = (c[s] + off[s] * (0.9 * rs.random_sample((k, 1)) * r[s, None])).astype(F)
    d[s] = _dirs(rs, k)
    # origins on the surface, leaving and entering (the first root near tmin)
    s = slice(2 * k, 3 * k)
    o[s] = (c[s] + off[s] * r[s, None]).astype(F)
    d[s] = _dirs(rs, k)
    # both roots outside (tmin, tmax): behind the origin, or beyond a tmax left by a quad
    s = slice(3 * k, 4 * k)
    d[s] = -d[s]
    s = slice(4 * k, 5 * k)
    t1 = np.sqrt((((c[s] - o[s]).astype(np.float64)) ** 2).sum(1)) / np.sqrt((d[s].astype(np.float64) ** 2).sum(1))
    tmax[s] = (t1 * (0.2 + 1.2 * rs.random_sample(k))).astype(F)
    # far origins: |o - c| = 1e3
    s = slice(5 * k, 6 * k)
    o[s] = (tgt[s] - off[np.roll(np.arange(n), 7)[s]] * 1e3).astype(F)
    d[s] = ((tgt[s] - o[s]) * _pow10(rs.randint(-3, 1, (k, 1))).astype(F)).astype(F)
    return words(o, d, c, r, tmin, tmax)


def _surface_points(rs, sc, n):
    """Points on the scene's quads and spheres with their normals (float32; the normal's side random)."""
    V = scene_verts(sc)
    q = _pick(rs, n, len(V))
    u, v = _uni(rs, 0, 1, (n, 1)), _uni(rs, 0, 1, (n, 1))
    p = (V[q, 0] + u * (V[q, 1] - V[q, 0]) + v * (V[q, 3] - V[q, 0])).astype(F)
    nn = np.cross((V[q, 1] - V[q, 0]).astype(np.float64), (V[q, 2] - V[q, 0]).astype(np.float64))
    nn = (nn / np.sqrt((nn * nn).sum(1, keepdims=True))).astype(F)
    ns = min(sc.n_spheres, 3)
    m = n // 4
    k = _pick(rs, m, ns)
    ctr = sc.points_np()[np.ctypeslib.as_array(sc.sphere_point)[:ns][k]]
    rad = np.ctypeslib.as_array(sc.sphere_radius)[:ns][k]
    off = _dirs(rs, m).astype(np.float64)
    off /= np.sqrt((off * off).sum(1, keepdims=True))
    p[:m] = (ctr + off * rad[:, None]).astype(F)
    nn[:m] = off.astype(F)
    nn *= np.where(rs.random_sample((n, 1)) < 0.5, -1, 1).astype(F)
    return p, nn


def light_geometry(sc):
    P = sc.points_np()
    ids = list(sc.light_box_pointids)[1:]
    return P[ids], P[sc.light_sphere_point], F(sc.sphere_radius[0])


def hit_points_cases(sc, tag):
    """Hit points and normals for the generator, pdf and scatter stages: surface points of the scene, points on the
    light quad and under its edges, points inside the light sphere (the sampler's sqrt of a negative), axis normals."""
    rs = _rs(tag)
    n, k = N_STAGE, N_STAGE // 8
    p, nn = _surface_points(rs, sc, n)
    lq, lc, lr = light_geometry(sc)
    u, v = _uni(rs, 0, 1, (k, 1)), _uni(rs, 0, 1, (k, 1))
    p[:k] = (lq[0] + u * (lq[1] - lq[0]) + v * (lq[3] - lq[0])).astype(F)        # on the light quad itself
    e = _pick(rs, k, 4)
    w = _uni(rs, 0, 1, (k, 1))
    under = (lq[e] + w * (lq[(e + 1) % 4] - lq[e])).astype(F)
    under[:, 1] = _uni(rs, 0, 1, k) * under[:, 1]
    p[k:2 * k] = under                                                           # under its edges
    off = _dirs(rs, k).astype(np.float64)
    off /= np.sqrt((off * off).sum(1, keepdims=True))
    p[2 * k:3 * k] = (lc + off * (lr * 0.999 * rs.random_sample((k, 1)))).astype(F)  # inside the light sphere
    ax = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=F)
    nn[3 * k:4 * k] = ax[_pick(rs, k, 6)]
    return p, nn


def generator_cases(sc) -> np.ndarray:
    rs = _rs("generator")
    n = N_STAGE
    p, nn = hit_points_cases(sc, "generator.points")
    kind = np.arange(n) % 3
    which = kind + 1
    off = rs.random_sample(n) < 0.1  # a worklet given another's `which` leaves the direction alone
    which = np.where(off, (which % 3) + 1, which)
    which[(kind == 0) & (rs.random_sample(n) < 0.1)] = 0  # `which <= current`
    seeds = rs.randint(0, 1 << 32, n, dtype=np.uint64).astype(U)
    return words(kind.astype(np.int32), which.astype(np.int32), nn, p, seeds)


def light_pdf_cases(sc) -> np.ndarray:
    """Generated directions toward the light quad and sphere: inside, across the edge, grazing, from behind."""
    rs = _rs("light_pdf")
    n, k = N_STAGE, N_STAGE // 8
    p, _ = hit_points_cases(sc, "light_pdf.points")
    lq, lc, lr = light_geometry(sc)
    kind = np.arange(n) % 2
    u, v = _uni(rs, -0.15, 1.15, (n, 1)), _uni(rs, -0.15, 1.15, (n, 1))
    tq = (lq[0] + u * (lq[1] - lq[0]) + v * (lq[3] - lq[0])).astype(F)
    off = _dirs(rs, n).astype(np.float64)
    off /= np.sqrt((off * off).sum(1, keepdims=True))
    ts = (lc + off * (lr * 1.2 * rs.random_sample((n, 1)))).astype(F)
    tgt = np.where(kind[:, None] == 0, tq, ts)
    g = ((tgt - p) * _uni(rs, 0.25, 2.0, (n, 1))).astype(F)
    # from behind the light quad (above it), and grazing it
    p[4 * k:5 * k, 1] = lq[0][1] + _uni(rs, 0.0, 0.2, k)
    g[4 * k:5 * k] = (tgt[4 * k:5 * k] - p[4 * k:5 * k]).astype(F)
    p[5 * k:6 * k, 1] = _nudge(np.full(k, lq[0][1], dtype=F), rs.randint(-40, 41, k))
    g[5 * k:6 * k] = (tgt[5 * k:5 * k + k] - p[5 * k:6 * k]).astype(F)
    g[6 * k:6 * k + 64] = 0
    fin = np.full(n, 8, dtype=np.int32)
    fin[rs.random_sample(n) < 0.05] = 0  # a dead ray: neither a draw nor a term
    s_in = np.where(rs.random_sample(n) < 0.5, 0, _uni(rs, 0, 4, n)).astype(F)
    seeds = rs.randint(0, 1 << 32, n, dtype=np.uint64).astype(U)
    return words(kind.astype(np.int32), fin, p, g, s_in, seeds)


def material_cases(sc) -> np.ndarray:
    rs = _rs("material")
    n = N_STAGE
    p, nn = hit_points_cases(sc, "material.points")
    kind = np.arange(n) % 3
    # hit ids: materials 0-2 Lambertian, 3 the light, 4 glass (CornellBox.cpp's tables); mostly the worklet's own
    own = np.where(kind == 0, _pick(rs, n, 3), np.where(kind == 1, 3, 4))
    hm = np.where(rs.random_sample(n) < 0.85, own, _pick(rs, n, 5))
    ht = np.where(hm == 4, 0, hm)
    fin = np.where(rs.random_sample(n) < 0.9, 8, rs.randint(0, 32, n)).astype(np.int32)
    o = _uni(rs, 0, 1, (n, 3))
    d = _dirs(rs, n)
    d[rs.random_sample(n) < 0.1] *= F(40.0)
    hrec = np.concatenate([np.zeros((n, 2), dtype=F), _uni(rs, 0.01, 2, (n, 1)), nn, p], 1)
    seeds = rs.randint(0, 1 << 32, n, dtype=np.uint64).astype(U)
    return words(kind.astype(np.int32), fin, o, d, hrec, hm.astype(np.int32), ht.astype(np.int32), seeds)


def dielectric_geometry():
    """(d, n, p, ref_idx) of the dielectric scatter cases: both signs of dot(d, n), refraction possible and total
    internal reflection for rays leaving the glass, near-grazing and near-normal incidence, unnormalised directions."""
    rs = _rs("dielectric")
    n = N_STAGE
    nn = _dirs(rs, n).astype(np.float64)
    nn /= np.sqrt((nn * nn).sum(1, keepdims=True))
    tang = np.cross(nn, _dirs(rs, n).astype(np.float64) + 1e-3)
    tang /= np.sqrt((tang * tang).sum(1, keepdims=True))
    cos_i = rs.random_sample(n)
    k = n // 8
    cos_i[:k] = 1e-3 * rs.random_sample(k)            # grazing
    cos_i[k:2 * k] = 1 - 1e-4 * rs.random_sample(k)   # along the normal
    # leaving the glass near the critical angle: sin = 1/1.5 either side
    crit = np.sqrt(1 - (1 / 1.5) ** 2)
    cos_i[2 * k:3 * k] = crit * (1 + 2e-6 * (rs.random_sample(k) - 0.5))
    sign = np.where(rs.random_sample(n) < 0.5, -1.0, 1.0)  # -1: entering (dot < 0), +1: leaving
    sign[2 * k:3 * k] = 1.0
    d = sign[:, None] * cos_i[:, None] * nn + np.sqrt(1 - cos_i ** 2)[:, None] * tang
    scale = np.where(rs.random_sample(n) < 0.3, _pow10(rs.randint(-3, 4, n)), 1.0)
    d = (d * scale[:, None]).astype(F)
    p = _uni(rs, 0, 1, (n, 3))
    ior = np.full(n, F(1.5))
    ior[rs.random_sample(n) < 0.1] = F(1.33)
    return d, nn.astype(F), p, ior


def dielectric_cases(thresholds) -> np.ndarray:
    """thresholds: reflect_prob of every geometry as the reference decides it (float32; found by bisection on
    _rand, tools/make_ref_stage_golden.py).  _rand is a double: the draws a render can make (float32 values one
    ulp either side of reflect_prob and at it), doubles between two floats just below reflect_prob (where a float
    _rand would round up to it), 0, values of a uniform draw, and just below 1."""
    rs = _rs("dielectric.rand")
    d, nn, p, ior = dielectric_geometry()
    n = len(d)
    th = np.asarray(thresholds, dtype=F)
    r = rs.random_sample(n).astype(F).astype(np.float64)
    sel = np.arange(n) % 8
    r = np.where(sel == 0, _nudge(th, -1).astype(np.float64), r)
    r = np.where(sel == 1, th.astype(np.float64), r)
    r = np.where(sel == 2, _nudge(th, 1).astype(np.float64), r)
    below = th.astype(np.float64) - (th.astype(np.float64) - _nudge(th, -1).astype(np.float64)) * 0.25
    r = np.where(sel == 3, below, r)
    r = np.where(sel == 4, 0.0, r)
    r = np.where(sel == 5, np.float64(_nudge(np.ones(1, dtype=F), -1)[0]), r)
    r = np.minimum(r, np.float64(_nudge(np.ones(1, dtype=F), -1)[0]))  # _rand = 1 reads an unset vector in the reference
    bits = np.ascontiguousarray(r, dtype=np.float64).view(np.uint64)
    return words(d, nn, p, (bits & 0xFFFFFFFF).astype(U), (bits >> 32).astype(U), ior)


def dielectric_probe(rand32) -> np.ndarray:
    """The scatter cases with _rand = the given float32 values (the bisection's probes)."""
    d, nn, p, ior = dielectric_geometry()
    bits = np.ascontiguousarray(np.asarray(rand32, dtype=F).astype(np.float64)).view(np.uint64)
    return words(d, nn, p, (bits & 0xFFFFFFFF).astype(U), (bits >> 32).astype(U), ior)


def scatter_cases(sc) -> np.ndarray:
    rs = _rs("scatter")
    n, k = N_STAGE, N_STAGE // 8
    p, nn = hit_points_cases(sc, "scatter.points")
    lq, lc, lr = light_geometry(sc)
    fin = np.where(np.arange(n) % 4 == 3, 24, 8).astype(np.int32)  # specular every fourth
    fin[rs.random_sample(n) < 0.08] = 0                              # dead: attenuation 1, the ray kept
    fin[rs.random_sample(n) < 0.02] = 2                              # finished: nothing written
    o, d = _uni(rs, 0, 1, (n, 3)), _dirs(rs, n)
    srec = np.concatenate([_uni(rs, 0, 1, (n, 3)), _dirs(rs, n), _uni(rs, 0.05, 1, (n, 3))], 1)
    g = _dirs(rs, n)
    g[:k] = (nn[:k] + _dirs(rs, k) * F(0.5)).astype(F)          # around the normal
    g[k:2 * k] = -g[k:2 * k]
    g[2 * k:2 * k + 32] = 0                                       # a generator that de_nan'd everything
    perp = np.cross(nn[3 * k:4 * k], _dirs(rs, k)).astype(F)      # cosine near 0: the pdf's sign tests
    g[3 * k:4 * k] = perp
    s = np.where(rs.random_sample(n) < 0.4, 0, _uni(rs, 0, 6, n)).astype(F)
    s[4 * k:4 * k + 16] = np.nan                                  # a hit point inside the light sphere
    return words(fin, o, d, nn, p, srec, s, g)


def collect_cases() -> np.ndarray:
    return (np.arange(N_STAGE) % 256).astype(U).reshape(-1, 1)


def bounce_rays(name: str, sc):
    """4096 rays of one scene: camera rays of two cameras, rays started on surfaces, inside the glass sphere, aimed
    at the light's edges, and rays that miss everything.  Seeds are distinct and cover the whole range."""
    rs = _rs("bounce." + name)
    n, k = N_BOUNCE, N_BOUNCE // 8
    P = sc.points_np()
    lo, hi = P.min(0), P.max(0)
    ext = F((hi - lo).max())
    mid = ((lo + hi) * F(0.5)).astype(F)
    o = np.zeros((n, 3), dtype=F)
    d = np.zeros((n, 3), dtype=F)
    eye1 = (mid + np.array([0, 0, -1.94], dtype=F) * ext).astype(F)          # the reference's view, roughly
    eye2 = (mid + np.array([0.35, 0.4, -0.45], dtype=F) * ext).astype(F)     # inside, looking down and across
    tg = (lo + _uni(rs, 0, 1, (2 * k, 3)) * (hi - lo)).astype(F)
    o[:k], o[k:2 * k] = eye1, eye2
    d[:2 * k] = (tg - o[:2 * k]).astype(F)
    d[:2 * k] = (d[:2 * k] / np.sqrt((d[:2 * k] * d[:2 * k]).sum(1, keepdims=True)).astype(F)).astype(F)
    p, nn = _surface_points(rs, sc, 3 * k)                                   # rays a bounce would start
    o[2 * k:5 * k] = p
    d[2 * k:5 * k] = _dirs(rs, 3 * k)
    gc, gr = P[sc.sphere_point[0]], F(sc.sphere_radius[0])                  # inside sphere 0 (glass in every scene)
    off = _dirs(rs, k)
    o[5 * k:6 * k] = (gc + off * (gr * F(1.1))).astype(F)
    d[5 * k:6 * k] = _dirs(rs, k)
    lq, _, _ = light_geometry(sc)                                            # at the light's edges, from below and above
    e = _pick(rs, k, 4)
    w = _uni(rs, 0, 1, (k, 1))
    tgt = _nudge(lq[e] + w * (lq[(e + 1) % 4] - lq[e]), rs.randint(-3, 4, (k, 3)))
    tgt = (tgt + _dirs(rs, k) * F(0.02) * (rs.random_sample((k, 1)) < 0.5)).astype(F)
    o[6 * k:7 * k] = (lo + _uni(rs, 0.05, 0.95, (k, 3)) * (hi - lo)).astype(F)
    o[6 * k:6 * k + k // 4, 1] = hi[1] + F(0.01) * ext
    d[6 * k:7 * k] = (tgt - o[6 * k:7 * k]).astype(F)
    o[7 * k:] = (mid + _dirs(rs, n - 7 * k) * ext * F(3.0)).astype(F)        # outside, pointing away: misses
    d[7 * k:] = (o[7 * k:] - mid).astype(F)
    half = (n - 7 * k) // 2
    d[7 * k + half:] = (mid - o[7 * k + half:] + _dirs(rs, n - 7 * k - half) * ext).astype(F)  # and back in
    seeds = rs.randint(0, 1 << 32, n, dtype=np.uint64).astype(U)
    seeds[:8] = [0, 0xFFFFFFFF, 61, 1, 2, 3, 1 << 31, 639999]
    return np.ascontiguousarray(np.concatenate([o, d], 1)), seeds


def stage_cases(name: str, scs, fixture=None) -> np.ndarray:
    sc = scs[STAGE_SCENE]
    if name in ("rng", "which"):
        return seeds_cases()
    if name == "dielectric_scatter":
        return dielectric_cases(fixture["dielectric_thresholds"])
    return {"onb": onb_cases, "quad_hit": lambda: quad_hit_cases(scs), "sphere_hit": lambda: sphere_hit_cases(scs),
            "material": lambda: material_cases(sc), "generator": lambda: generator_cases(sc),
            "light_pdf": lambda: light_pdf_cases(sc), "scatter": lambda: scatter_cases(sc),
            "collect": collect_cases}[name]()


# ---------------------------------------------------------------- outcomes --
OUTCOMES = ("missed", "light_front", "light_behind", "lambertian_cosine", "lambertian_quad", "lambertian_sphere",
            "dielectric")


def bounce_outcomes(sc, rec) -> np.ndarray:
    """Index into OUTCOMES of every ray, from the recorded states (rec: (n, 13, 37) words)."""
    mt = np.ctypeslib.as_array(sc.mat_type)
    after_collect = rec[:, 2, REC["status"]]
    last = rec[:, 12]
    hit_mt = mt[last[:, REC["M"]].astype(np.int64) % len(mt)]
    E = last[:, REC["E"]:REC["E"] + 3].view(F)
    which = last[:, REC["which"]].view(np.int32)
    out = np.full(len(rec), -1, dtype=np.int8)
    missed = (after_collect & 8) == 0
    out[missed] = 0
    out[~missed & (hit_mt == 1) & (E != 0).any(1)] = 1
    out[~missed & (hit_mt == 1) & (E == 0).all(1)] = 2
    for w in (1, 2, 3):
        out[~missed & (hit_mt == 0) & (which == w)] = 2 + w
    out[~missed & (hit_mt == 2)] = 6
    assert (out >= 0).all()
    return out


FINAL_TYPES = "u" + "f" * 12 + "uu"


def final_state(rec) -> np.ndarray:
    """What rtp_debug_bounce reports for a ray, from the reference's state after PDFCosineWorklet (rec: (n, 13, 37)
    words): (n, 15) words = result, emitted[0], attenuation[0], origin, direction, seed, non-finite flag.
      result 1 (missed): no scatter bit after CollectIntersecttWorklet, which set attenuation 1 and emitted 0;
      result 2 (light): status 0 after a hit, emitted[0] as DiffuseLightWorklet left it, attenuation 1;
      result 0: the path goes on from the new origin and direction with attenuation[0];
      the seed is the reference's after every draw of the depth, a dead ray's generator draws included;
      the flag is set where a path that goes on stored an attenuation that is not finite."""
    last = rec[:, 12]
    missed = (rec[:, 2, REC["status"]] & 8) == 0
    status = last[:, REC["status"]]
    code = np.where(missed, 1, np.where(status == 0, 2, 0)).astype(U)
    A = last[:, REC["A"]:REC["A"] + 3]
    nonfinite = ((code == 0) & ~np.isfinite(np.ascontiguousarray(A).view(F)).all(1)).astype(U)
    cols = [code[:, None]] + [last[:, REC[k]:REC[k] + 3] for k in ("E", "A", "org", "dir")] + [last[:, REC["seed"], None], nonfinite[:, None]]
    return canonical(np.concatenate(cols, 1), FINAL_TYPES)


def coverage(fx, scs):
    """The counts the issue lists, from the reference's results."""
    c = {}
    for nm in BOUNCE_SCENES:
        for k, v in zip(OUTCOMES, np.bincount(fx[nm + "_outcome"], minlength=len(OUTCOMES))):
            c[k] = c.get(k, 0) + int(v)
    cls = fx["dielectric_class"]
    for k, name in enumerate(("dielectric_reflected_schlick", "dielectric_refracted", "dielectric_total_internal")):
        c[name] = int((cls == k).sum())
    cases = stage_cases("generator", scs).view(np.int32)
    gen = fx["generator_out"][:, :3].view(F)
    took = np.where(cases[:, 0] == 0, cases[:, 1] <= 1, cases[:, 1] == cases[:, 0] + 1)
    c["de_nan_changed"] = int(((cases[:, 0] == 2) & took & (gen == 0).all(1)).sum())
    cases = stage_cases("light_pdf", scs)
    live = (cases[:, 1] & 8) != 0
    same = fx["light_pdf_out"][:, 0] == cases[:, 8]  # sum_value left as it was: a zero pdf
    for k, name in enumerate(("quad_pdf", "sphere_pdf")):
        m = live & (cases[:, 0] == k) & (cases[:, 8].view(F) == 0)
        c[name + "_zero"], c[name + "_nonzero"] = int((m & same).sum()), int((m & ~same).sum())
    cases = stage_cases("quad_hit", scs)
    out = fx["quad_hit_out"]
    br = quad_hit_branches(cases)
    hit = out[:, 0] != 0
    for a in range(3):
        c[f"quad_hit_axis{a}"] = int((hit & (br["axis"] == a)).sum())
        c[f"quad_hit_bilinear{a}"] = int((hit & (br["bilinear"] == a)).sum())
    with np.errstate(all="ignore"):
        ab = br["alpha"] + br["beta"]
    c["quad_hit_first_triangle"], c["quad_hit_second_triangle"] = int((hit & (ab <= 1)).sum()), int((hit & (ab > 1)).sum())
    near = np.abs(br["det"]) < 4e-5
    c["quad_hit_det_below_eps"] = int((near & (np.abs(br["det"]) < F(1e-5))).sum())
    c["quad_hit_det_above_eps"] = int((near & ~(np.abs(br["det"]) < F(1e-5)) & hit).sum())
    tmin, tmax = cases[:, 18].view(F), cases[:, 19].view(F)
    t = out[:, 3].view(F)
    isect = out[:, 4] != 0
    c["quad_hit_t_below_tmin"] = int((hit & ~isect & (t <= tmin)).sum())
    c["quad_hit_t_above_tmin"] = int((isect & (t < 2 * tmin)).sum())
    c["quad_hit_t_below_tmax"] = int((isect & (tmax < FLT_MAX)).sum())
    c["quad_hit_t_beyond_tmax"] = int((hit & ~isect & (t >= tmax)).sum())
    c["quad_hit_in_plane_rejected"] = int((~hit & (np.abs(br["det"]) < F(1e-5))).sum())
    so = fx["sphere_hit_out"]
    sc_ = stage_cases("sphere_hit", scs).view(F)
    c["sphere_hit"], c["sphere_miss"] = int((so[:, 0] != 0).sum()), int((so[:, 0] == 0).sum())
    oc = sc_[:, 0:3] - sc_[:, 6:9]
    inside = (oc * oc).sum(1) < sc_[:, 9] * sc_[:, 9] * F(0.98)
    c["sphere_hit_second_root"] = int(((so[:, 0] != 0) & inside).sum())
    return c


# ------------------------------------------- the hit stages as whole scenes --
def hit_scenes(oracle, scs) -> dict:
    """The quad cases' quads but the degenerate ones (the zoo's, the Cornell box's and the synthetic ones: 76 of the
    device's 256) and 253 of
    the sphere cases' spheres, each added to the zoo, with the cases' rays: name -> (Scene, rays (n, 6), the _scenes.Zoo it was made from).  Only the finite
    rays: the device's quad tests are exact for finite rays (rtp_device.hpp, "Zero structure"), which is what a
    render gives them (directions are de_nan'd, origins are hit points); the oracle takes the others too."""
    import _scenes

    zq = _scenes.zoo()
    for v in np.concatenate([scene_verts(scs["cornell0"]), synthetic_quads(degenerate=False)]):
        zq.add_quad(v, _scenes.WHITE)  # (a degenerate quad has no unit normal for the device's quad table)
    assert len(zq.quads) <= _scenes.MAX_QUADS and np.array_equal(zq.verts(), quad_pool(scs, degenerate=False))
    zs = _scenes.zoo()
    c = sphere_hit_cases(scs).view(F)
    for j in range(256 - len(zs.spheres)):
        zs.add_sphere(c[j, 6:9], c[j, 9], _scenes.GREEN)
    # The far origins (|o - c| = 1e3) go to a scene of their own with 8 spheres, which the device scans one by one.
    # From 9 spheres on it walks a BVH whose boxes cull soundly only for origins within two diagonals of the scene
    # (include/rtp.h rtp_set_scene): at 1e3 float32 accepts rays passing a sphere by more than its radius.
    k = N_STAGE // 8
    far = np.arange(5 * k, 6 * k)
    zf = _scenes.zoo()
    for j in far[:8 - len(zf.spheres)]:
        zf.add_sphere(c[j, 6:9], c[j, 9], _scenes.GREEN)
    rq = np.ascontiguousarray(quad_hit_cases(scs)[:, :6]).view(F)
    near = np.setdiff1d(np.arange(N_STAGE), far)
    return {"hit_quads": (zq.scene(oracle), np.ascontiguousarray(rq[np.isfinite(rq).all(1)]), zq),
            "hit_spheres": (zs.scene(oracle), np.ascontiguousarray(c[near, :6]), zs),
            "hit_spheres_far": (zf.scene(oracle), np.ascontiguousarray(c[far, :6]), zf)}


def reference_closest_hits(sc, rays, exe: str = REF_STAGES) -> np.ndarray:
    """(n, 3) words (t bits, kind, index) as rtp_debug_closest_hit reports a hit: the minimum over the reference's
    own per-primitive t (QuadLeafIntersector::intersect and SphereLeafIntersector::hit of every ray against every
    primitive, within (0.001, FLT_MAX)), a tie to the lower index, a sphere only when strictly nearer than the
    quads (BVHTraverser.h:225-226: the spheres' tmax is the quads' t); a miss is (FLT_MAX, -1, 0)."""
    rays = np.ascontiguousarray(rays, dtype=F)
    n = len(rays)

    def nearest(stage, prim, flag_col, t_col):
        m = len(prim)
        cases = words(np.repeat(rays, m, 0), np.tile(prim, (n, 1)), np.full(n * m, F(0.001)), np.full(n * m, FLT_MAX))
        out = driver_stage(stage, sc, cases, exe)
        t = np.where(out[:, flag_col] != 0, out[:, t_col].view(F), F(np.inf)).reshape(n, m)
        i = t.argmin(1)
        return t[np.arange(n), i], i

    V = scene_verts(sc)
    tq, iq = nearest("quad_hit", V.reshape(len(V), 12), 4, 5)
    ns = sc.n_spheres
    ctr = sc.points_np()[np.ctypeslib.as_array(sc.sphere_point)[:ns]]
    rad = np.ctypeslib.as_array(sc.sphere_radius)[:ns].astype(F)
    ts, isph = nearest("sphere_hit", np.concatenate([ctr, rad[:, None]], 1), 0, 1)
    out = np.zeros((n, 3), dtype=U)
    out[:, 0] = fbits(np.full(n, FLT_MAX))
    out[:, 1] = 0xFFFFFFFF
    hq = np.isfinite(tq)
    out[hq] = np.stack([fbits(tq[hq]), np.zeros(hq.sum(), dtype=U), iq[hq].astype(U)], 1)
    hs = np.isfinite(ts) & (ts < np.where(hq, tq, FLT_MAX))
    out[hs] = np.stack([fbits(ts[hs]), np.ones(hs.sum(), dtype=U), isph[hs].astype(U)], 1)
    return out


# ------------------------------------------- ray generation, the backward product, whole frames --
# tests/golden/ref_frames.npz: what the reference's own Camera::RayGen (pathtracing/Camera.cxx), details::WangInit
# (MapperPathTracer.cxx), BinarySliceTransformIdxKernel (PathAlgorithms.h) and the whole sample and depth loop of
# RenderCellsImpl over its worklets compute (ref_stage_driver.cpp modes camera, raygen, seed_init, backward, frame).
FRAMES_FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_frames.npz")
# name: (driver mode, words per case (None: set by the rows), result word types)
FRAME_STAGES = {
    "camera": (12, 12, "f" * 9),      # position, look-at, up, fov, nx, ny -> nlook, delta_x, delta_y
    "raygen": (13, 14, "fffui"),      # ... work index, seed -> direction, seed after, pixelIndex
    "seed_init": (14, 1, "u"),        # the stencil value -> WangInit's value of it
    "backward": (15, None, "ffff"),   # D, S, S x D x (emitted rgba, attenuation rgba) -> the canvas sum rgba
}
FRAME_MODE = 16
N_BACKWARD = 64
BACKWARD_SHAPES = tuple((d, s) for d in (1, 2, 3, 50) for s in (1, 4))
CANVASES = ((1, 1), (2, 2), (7, 40), (200, 120), (800, 800), (3840, 2160), (16384, 16384))
CORNERS_ONLY = (16384, 16384)  # 2^28 rays: taken at its corner indices only
FRAME_OUTCOMES = OUTCOMES + ("entered_dead",)


def cameras() -> dict:
    """name -> (position, look-at, up, fov): the default view, the scene zoo's, views along every axis with up
    along another (zeros in nlook, delta_x and delta_y), an up that is not a unit vector, an up nearly parallel to
    the look vector, a view at 555 scale, and fields of view from 1 to 179 degrees."""
    import _scenes

    d = (278 / 555.0, 278 / 555.0, -800 / 555.0), (278 / 555.0, 278 / 555.0, 278 / 555.0)
    h = _scenes.HIGH_CAM
    c = {
        "default": (*d, (0, 1, 0), 40.0),
        "high": (h["position"], h["look_at"], h["view_up"], h["fov_y"]),
        "skewed_up": ((0.85, 0.7, -1.0), (0.4, 0.45, 0.55), (0.1, 1.0, 0.05), 50.0),
        "along+x": ((-1.5, 0.5, 0.5), (0.5, 0.5, 0.5), (0, 0, 1), 40.0),
        "along-x": ((2.5, 0.5, 0.5), (0.5, 0.5, 0.5), (0, 1, 0), 40.0),
        "along+y": ((0.5, -1.5, 0.5), (0.5, 0.5, 0.5), (1, 0, 0), 40.0),
        "along-y": ((0.5, 2.5, 0.5), (0.5, 0.5, 0.5), (0, 0, -1), 40.0),
        "along+z": ((0.5, 0.5, -1.5), (0.5, 0.5, 0.5), (0, 1, 0), 40.0),
        "along-z": ((0.5, 0.5, 2.5), (0.5, 0.5, 0.5), (1, 0, 0), 40.0),
        "up_not_unit": (*d, (0, 2, 0), 40.0),
        "up_nearly_look": ((0.5, 0.5, -1.0), (0.5, 0.5, 0.5), (0, 0.001, 1), 40.0),
        "scale555": ((278, 278, -800), (278, 278, 278), (0, 1, 0), 40.0),
        "fov1": (*d, (0, 1, 0), 1.0),
        "fov90": (*d, (0, 1, 0), 90.0),
        "fov179": (*d, (0, 1, 0), 179.0),
        "down_left": ((0.9, 0.9, -0.6), (0.1, 0.2, 0.7), (-0.3, 0.8, 0.2), 65.0),
        # between the ceiling and the light quad, looking down (a quad's normal is turned to face the ray, so it
        # still emits), and inside the zoo's emissive sphere, whose outward normal makes it dark from within
        "above_light": ((0.5, 0.9995, 0.5), (0.5, 0.5, 0.5), (0, 0, 1), 150.0),
        "in_light_sphere": ((0.85, 0.8, 0.7), (0.5, 0.5, 0.5), (0, 1, 0), 40.0),
    }
    return {k: (np.asarray(p, dtype=F), np.asarray(a, dtype=F), np.asarray(u, dtype=F), F(f))
            for k, (p, a, u, f) in c.items()}


AXIS_CAMERAS = ("along+x", "along-x", "along+y", "along-y", "along+z", "along-z")


def camera_words(cam, nx, ny) -> np.ndarray:
    p, a, u, f = cam
    return np.concatenate([fbits(p), fbits(a), fbits(u), fbits([f]), np.array([nx, ny], dtype=U)])


def camera_cases() -> np.ndarray:
    """Every camera on every canvas: (18 * 7, 12) words."""
    return np.stack([camera_words(c, nx, ny) for c in cameras().values() for nx, ny in CANVASES])


def wang32_np(s):
    """wangXor.h:30-38, for building and counting cases only."""
    s = np.asarray(s, dtype=np.uint64) & 0xFFFFFFFF
    s = (s ^ 61) ^ (s >> 16)
    s = (s * 9) & 0xFFFFFFFF
    s = s ^ (s >> 4)
    s = (s * 0x27D4EB2D) & 0xFFFFFFFF
    return (s ^ (s >> 15)).astype(U)


def _seed_for_draws(first=None, second=None, rnd=None):
    """A seed whose first (second) hash is the given one; the other draw is whatever follows."""
    if first is not None:
        return inv_wang32(first)
    if second is not None:
        return inv_wang32(inv_wang32(second))
    return rnd


ONE_HASH = 4294967168  # the lowest hash whose draw is 1.0f (RNG known answers)
HALF_HASH = 1 << 31    # float(2^31) / 4294967295.f = 0.5f


def raygen_cases() -> np.ndarray:
    """(2048, 14) words: camera, canvas, work index, seed.
      - the four corners and the centre of every canvas (the corners only of the largest), under four cameras;
      - seeds whose first or second draw is exactly 0 and exactly 1.0f, at corners and random pixels;
      - the axis cameras on the columns where i + (1 - u) = nx/2 and the rows where j + v = ny/2 with u, v in
        {0, 0.5, 1}: a component of ray_dir is exactly zero there and the += 0.0000001f runs;
      - random pixels of random canvases under random cameras."""
    rs = _rs("raygen")
    cams = cameras()
    names = list(cams)
    rows = []

    def add(cam, nx, ny, idx, seed):
        rows.append(np.concatenate([camera_words(cams[cam], nx, ny), np.array([idx, seed], dtype=np.uint64).astype(U)]))

    def rseed():
        return int(rs.randint(0, 1 << 32, dtype=np.uint64))

    k = 0
    for nx, ny in CANVASES:
        pix = [0, nx - 1, nx * (ny - 1), nx * ny - 1] + ([] if (nx, ny) == CORNERS_ONLY else [(ny // 2) * nx + nx // 2])
        for p in pix:
            for _ in range(4):
                add(names[k % len(names)], nx, ny, p, rseed())
                k += 1
    small = [c for c in CANVASES if c != CORNERS_ONLY]
    edge_hashes = [0, ONE_HASH, 0xFFFFFFFF, ONE_HASH - 1, 1]
    for which in ("first", "second"):
        for t in edge_hashes:
            for nx, ny in small:
                for p in (0, nx * ny - 1, int(rs.randint(0, nx * ny))):
                    add(names[k % len(names)], nx, ny, p, int(_seed_for_draws(**{which: t})))
                    k += 1
    # the nudge: (draw hash, pixel coordinate) pairs that make a jitter term exactly zero
    for cam in AXIS_CAMERAS:
        for nx, ny in small:
            cols = [(0, nx // 2 - 1), (ONE_HASH, nx // 2), (0xFFFFFFFF, nx // 2)] if nx % 2 == 0 else [(HALF_HASH, nx // 2)]
            rows_ = [(0, ny // 2), (ONE_HASH, ny // 2 - 1), (0xFFFFFFFF, ny // 2 - 1)] if ny % 2 == 0 else [(HALF_HASH, ny // 2)]
            for t, i in cols:
                if 0 <= i < nx:
                    for j in sorted({0, ny - 1, int(rs.randint(0, ny))}):
                        add(cam, nx, ny, j * nx + i, int(inv_wang32(t)))
            for t, j in rows_:
                if 0 <= j < ny:
                    for i in sorted({0, nx - 1, int(rs.randint(0, nx))}):
                        add(cam, nx, ny, j * nx + i, int(inv_wang32(inv_wang32(t))))
            # both at once: the second hash is the hash of the first, so the pair is searched among the columns'
            for t, i in cols:
                t2 = int(wang32_np(t))
                v = F(t2) / F(4294967295.0)
                j = F(ny) / F(2) - v
                if 0 <= i < nx and j == np.floor(j) and 0 <= j < ny:
                    add(cam, nx, ny, int(j) * nx + i, int(inv_wang32(t)))
    while len(rows) < N_STAGE:
        nx, ny = small[int(rs.randint(0, len(small)))]
        add(names[int(rs.randint(0, len(names)))], nx, ny, int(rs.randint(0, nx * ny)), rseed())
    assert len(rows) == N_STAGE, len(rows)
    return np.stack(rows)


def raygen_nudged(cases, camera_out) -> np.ndarray:
    """(n, 3) bool: the components of ray_dir that are exactly zero before the nudge (Camera.cxx:513-517).  A float32
    restatement for counting only, like quad_hit_branches; the camera constants are the reference's recorded ones
    (camera_out rows in camera_cases() order)."""
    key = {camera_cases()[r, :12].tobytes(): r for r in range(len(camera_out))}
    con = np.stack([camera_out[key[c[:12].tobytes()]] for c in cases]).view(F)
    nlook, dx, dy = con[:, 0:3], con[:, 3:6], con[:, 6:9]
    nx, ny = cases[:, 10].astype(np.int64), cases[:, 11].astype(np.int64)
    idx = cases[:, 12].astype(np.int64)
    i, j = (idx % nx).astype(F), (idx // nx).astype(F)
    t1 = wang32_np(cases[:, 13])
    t2 = wang32_np(t1)
    u = t1.astype(F) / F(4294967295.0)
    v = t2.astype(F) / F(4294967295.0)
    a = ((F(2) * (i + (F(1) - u)) - nx.astype(F)) / F(2)).astype(F)
    b = ((F(2) * (j + v) - ny.astype(F)) / F(2)).astype(F)
    rd = ((nlook + (dx * a[:, None]).astype(F)).astype(F) + (dy * b[:, None]).astype(F)).astype(F)
    return rd == 0


def backward_cases(d: int, s: int) -> np.ndarray:
    """(64, 2 + 8*s*d) words: per sample and depth emitted rgba and attenuation rgba.  Ordinary paths (emitted mostly
    0, attenuation 0 .. 2); paths that died on the light at a random depth (emitted 15 there, then attenuation 1 and
    emitted 0 to the end: CollectIntersecttWorklet's planes of a dead ray); entries with inf, NaN and -0, and
    0 * inf both ways round."""
    rs = _rs(f"backward.{d}.{s}")
    n = N_BACKWARD
    E = np.where(rs.random_sample((n, s, d, 4)) < 0.8, 0, _uni(rs, 0, 15, (n, s, d, 4))).astype(F)
    A = _uni(rs, 0, 2, (n, s, d, 4))
    k = n // 4
    for r in range(k, 2 * k):  # died on the light
        for q in range(s):
            at = int(rs.randint(0, d))
            E[r, q, :at] = 0
            E[r, q, at] = F(15)
            E[r, q, at + 1:] = 0
            A[r, q, at:] = 1
    special = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, FLT_MAX, 1e-45], dtype=F)
    for r in range(2 * k, 3 * k):  # one special entry somewhere, in either array
        for q in range(s):
            arr = E if rs.random_sample() < 0.5 else A
            arr[r, q, int(rs.randint(0, d)), int(rs.randint(0, 3))] = special[int(rs.randint(0, len(special)))]
    for r in range(3 * k, n):  # 0 * inf: an infinite radiance under a zero attenuation, and the other way round
        for q in range(s):
            at = int(rs.randint(0, d))
            c = int(rs.randint(0, 3))
            if rs.random_sample() < 0.5:
                E[r, q, at, c], A[r, q, :at, c] = np.inf, 0
            else:
                E[r, q, at, c] = 0
                E[r, q, at + 1:, c] = 0
                A[r, q, :at, c] = np.inf
    body = np.concatenate([fbits(E), fbits(A)], axis=3).reshape(n, s * d * 8)
    head = np.tile(np.array([d, s], dtype=U), (n, 1))
    return np.ascontiguousarray(np.concatenate([head, body], 1))


def frame_stage_cases(name: str) -> np.ndarray:
    if name == "camera":
        return camera_cases()
    if name == "raygen":
        return raygen_cases()
    if name == "seed_init":
        return np.array([[1]], dtype=U)  # the constant stencil of MapperPathTracer.cxx:266
    raise KeyError(name)


def driver_frame_stage(name: str, sc, cases, exe: str = REF_STAGES) -> np.ndarray:
    mode, kin, types = FRAME_STAGES[name]
    assert kin is None or cases.shape[1] == kin
    return run_driver(mode, len(types), sc, cases, exe)


# name: (scene, camera, nx, ny, spp, depth)
FRAMES = {
    "cornell0": ("cornell0", "default", 24, 16, 4, 8),
    "cornell1": ("cornell1", "default", 24, 16, 4, 8),
    "cornell2": ("cornell2", "default", 24, 16, 4, 8),
    "cornell3": ("cornell3", "default", 24, 16, 4, 8),
    "zoo": ("zoo", "default", 24, 16, 4, 8),
    "cornell1_deep": ("cornell1", "default", 8, 8, 2, 50),
    "one_pixel": ("cornell0", "default", 1, 1, 4, 8),
    "depth1": ("cornell2", "skewed_up", 12, 8, 4, 1),
    "depth2": ("cornell2", "high", 12, 8, 4, 2),
    "above_light": ("cornell2", "above_light", 12, 8, 4, 8),
    "in_light_sphere": ("zoo", "in_light_sphere", 12, 8, 4, 8),
}


def frame_case(name: str) -> np.ndarray:
    _, cam, nx, ny, spp, depth = FRAMES[name]
    return np.concatenate([camera_words(cameras()[cam], nx, ny), np.array([spp, depth], dtype=U)]).reshape(1, -1)


def driver_frame(name: str, scs, exe: str = REF_STAGES):
    """The reference's frame: (pixels (n, 5) words: rgb bits, final seed, live count; states (spp, depth, n, 37))."""
    scn, _, nx, ny, spp, depth = FRAMES[name]
    n = nx * ny
    case = frame_case(name)
    with tempfile.TemporaryDirectory() as td:
        fin, fout = os.path.join(td, "cases.bin"), os.path.join(td, "results.bin")
        with open(fin, "wb") as fh:
            np.array([MAGIC, FRAME_MODE, 1, case.shape[1]], dtype=U).tofile(fh)
            scene_words(scs[scn]).tofile(fh)
            case.tofile(fh)
        subprocess.run([exe, fin, fout], check=True)
        res = np.fromfile(fout, dtype=U)
    assert res[:3].tolist() == [FRAME_MODE, 1, 5 * n + spp * depth * n * REC_WORDS], res[:3]
    return res[3:3 + 5 * n].reshape(n, 5), res[3 + 5 * n:].reshape(spp, depth, n, REC_WORDS)


def canonical_states(states) -> np.ndarray:
    return canonical(np.asarray(states).reshape(-1, REC_WORDS), REC_TYPES).reshape(np.asarray(states).shape)


def state_digests(states) -> list:
    """SHA-256 of all rays' canonical states after every depth of every sample: [sample][depth]."""
    can = canonical_states(states)
    return [[digest(can[s, d]) for d in range(can.shape[1])] for s in range(can.shape[0])]


def frame_outcomes(sc, states) -> np.ndarray:
    """(spp, depth, n) int8 index into FRAME_OUTCOMES of what each depth did to each ray, from the recorded states:
    a ray enters a depth alive at depth 0 (Status = 8, MapperPathTracer.cxx:283) or where the state before has the
    scatter bit; one that leaves without it has missed (T still FLT_MAX) or ended on the light."""
    st = canonical_states(states)
    mt = np.ctypeslib.as_array(sc.mat_type)
    alive_after = (st[..., REC["status"]] & 8) != 0
    entered = np.concatenate([np.ones_like(alive_after[:, :1]), alive_after[:, :-1]], 1)
    T = st[..., REC["T"]].view(F)
    hit_mt = mt[st[..., REC["M"]].astype(np.int64) % len(mt)]
    E = st[..., REC["E"]:REC["E"] + 3].view(F)
    which = st[..., REC["which"]].view(np.int32)
    out = np.full(alive_after.shape, -1, dtype=np.int8)
    out[~entered] = 7
    ended = entered & ~alive_after
    out[ended & (T == FLT_MAX)] = 0
    lit = ended & (T != FLT_MAX)
    assert (hit_mt[lit] == 1).all()
    out[lit & (E != 0).any(-1)] = 1
    out[lit & (E == 0).all(-1)] = 2
    for w in (1, 2, 3):
        out[entered & alive_after & (hit_mt == 0) & (which == w)] = 2 + w
    out[entered & alive_after & (hit_mt == 2)] = 6
    assert (out >= 0).all()
    return out


def frame_coverage(fx) -> dict:
    """Ray-depths of every outcome over all recorded frames, and the samples that start on a ray whose previous
    sample had died before its last depth (so that stale normals, points and records are what the dead depths and
    the next sample find)."""
    c = {k: 0 for k in FRAME_OUTCOMES}
    c["sample_after_early_death"] = 0
    for nm in FRAMES:
        oc = fx[nm + "_outcome"]
        for k, v in zip(FRAME_OUTCOMES, np.bincount(oc.reshape(-1), minlength=len(FRAME_OUTCOMES))):
            c[k] += int(v)
        c["sample_after_early_death"] += int((oc[:-1, -1] == 7).sum())
    return c


def frame_stage_coverage(fx) -> dict:
    nud = raygen_nudged(raygen_cases(), fx["camera_out"])
    c = {f"raygen_nudged_{a}": int(nud[:, k].sum()) for k, a in enumerate("xyz")}
    cases = raygen_cases()
    t1 = wang32_np(cases[:, 13])
    t2 = wang32_np(t1)
    c["raygen_first_draw_0"], c["raygen_first_draw_1"] = int((t1 == 0).sum()), int((t1 >= ONE_HASH).sum())
    c["raygen_second_draw_0"], c["raygen_second_draw_1"] = int((t2 == 0).sum()), int((t2 >= ONE_HASH).sum())
    return c
