// rtp_trace.hpp -- the per-ray device code of the path tracer: the quad and
// sphere tests, the sphere-BVH walks, closest_hit, one depth of a path
// (bounce / shade_hit), path_radiance, the camera ray and the pixel-index
// arithmetic.  Device functions only: the kernels that run them are in
// rtp_pool.hpp (the renders) and rtp_diag.hpp (diagnostics and utilities).
#pragma once
#include <hip/hip_runtime.h>

#include "rtp_device.hpp"

namespace rtp {

typedef uint32_t u16v __attribute__((ext_vector_type(16)));  // 64 bytes: one s_load_dwordx16

struct Hit {
  float t;
  int kind;  // -1 none, 0 quad, 1 sphere
  int idx;
};

// Closest hit over every quad then every sphere with tmax from the quads: the
// closest-hit semantics of BVHTraverser.h:128-227 over Surface.h:208-254 /
// 376-409 with quads visited in index order and a strict '<'.  That scan
// returns the lexicographic minimum of (t, index) over the hits, so the quads
// can be visited grouped by zero-structure kind (one tight loop per kind) as
// long as equal t is broken by the original index.
// The (t, orig) minimum as one unsigned 64-bit key {bits(t), orig << 8 | q}:
// an accepted t is > 0.001, and positive floats order like their bit
// patterns, so key order is exactly "t, then reference index".  The scan
// position q rides in the low bits (orig is unique, so it never decides).
static_assert(kMaxQuads <= 256, "key_lo packs orig and the scan position in 8 bits each");
constexpr uint64_t kNoHitKey = (uint64_t)0x7f7fffffu << 32 | 0xffffffffu;  // {FLT_MAX, none}
// The scan reads the quads' 64-byte scan heads (QuadGeom) as one
// s_load_dwordx16 each, the NEXT quad's issued before the current one is
// tested, so its scalar-load latency hides behind the test's VALU work (the
// field-by-field loads compiled to ~5 dependent s_load / s_waitcnt round
// trips per quad).  The two head registers ping-pong (no copy of the
// prefetched head per quad) and the walk is a pointer (2 SALU per prefetch
// address, not ~7 for a clamped index).  `cur` holds quad b's head on entry
// and quad e's (the next group's first: the groups are contiguous in scan
// order) on exit.
RTP_DEV u16v quad_head(const DevScene* __restrict__ sc, int q) {
  return reinterpret_cast<const u16v*>(sc->quads)[2 * min(q, kMaxQuads - 1)];
}
template <int K>
RTP_DEV void scan_one(const DevQuad& M, const u16v& head, f3 o, f3 d, uint64_t& best) {
  QuadGeom G;
  __builtin_memcpy(&G, &head, sizeof(G));
  float t;
  const bool ok = quad_hit_masked<K>(G, M, o, d, t);
  const uint64_t key = (uint64_t)__float_as_uint(t) << 32 | G.key_lo;
  best = (ok && t > 0.001f && key < best) ? key : best;
}
RTP_DEV u16v head_at(const DevQuad* q) { return *reinterpret_cast<const u16v*>(q); }
template <int K>
RTP_DEV void scan_kind_pf(const DevScene* __restrict__ sc, int b, int e, f3 o, f3 d, uint64_t& best, u16v& cur) {
  // (the prefetches read at most two records past quads[] -- still inside
  // DevScene, whose spheres[] follow -- and those values are never used)
  const DevQuad* qp = sc->quads + b;
  for (int n = e - b; n > 0; n -= 2, qp += 2) {
    const u16v nxt = head_at(qp + 1);
    scan_one<K>(qp[0], cur, o, d, best);
    if (n == 1) {
      cur = nxt;
      break;
    }
    cur = head_at(qp + 2);
    scan_one<K>(qp[1], nxt, o, d, best);
  }
}

// SphereLeafIntersector::hit's accepted root without the tmax test: the
// reference takes r1 = (-b-sq)/a if tmin < r1 < tmax, else r2 = (-b+sq)/a if
// tmin < r2 < tmax.  r1 <= r2 (a > 0), so r1 >= tmax rules out r2 too: the
// accepted root is "r1 if r1 > tmin else r2", accepted iff it is > tmin and
// < tmax.  It does not depend on tmax, so spheres may be visited in any order.
RTP_DEV bool sphere_root(f3 o, f3 d, float tmin, f3 c, float rr, float& t_out) {
  f3 oc = sub(o, c);
  float a = dot(d, d);
  float b = dot(oc, d);
  float cc = dot(oc, oc) - rr;
  float disc = b * b - a * cc;
  if (!(disc > 0)) return false;
  float sq = sqrt_exact(b * b - a * cc);
  float r1 = (-b - sq) / a;
  float t = r1 > tmin ? r1 : (-b + sq) / a;
  t_out = t;
  return t > tmin;
}

// Threaded-BVH walk over the spheres (scenes with >= kBvhMinSpheres).  The
// brute-force scan in index order with a strict '<' returns the
// lexicographic minimum of (t, quads before spheres, sphere index); the walk
// visits spheres in BVH order and keeps that minimum explicitly.  Node boxes
// only cull (padded on the host; compared with slack here), so no sphere
// whose root could win is skipped.  (Loading node i+1 while testing i was
// faster with flat loads and 16% slower with global ones: DESIGN.md 4.1.)
typedef float f4v __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) f4v GF4;
typedef uint32_t u4v __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) u4v GU4;
typedef const __attribute__((address_space(1))) int32_t GI32;
// 1/d per component for the slab tests (tiny components clamped)
RTP_DEV float slab_rcp(float v) { return __builtin_amdgcn_rcpf(fabsf(v) < 1e-20f ? copysignf(1e-20f, v) : v); }
// A ray's view of the sphere BVH: the compact copy of the tree ordered
// near-to-far for its direction octant (rtp_layout.hpp kCBvhSphereBit) and
// that copy's sphere-index table.  (Global, address space 1, pointers: through
// the generic ones loaded from the scene the walk compiled to flat loads.)
// The slab test runs as fma(box, 1/d, -o/d): one rounding of o/d per
// component instead of a rounded (box - o) per face.  The boxes only cull,
// and each sphere lies at least the builders' pad inside its boxes on every
// axis (rtp_layout.hpp bvh_sphere_pad).  Its first part, 0.002 r + 1e-5 +
// 2^-16 (|c| + r), is this test's: a ray through a sphere crosses every box
// around it over a parameter interval 2 pad / |d| wider than the sphere's,
// far above these roundings (2^-24 |o| / |d|).  Its second part covers what
// sphere_root accepts beyond the exact sphere (its discriminant's roundings).
struct BvhRay {
  GU4* nodes;
  GI32* cidx;
  GI32* orig;           // LDS walk: the scene index of a leaf-order sphere position (kind 3 hits)
  float ix, iy, iz;     // 1/d (clamped)
  float ox, oy, oz;     // -o/d
};
RTP_DEV int ray_octant(f3 d) { return (d.x < 0.f ? 1 : 0) | (d.y < 0.f ? 2 : 0) | (d.z < 0.f ? 4 : 0); }
// kLds: the LDS walk's tree (its global side tables; the nodes are read from LDS)
template <bool kLds = false>
RTP_DEV BvhRay bvh_ray(const DevScene* __restrict__ sc, f3 o, f3 d) {
  const int oct = ray_octant(d) & (kLds ? 7 : sc->oct_mask);
  const int64_t base = (int64_t)oct * (kLds ? sc->n_lw_nodes : sc->n_nodes);
  BvhRay R;
  R.nodes = (GU4*)((kLds ? sc->lw_nodes : sc->cnodes) + 4 * base);
  R.cidx = (GI32*)((kLds ? sc->lw_cidx : sc->cidx) + base);
  R.orig = (GI32*)sc->lw_orig;
  R.ix = slab_rcp(d.x);
  R.iy = slab_rcp(d.y);
  R.iz = slab_rcp(d.z);
  R.ox = -(o.x * R.ix);
  R.oy = -(o.y * R.iy);
  R.oz = -(o.z * R.iz);
  return R;
}
// During a walk a sphere hit is h.kind == 2 with h.idx the leaf's node (the
// sphere's scene index is cidx[node]), or, in the LDS walk's multi-sphere
// leaves, h.kind == 3 with h.idx the sphere's leaf-order position (scene index
// orig[pos]); bvh_resolve turns either into kind 1 with the scene index.
// Kind 1 hits (the global walk's multi-sphere leaves) carry the index.
RTP_DEV int bvh_hit_index(const Hit& h, const BvhRay& R) {
  return h.kind == 2 ? R.cidx[h.idx] : h.kind == 3 ? R.orig[h.idx] : h.idx;
}
RTP_DEV void bvh_resolve(Hit& h, const BvhRay& R) {
  if (h.kind >= 2) {
    h.idx = bvh_hit_index(h, R);
    h.kind = 1;
  }
}
// the closest-sphere update: the (t, scene index) minimum, quads winning t
// ties; `ref` is the hit's kind-`kind` reference, `orig` reads its scene index
// (only for an exact tie between spheres: rare)
template <class Orig>
RTP_DEV void bvh_accept(Hit& h, float t, int kind, int ref, const BvhRay& R, Orig orig) {
  if (t < h.t) {
    h.t = t;
    h.kind = kind;
    h.idx = ref;
  } else if (t == h.t && h.kind >= 1) {
    if (orig() < bvh_hit_index(h, R)) {
      h.kind = kind;
      h.idx = ref;
    }
  }
}
RTP_DEV float half_lo(uint32_t v) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(v & 0xffffu)); }
RTP_DEV float half_hi(uint32_t v) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(v >> 16)); }
// One node of the walk: node ni (its 16 bytes v) is tested against the ray
// and the best hit so far; returns the next node (>= n_nodes: the walk is
// done).  A sphere leaf runs the exact root test (no box); an inner node's
// box (padded on the host, rounded outward to half precision, compared with
// slack here) only culls.
// kLds: the LDS walk (rtp_render_pool_lds): a multi-sphere leaf's spheres
// are (centre, r^2) float4s in the block's LDS (lsph), else 32-byte
// DevSphereG records in global memory (geom_g).
typedef const __attribute__((address_space(3))) f4v LF4;
typedef const __attribute__((address_space(3))) u4v LU4;
template <bool kLds = false>
RTP_DEV int bvh_visit(GF4* __restrict__ geom_g, LF4* __restrict__ lsph, const BvhRay& R, f3 o, f3 d, u4v v, int ni,
                      Hit& h) {
  if ((int32_t)v.w < 0) {  // a sphere leaf: centre, r^2
    float t;
    if (sphere_root(o, d, 0.001f, mk(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z)),
                    __uint_as_float(v.w & ~kCBvhSphereBit), t))
      bvh_accept(h, t, 2, ni, R, [&] { return R.cidx[ni]; });
    return ni + 1;
  }
  const float x0 = __builtin_fmaf(half_lo(v.x), R.ix, R.ox), x1 = __builtin_fmaf(half_hi(v.y), R.ix, R.ox);
  const float y0 = __builtin_fmaf(half_hi(v.x), R.iy, R.oy), y1 = __builtin_fmaf(half_lo(v.z), R.iy, R.oy);
  const float z0 = __builtin_fmaf(half_lo(v.y), R.iz, R.oz), z1 = __builtin_fmaf(half_hi(v.z), R.iz, R.oz);
  const float tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
  const float tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
  const float slack = 1e-5f * fabsf(tf) + 1e-7f;
  const bool hit = tn <= tf + slack && tf >= 0.0f && tn <= h.t * 1.00001f + 1e-7f;
  const bool leaf = (v.w & kCBvhLeafBit) != 0;
  if (hit && leaf) {  // a multi-sphere leaf: its spheres in leaf order
    const int first = (int)((v.w & ~kCBvhLeafBit) >> 3), cnt = (int)(v.w & 7u);
    for (int j = first; j < first + cnt; j++) {
      float t;
      if constexpr (kLds) {
        const f4v g0 = lsph[j];  // c, rr
        if (sphere_root(o, d, 0.001f, mk(g0.x, g0.y, g0.z), g0.w, t)) bvh_accept(h, t, 3, j, R, [&] { return R.orig[j]; });
      } else {
        const f4v g0 = geom_g[2 * j], g1 = geom_g[2 * j + 1];  // c, rr | orig
        if (sphere_root(o, d, 0.001f, mk(g0.x, g0.y, g0.z), g0.w, t))
          bvh_accept(h, t, 1, __float_as_int(g1.x), R, [&] { return __float_as_int(g1.x); });
      }
    }
  }
  return (hit || leaf) ? ni + 1 : (int)v.w;
}
// Threaded-BVH walk over the spheres (scenes with >= kBvhMinSpheres).  The
// brute-force scan in index order with a strict '<' returns the
// lexicographic minimum of (t, quads before spheres, sphere index); the walk
// visits spheres in BVH order and keeps that minimum explicitly, so no
// sphere whose root could win is skipped and the order does not matter.
RTP_DEV void spheres_bvh(const DevScene* __restrict__ sc, f3 o, f3 d, Hit& h) {
  const BvhRay R = bvh_ray(sc, o, d);
  const int nn = sc->n_nodes;
  GF4* __restrict__ geom_g = (GF4*)sc->sph_geom;  // DevSphereG: 2 x 16 B
  int ni = 0;
  u4v v = R.nodes[0];
  while (ni < nn) {
    const int next = bvh_visit(geom_g, nullptr, R, o, d, v, ni, h);
    if (next < nn) v = R.nodes[next];
    ni = next;
  }
  bvh_resolve(h, R);
}

// ---------------------------------------------------------- mesh scenes ---
// Mesh scenes (rtp_set_scene_mesh): the quads lie in global memory in the
// leaf order of a threaded BVH (rtp_layout.hpp DevScene::mesh_nodes), the
// spheres (at most kBvhMinSpheres - 1) inline.  The closest hit is the
// scan's: the minimum of (t, quads before spheres, index in the caller's
// list).  Every quad runs the general test, quad_hit_masked<0>, on a per-lane
// copy of its 64-byte scan head (4 x 16-byte loads); the e21 / e23 tail is
// read from memory only by lanes whose quad is no exact parallelogram and
// whose alpha + beta > 1.  By the zero-structure argument of rtp_device.hpp
// the general test equals the kind-specific ones on finite rays.
// A triangle cell (kind == kMeshKindTri: v11 == v01, so e23 == 0) is the
// first triangle alone: where alpha + beta > 1 the general test's second
// branch computes detp = e23 . Pp = 0 and rejects (rtp_layout.hpp kMeshCosMin,
// "Triangle cells").  mesh_tri_hit is the first-triangle arithmetic of
// quad_hit_masked<0>'s general path, the same products and sums in the same
// order, and that rejection without the gather of the e21 / e23 tail.
RTP_DEV bool mesh_tri_hit(const QuadGeom& Q, f3 o, f3 d, float& t_out) {
  const float dv[3] = {d.x, d.y, d.z};
  const float P[3] = {cross_c<7, 0>(dv, Q.e03), cross_c<7, 1>(dv, Q.e03), cross_c<7, 2>(dv, Q.e03)};
  const float det = dot_m<7>(Q.e01, P);
  const float inv_det = rcp_det(det);
  const float T[3] = {o.x - Q.vv[0][0], o.y - Q.vv[1][0], o.z - Q.vv[2][0]};
  const float alpha = dot_m<7>(T, P) * inv_det;
  const float Qv[3] = {cross_c<7, 0>(T, Q.e01), cross_c<7, 1>(T, Q.e01), cross_c<7, 2>(T, Q.e01)};
  const float beta = dot_m<7>(dv, Qv) * inv_det;
  const float t = dot_m<7>(Q.e03, Qv) * inv_det;
  t_out = t;
  return !(fabsf(det) < kEps) && !(alpha < 0.0f) && !(beta < 0.0f) && !(t < 0.0f) && !((alpha + beta) > 1.0f);
}
// One quad (leaf-order position j) against the closest hit so far; h.kind is
// -1 (none), 0 (a quad, h.idx its caller's index) or 1 (an inline sphere).
RTP_DEV void mesh_quad_test(GF4* __restrict__ quads, int j, f3 o, f3 d, Hit& h) {
  GF4* q = quads + 8 * (int64_t)j;  // DevQuad: 8 x 16 B
  const f4v hd[4] = {q[0], q[1], q[2], q[3]};
  QuadGeom G;
  __builtin_memcpy(&G, hd, sizeof(G));
  float t;
#if RTP_MESH_TRI_TEST
  const bool ok = G.kind == kMeshKindTri
                      ? mesh_tri_hit(G, o, d, t)
                      : quad_hit_masked<0>(G, *reinterpret_cast<const DevQuad*>((const f4v*)q), o, d, t);
#else
  const bool ok = quad_hit_masked<0>(G, *reinterpret_cast<const DevQuad*>((const f4v*)q), o, d, t);
#endif
  const int idx = (int)G.key_lo;
  if (ok && t > 0.001f && (t < h.t || (t == h.t && (h.kind == 1 || (h.kind == 0 && idx < h.idx))))) {
    h.t = t;
    h.kind = 0;
    h.idx = idx;
  }
}
// the inline spheres of a mesh scene, in index order with a strict '<': the
// start of a ray's search (a quad at the same t wins in mesh_quad_test)
RTP_DEV Hit mesh_spheres(const DevScene* __restrict__ sc, f3 o, f3 d) {
  Hit h{3.40282347e+38f, -1, 0};
  const int ns = sc->n_spheres;
  for (int k = 0; k < ns; k++) {
    const DevSphere& S = sc->spheres[k];
    float t;
    if (sphere_hit(o, d, 0.001f, h.t, ld3(S.c), S.rr, t)) {
      h.t = t;
      h.kind = 1;
      h.idx = k;
    }
  }
  return h;
}
// A ray's view of the mesh BVH: its octant's near-to-far copy and the slab
// test's constants (BvhRay's).
struct MeshRay {
  GU4* nodes;
  float ix, iy, iz;
  float ox, oy, oz;
};
RTP_DEV MeshRay mesh_ray(const DevScene* __restrict__ sc, f3 o, f3 d) {
  MeshRay R;
  R.nodes = (GU4*)(sc->mesh_nodes + 4 * ((int64_t)ray_octant(d) * sc->n_mesh_nodes));
  R.ix = slab_rcp(d.x);
  R.iy = slab_rcp(d.y);
  R.iz = slab_rcp(d.z);
  R.ox = -(o.x * R.ix);
  R.oy = -(o.y * R.iy);
  R.oz = -(o.z * R.iz);
  return R;
}
// One node of the mesh walk (bvh_visit's shape: the same slab test and cull;
// the boxes are padded on the host, rtp_layout.hpp kMeshCosMin): returns the
// next node (>= n_mesh_nodes: done).
RTP_DEV int mesh_visit(GF4* __restrict__ quads, const MeshRay& R, f3 o, f3 d, u4v v, int ni, Hit& h) {
  const float x0 = __builtin_fmaf(half_lo(v.x), R.ix, R.ox), x1 = __builtin_fmaf(half_hi(v.y), R.ix, R.ox);
  const float y0 = __builtin_fmaf(half_hi(v.x), R.iy, R.oy), y1 = __builtin_fmaf(half_lo(v.z), R.iy, R.oy);
  const float z0 = __builtin_fmaf(half_lo(v.y), R.iz, R.oz), z1 = __builtin_fmaf(half_hi(v.z), R.iz, R.oz);
  const float tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
  const float tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
  const float slack = 1e-5f * fabsf(tf) + 1e-7f;
  const bool hit = tn <= tf + slack && tf >= 0.0f && tn <= h.t * 1.00001f + 1e-7f;
  const bool leaf = (v.w & kCBvhLeafBit) != 0;
  if (hit && leaf) {
    const int first = (int)((v.w & ~kCBvhLeafBit) >> 3), cnt = (int)(v.w & 7u);
    for (int j = first; j < first + cnt; j++) mesh_quad_test(quads, j, o, d, h);
  }
  return (hit || leaf) ? ni + 1 : (int)v.w;
}
// The whole search of one ray (the diagnostics kernels; the pool kernel runs
// the same steps resumably): kScan: every quad in storage order instead of
// the walk -- the (t, index) minimum does not depend on the order, so this is
// the scan in index order with a strict '<'.
template <bool kScan>
RTP_DEV Hit closest_hit_mesh(const DevScene* __restrict__ sc, f3 o, f3 d) {
  Hit h = mesh_spheres(sc, o, d);
  GF4* __restrict__ quads = (GF4*)sc->mesh_quads;
  if constexpr (kScan) {
    const int nq = sc->n_mesh_quads;
    for (int j = 0; j < nq; j++) mesh_quad_test(quads, j, o, d, h);
  } else {
    const MeshRay R = mesh_ray(sc, o, d);
    const int nn = sc->n_mesh_nodes;
    int ni = 0;
    u4v v = R.nodes[0];
    while (ni < nn) {
      const int next = mesh_visit(quads, R, o, d, v, ni, h);
      if (next < nn) v = R.nodes[next];
      ni = next;
    }
  }
  return h;
}

// qshade: the block's LDS copy of the quads' shading data (n, alb, mt) so
// the hit's material is an LDS gather instead of a global one.
// Every quad of a scene (kMaxQuads, 8 KiB): with a table that could be
// absent, the compiler merged the LDS and global reads of the hit's record
// into 7 flat loads (waited on both counters); now they are 2 ds_read_b128.
constexpr int kLdsQuads = kMaxQuads, kQShadeFloats = 8;  // per quad: n, alb, mt, pad
// The block's LDS table also holds the prefilter's PreExact records (after
// the shading data): the candidate's record is then 4 ds_read_b128 instead of
// 4 global loads (L2 hits) on every bounce's critical path (C2 kernel -1.7%,
// r03c; an LDS copy of the quads in round 1 had been slower).
constexpr int kPrexLdsOffset = kLdsQuads * kQShadeFloats;
constexpr int kQTableFloats = kPrexLdsOffset + kMaxPre * 16;

RTP_DEV void fill_qshade(const DevScene* __restrict__ sc, float* s_qshade) {
  for (int i = threadIdx.x; i < sc->n_quads * kQShadeFloats; i += blockDim.x) {
    const DevQuad& Q = sc->quads[i / kQShadeFloats];
    const int f = i % kQShadeFloats;
    s_qshade[i] = f < 3 ? Q.n[f] : f < 6 ? Q.alb[f - 3] : f == 6 ? __int_as_float(Q.mt) : 0.f;
  }
  const float* px = reinterpret_cast<const float*>(sc->prex);
  for (int i = threadIdx.x; i < sc->n_pre * 16; i += blockDim.x) s_qshade[kPrexLdsOffset + i] = px[i];
}

// Closest-hit prefilter over the axis-plane quads (kinds 1..6).
// The exact Lagae-Dutre test costs ~40 VALU per quad and every quad meets
// some lane of a wave, so the scan paid it for all of them.  The prefilter
// instead takes, per quad, the ray's parameter at the quad's plane and the
// hit point's distance outside the quad's box, both in a few ops, with an
// error margin m >= the difference between these approximations and the
// exact test's own roundings:
//   m = 2^-18 * (|t| * max(max|d|, 1) + max|o| + scene scale + 1),
// about six times the worst case of either computation (a handful of
// roundings each of |t*d|, |o| and the vertex coordinates).
// A quad the exact test accepts (0.001 < t, inside) is therefore a
// candidate, and t - m is a lower bound of its exact t.  Each lane keeps its
// two smallest lower bounds, runs the exact test on the first (quad_hit_axis
// on the quad's PreExact record, a per-lane load from the small global prex
// table: the kind's own parallelogram arithmetic in the quad's axes, bit-equal
// to it), and is done when the second lower bound exceeds the best exact hit:
// every other candidate's exact t is larger, so it loses whatever its index.
// Otherwise -- near an edge, a near tie, no finite ray, coordinates beyond
// kPreLim -- the lane runs the exact scan of every axis-plane quad, as
// without the prefilter.  (The host disables the prefilter for scenes it
// does not cover, and with RTP_PREFILTER=0: DevScene::n_pre == 0.)
constexpr float kPreTmin = 0.0005f;  // candidates: approximate t above this (accepted hits: t > 0.001)
constexpr float kPreLimD = 16.0f;    // larger |o| or |d| components: exact scan (margin bound below tmin)
constexpr float kPreK = 0x1p-18f;    // margin factor, 64 units of 2^-24
template <int A>
RTP_DEV float comp(f3 v) {
  if constexpr (A == 0) return v.x;
  else if constexpr (A == 1) return v.y;
  else return v.z;
}
// k1 <= k2: the two smallest candidate keys {bits(t - m) & ~31, quad position}
// (positive floats order like their bit patterns; rounding the low bits
// down keeps the lower bound).  No candidate: ~0u.
// Each PreQuad is one s_load_dwordx8, the next one's issued before the
// current one is tested (as scan_kind_pf); `cur` carries quad b's record in
// and quad e's (the next axis group's first) out.  v_and_or_b32 / v_med3_u32
// are inline asm: the compiler emits 2 + 2 ops for them, which left the
// prefilter at break-even.
typedef uint32_t u8v __attribute__((ext_vector_type(8)));
RTP_DEV u8v pre_rec(const DevScene* __restrict__ sc, int i) {
  return reinterpret_cast<const u8v*>(sc->pre)[min(i, kMaxPre - 1)];
}
template <int A>
RTP_DEV void pre_axis(const DevScene* __restrict__ sc, int b, int e, f3 o, f3 d, float ma, float mb, uint32_t& k1,
                      uint32_t& k2, u8v& cur) {
  constexpr int B = (A + 1) % 3, C = (A + 2) % 3;
  if (b == e) return;
  const float inv = __builtin_amdgcn_rcpf(comp<A>(d));
  const float oa = comp<A>(o);
  const f2v obc = f2v{comp<B>(o), comp<C>(o)}, dbc = f2v{comp<B>(d), comp<C>(d)};
  // the candidate key of one quad (~0u: not a candidate)
  auto key_of = [&](const PreQuad& P) -> uint32_t {
    const float t = (P.x - oa) * inv;
    // the two in-plane coordinates as one packed FMA and one packed subtract
    const f2v u = __builtin_elementwise_fma(f2v{t, t}, dbc, obc) - f2v{P.cb, P.cc};
    const float ub = fabsf(u.x) - P.rb, uc = fabsf(u.y) - P.rc;
    const float m = __builtin_fmaf(fabsf(t), ma, mb);
    // t = +-inf (d[A] ~ 0) gives NaN or inf here and at worst a key above
    // every finite one; the exact test rejects such a quad (|det| < eps)
    const bool ok = (fmaxf(ub, uc) <= m) & (t > kPreTmin);
    uint32_t key;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(key) : "v"(__float_as_uint(t - m)), "v"(~31u), "s"((uint32_t)P.qpos));
    return ok ? key : ~0u;
  };
  auto fold = [&](uint32_t key) {  // keep the two smallest keys
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(k2) : "v"(k1), "v"(k2), "v"(key));
    k1 = min(k1, key);
  };
  // ping-pong heads, pointer walk (as scan_kind_pf; prefetches past pre[]
  // stay inside DevScene: prex[] follows)
  auto as_pre = [](const u8v& v) {
    PreQuad P;
    __builtin_memcpy(&P, &v, sizeof(P));
    return P;
  };
  const PreQuad* pq = sc->pre + b;
  for (int n = e - b; n > 0; n -= 2, pq += 2) {
    const u8v nxt = *reinterpret_cast<const u8v*>(pq + 1);
    fold(key_of(as_pre(cur)));
    if (n == 1) {
      cur = nxt;
      break;
    }
    cur = *reinterpret_cast<const u8v*>(pq + 2);
    fold(key_of(as_pre(nxt)));
  }
}

// quad_hit_masked<K>'s parallelogram path for an axis-plane quad of any of
// the kinds 1..6, the kind chosen per lane: the same products, sums and
// signs (derived in DESIGN.md 4.1), on o and d permuted into the quad's axes.
RTP_DEV bool quad_hit_axis(const PreExact& E, f3 o, f3 d, float& t_out) {
  const bool x0 = E.i == 0, x1 = E.i == 1, pos = E.s > 0;
  auto perm = [&](f3 v, float& vi, float& va, float& vj) {
    const float r0 = x0 ? v.x : (x1 ? v.y : v.z);
    const float r1 = x0 ? v.y : (x1 ? v.z : v.x);
    const float r2 = x0 ? v.z : (x1 ? v.x : v.y);
    vi = r0;
    vj = pos ? r1 : r2;
    va = pos ? r2 : r1;
  };
  float oi, oa, oj, di, da, dj;
  perm(o, oi, oa, oj);
  perm(d, di, da, dj);
  const float Pa = di * E.cs;     // s * d_i c
  const float Pi = -(da * E.cs);  // -s * d_a c
  const float det = E.b * Pi;
  const float inv_det = rcp_det(det);
  const f2v Ta = f2v{oa, oa} - f2v{E.va, E.wa};
  const f2v Ti = f2v{oi, oi} - f2v{E.vi, E.wi};
  const f2v Tj = f2v{oj, oj} - f2v{E.vj, E.wj};
  const f2v al2 = (Ti * Pi + Ta * Pa) * inv_det;  // (alpha, -ap)
  const f2v Qj = Ta * E.bs;                       // s * T_a b
  const f2v Qa = -(Tj * E.bs);                    // -s * T_j b
  const f2v be2 = (f2v{dj, dj} * Qj + f2v{da, da} * Qa) * inv_det;  // (beta, -bp)
  const float t = (E.c * Qj.x) * inv_det;
  const bool ok1 = !(fabsf(det) < kEps) & !(fminf(fminf(al2.x, be2.x), t) < 0.0f);  // (see quad_hit_masked)
  const bool second = (al2.x + be2.x) > 1.0f;
  const bool bad2 = (al2.y > 0.0f) | (be2.y > 0.0f);
  t_out = t;
  return ok1 & !(second & bad2);
}

// kSpheres = false: the quads only (the pool kernel's resumable sphere-BVH
// walk, spheres_bvh_step, continues from the quads' hit).
template <bool kBvh, bool kSpheres = true>
RTP_DEV Hit closest_hit(const DevScene* __restrict__ sc, f3 o, f3 d, bool prefilter,
                        uint32_t* full_out, const float* lds_prex) {
  Hit h{3.40282347e+38f, -1, 0};
  const float tmin = 0.001f;
  // the (t, orig) key minimum: the order the kinds are scanned in is free
  uint64_t key = kNoHitKey;
  bool full = true;  // this lane needs the exact scan of the axis-plane quads (kinds 1..6)
  const bool pre = prefilter && sc->n_pre > 0;  // wave-uniform
  {  // kinds 7..10 and 0: the exact scan, always (their keys are final)
    const int g6 = sc->kind_begin[6], g7 = sc->kind_begin[7], g8 = sc->kind_begin[8], g9 = sc->kind_begin[9],
              g10 = sc->kind_begin[10], g11 = sc->kind_begin[11];
    u16v cur = quad_head(sc, g6);
    scan_kind_pf<7>(sc, g6, g7, o, d, key, cur);
    scan_kind_pf<8>(sc, g7, g8, o, d, key, cur);
    scan_kind_pf<9>(sc, g8, g9, o, d, key, cur);
    scan_kind_pf<10>(sc, g9, g10, o, d, key, cur);
    scan_kind_pf<0>(sc, g10, g11, o, d, key, cur);
  }
  if (pre) {
    const bool lane_ok = (int)(fabsf(o.x) <= kPreLimD) & (int)(fabsf(o.y) <= kPreLimD) &
                         (int)(fabsf(o.z) <= kPreLimD) & (int)(fabsf(d.x) <= kPreLimD) &
                         (int)(fabsf(d.y) <= kPreLimD) & (int)(fabsf(d.z) <= kPreLimD);
    const float dmax = fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fmaxf(fabsf(d.z), 1.0f));
    const float omax = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
    const float ma = kPreK * dmax, mb = kPreK * (omax + (sc->pre_scale + 1.0f));
    uint32_t k1 = ~0u, k2 = ~0u;
    const int p0 = sc->pre_begin[0], p1 = sc->pre_begin[1], p2 = sc->pre_begin[2], p3 = sc->pre_begin[3];
    u8v pcur = pre_rec(sc, p0);
    pre_axis<0>(sc, p0, p1, o, d, ma, mb, k1, k2, pcur);
    pre_axis<1>(sc, p1, p2, o, d, ma, mb, k1, k2, pcur);
    pre_axis<2>(sc, p2, p3, o, d, ma, mb, k1, k2, pcur);
    // the candidate's PreExact record from the block's LDS table: four
    // 16-byte reads issued together (every lane: k1 = ~0u reads record 31,
    // in bounds, unused)
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v* lx = reinterpret_cast<const f4v*>(lds_prex) + 4 * (k1 & 31u);
    f4v xr[4] = {lx[0], lx[1], lx[2], lx[3]};
    static_assert(sizeof(PreExact) == sizeof(xr), "PreExact is four 16-byte loads");
    if (lane_ok && k1 != ~0u) {  // (finite o, d: the generic arithmetic equals the kind's)
      PreExact Q;
      __builtin_memcpy(&Q, xr, sizeof(Q));
      float t;
      const bool ok = quad_hit_axis(Q, o, d, t);
      const uint64_t kq = (uint64_t)__float_as_uint(t) << 32 | Q.key_lo;
      key = (ok && t > 0.001f && kq < key) ? kq : key;
    }
    full = !lane_ok || (k2 & ~31u) <= (uint32_t)(key >> 32);  // k2 = ~0u (none) never is
  }
  if (full_out) *full_out = !pre ? 2u : full ? 1u : 0u;  // 2: prefilter off for this scene
  if (__ballot(full)) {
    if (full) {
      const int g0 = sc->kind_begin[0], g1 = sc->kind_begin[1], g2 = sc->kind_begin[2], g3 = sc->kind_begin[3],
                g4 = sc->kind_begin[4], g5 = sc->kind_begin[5], g6 = sc->kind_begin[6];
      u16v cur = quad_head(sc, g0);
      scan_kind_pf<1>(sc, g0, g1, o, d, key, cur);
      scan_kind_pf<2>(sc, g1, g2, o, d, key, cur);
      scan_kind_pf<3>(sc, g2, g3, o, d, key, cur);
      scan_kind_pf<4>(sc, g3, g4, o, d, key, cur);
      scan_kind_pf<5>(sc, g4, g5, o, d, key, cur);
      scan_kind_pf<6>(sc, g5, g6, o, d, key, cur);
    }
  }
  if (key != kNoHitKey) {
    h.t = __uint_as_float((uint32_t)(key >> 32));
    h.kind = 0;
    h.idx = (int)(key & 0xffu);
  }
  static_assert(kQuadKinds == 11, "closest_hit scans every kind");
  if constexpr (!kSpheres) {
  } else if constexpr (kBvh) {
    spheres_bvh(sc, o, d, h);
  } else {
    const int ns = sc->n_spheres;
    for (int k = 0; k < ns; k++) {
      const DevSphere& S = sc->spheres[k];
      float t;
      if (sphere_hit(o, d, tmin, h.t, ld3(S.c), S.rr, t)) {
        h.t = t;
        h.kind = 1;
        h.idx = k;
      }
    }
  }
  return h;
}

// Camera::RayGen (Camera.cxx:482-524): 2 draws, jittered direction
// (camera_ray_at: the same ray for given jitter values ru, rv -- the first-hit
// guides take the pixel centre, 0.5f twice, and touch no RNG)
template <class Cam>  // DevCamera, or one read through an address-space-4 (kernarg) reference
RTP_DEV f3 camera_ray_at(const Cam& cam, int pi, int pj, int nx, int ny, float ru, float rv) {
  f3 rd = add(add(ld3(cam.nlook), scl(ld3(cam.dx), ((2.f * ((float)pi + (1.f - ru)) - (float)nx) / 2.0f))),
              scl(ld3(cam.dy), ((2.f * ((float)pj + rv) - (float)ny) / 2.0f)));
  if (rd.x == 0.f) rd.x += 0.0000001f;
  if (rd.y == 0.f) rd.y += 0.0000001f;
  if (rd.z == 0.f) rd.z += 0.0000001f;
  float sq_mag = __builtin_sqrtf(dot(rd, rd));
  // rd.x / sq_mag, ... as Markstein divisions by one reciprocal: rd =
  // nlook + a*dx + b*dy with dx, dy orthogonal to the unit nlook (Camera.cxx:
  // 437-474), so sq_mag is >= ~1 and at most ~|tan(fov/2)| + 1 < 2^26 for fov
  // <= 180: inside rcp_nr1's exact range [2^-40, 2^40]; each |component| is
  // <= sq_mag and >= 1e-7 (the zero fix above), so no quotient or remainder
  // under- or overflows.
  const float r = rcp_nr1(sq_mag);
  return mk(div_markstein(rd.x, sq_mag, r), div_markstein(rd.y, sq_mag, r), div_markstein(rd.z, sq_mag, r));
}
template <class Cam>
RTP_DEV f3 camera_ray(const Cam& cam, int pi, int pj, int nx, int ny, uint32_t& seed) {
  const float ru = randf(seed);
  const float rv = randf(seed);
  return camera_ray_at(cam, pi, pj, nx, ny, ru, rv);
}

struct Path {
  f3 org, dir;
  int d;           // current depth (the path is alive at the start of depth d)
  bool nonfinite;  // some stored A[d'] (d' <= D-2) is +-Inf or NaN
};

enum BounceResult { kAlive = 0, kMissed = 1, kLight = 2 };

// One depth for a ray that is alive at its start:
// intersect, collect, material, generate, pdfs, scatter.  Advances the RNG by
// exactly the reference's draws for this depth and stores A[d] at hist_d
// (when d <= D-2).  On kLight, `emit` receives E[d].
RTP_DEV unsigned long long stamp(bool on) { return on ? __builtin_amdgcn_s_memtime() : 0ull; }
// Stats build only (RTP_DEBUG_STATS=1): counters updated from divergent code
// go straight to the wave's record in global memory (gdbg = p.dbg + wave *
// kDbgCounters, zeroed before the launch), from its first active lane.
// dbg_region: one visit and the lanes active at the region's start;
// dbg_add: the sum of v over the active lanes.
RTP_DEV void dbg_region(unsigned long long* gdbg, int c) {
  const uint64_t m = __ballot(true);
  if ((int)(threadIdx.x & 63) == (int)__builtin_ctzll(m)) {
    atomicAdd(gdbg + c, 1ull);
    atomicAdd(gdbg + c + 1, (unsigned long long)__popcll(m));
  }
}
RTP_DEV void dbg_add(unsigned long long* gdbg, int c, unsigned long long v) { atomicAdd(gdbg + c, v); }

// kDeferDead: a path that misses or hits the light at depth k leaves its
// depth-k draws (which + generator, exactly one dead step) to the caller's
// fast-forward instead of drawing them here.
// qshade: the block's LDS quad table (fill_qshade).
// kMesh: a mesh scene (a quad hit's record comes from DevScene::mesh_shade).
template <bool kBvh, bool kDeferDead, bool kMesh = false>
RTP_DEV int shade_hit(const DevScene* __restrict__ sc, Path& ps, uint32_t& seed, f3& emit, float4* __restrict__ hist_d,
                      int D, const float* qshade, const Hit h, unsigned long long* dbg = nullptr);
template <bool kBvh, bool kDeferDead = false>
RTP_DEV int bounce(const DevScene* __restrict__ sc, Path& ps, uint32_t& seed, f3& emit, float4* __restrict__ hist_d,
                   int D, unsigned long long* dbg, const float* qshade, unsigned long long* gdbg = nullptr) {
  const bool st = dbg != nullptr;
  const unsigned long long t0 = stamp(st);
  const f3 org = ps.org, dir = ps.dir;
  // intersect + CollectIntersecttWorklet (SurfaceWorklets.h:104-109)
  uint32_t fb = 0;  // (stats) 1: this lane ran the exact scan of the prefiltered quads
  Hit h = closest_hit<kBvh>(sc, org, dir, true, st ? &fb : nullptr, qshade + kPrexLdsOffset);
  if (st) {
    const unsigned long long m = __ballot(fb == 1u);
    dbg[kDbgFallbackSteps] += m ? 1 : 0;
    dbg[kDbgFallbackLanes] += (unsigned long long)__popcll(m);
  }
  if (gdbg) {  // (stats) lanes whose closest hit is one of the exact-scan quads (kinds 7..10, 0)
    const uint64_t mb = __ballot(h.kind == 0 && h.idx >= sc->kind_begin[6]);
    if ((int)(threadIdx.x & 63) == (int)__builtin_ctzll(__ballot(true))) {
      if (mb == 0) dbg_add(gdbg, kDbgBoxFreeSteps, 1ull);
      dbg_add(gdbg, kDbgBoxLanes, (unsigned long long)__popcll(mb));
    }
  }
  if (st) {
    const unsigned long long t1s = __builtin_amdgcn_s_memtime();
    dbg[kDbgCyclesIntersect] += t1s - t0;
  }
  return shade_hit<kBvh, kDeferDead>(sc, ps, seed, emit, hist_d, D, qshade, h, gdbg);
}

// The rest of one depth once the closest hit h is known: collect, material,
// generate, pdfs, scatter (bounce() above; the pool kernel's resumable
// sphere-BVH walk calls it directly for the lanes whose walk has finished).
// dbg (stats build only): the wave's global counter record (dbg_region).
template <bool kBvh, bool kDeferDead, bool kMesh>
RTP_DEV int shade_hit(const DevScene* __restrict__ sc, Path& ps, uint32_t& seed, f3& emit, float4* __restrict__ hist_d,
                      int D, const float* qshade, const Hit h, unsigned long long* dbg) {
  const uint32_t t1 = sc->which_t1, t2 = sc->which_t2;
  const DevLights& L = sc->light;
  const f3 org = ps.org, dir = ps.dir;
  const int d = ps.d;
  if (h.kind < 0) {
    if (!kDeferDead) seed = dead_step(seed, t1, t2);  // which + generator draws of the now-dead ray
    return kMissed;
  }
  if (dbg) dbg_region(dbg, kDbgHitVisits);
  f3 hp = add(org, scl(dir, h.t));
  f3 hn;
  int mt;
  f3 alb;
  if constexpr (kMesh) {
    if (h.kind == 0) {  // a mesh quad: its 32-byte record, a per-lane global gather (h.idx: the caller's index)
      GF4* r = (GF4*)sc->mesh_shade + 2 * (int64_t)h.idx;
      const f4v r0 = r[0], r1 = r[1];
      hn = mk(r0.x, r0.y, r0.z);
      alb = mk(r0.w, r1.x, r1.y);
      mt = __float_as_int(r1.z);
      if (dot(hn, dir) > 0.f) hn = neg(hn);  // Surface.h:184-185
    } else {
      const DevSphere& S = sc->spheres[h.idx];
      hn = mk((hp.x - S.c[0]) / S.r, (hp.y - S.c[1]) / S.r, (hp.z - S.c[2]) / S.r);
      mt = S.mt;
      alb = ld3(S.alb);
    }
  } else if (h.kind == 0) {
    // (an LDS table always: a global fallback here made the compiler read
    // both through one flat pointer)
    const float4* r = reinterpret_cast<const float4*>(qshade + h.idx * kQShadeFloats);  // 16-byte aligned
    const float4 r0 = r[0], r1 = r[1];
    hn = mk(r0.x, r0.y, r0.z);
    alb = mk(r0.w, r1.x, r1.y);
    mt = __float_as_int(r1.z);
    if (dot(hn, dir) > 0.f) hn = neg(hn);  // Surface.h:184-185
  } else {
    const DevSphere& S = kBvh ? sc->sph_all[h.idx] : sc->spheres[h.idx];
    hn = mk((hp.x - S.c[0]) / S.r, (hp.y - S.c[1]) / S.r, (hp.z - S.c[2]) / S.r);
    mt = S.mt;
    alb = ld3(S.alb);
  }
  // applyMaterials (EmitWorklet.h)
  if (mt == 1) {  // DiffuseLightWorklet: emit, path ends (status &= 0)
    if (dbg) dbg_region(dbg, kDbgLightVisits);
    emit = (dot(hn, dir) < 0.0f) ? alb : mk(0.f, 0.f, 0.f);
    if (!kDeferDead) seed = dead_step(seed, t1, t2);
    return kLight;
  }
  f3 atten;
  // The RNG draws of both scattering materials, taken together (one pass for
  // the dielectric and Lambertian lanes instead of one per branch): the
  // dielectric's own draw (DielectricWorklet, EmitWorklet.h), then for both
  // the which draw and the generator's 2 / 3 / 2 draws (PdfWorklet.h:20,
  // 63-213; a dielectric discards the direction: dead_step's advance) and
  // SpherePDFWorklet's discarded draw (no draw lies between the generator and
  // it: quad_pdf_value draws none).
  const bool glass = mt == 2;
  float rglass = 0.0f;
  if (glass) rglass = randf(seed);
  const uint32_t tw = wang(seed);  // which (PdfWorklet.h:20)
  seed = tw;
  const bool is_cos = tw < t1, is_quad = !is_cos && tw < t2;
  const float ra = randf(seed);
  const float rb = randf(seed);
  uint32_t s3 = seed;
  const float rc = randf(s3);
  seed = is_quad ? s3 : seed;
  (void)randf(seed);  // SpherePDFWorklet's discarded draw
  if (glass) {  // DielectricWorklet: specular
    const unsigned long long td0 = stamp(dbg != nullptr);
    if (dbg) dbg_region(dbg, kDbgDielVisits);
    f3 sd;
    dielectric_scatter(dir, hn, sc->ior, sc->ior_r0sq, sc->ior_inv, rglass, sd);
    atten = mk(1.f, 1.f, 1.f);
    ps.org = hp;
    ps.dir = sd;
    if (dbg) {
      const unsigned long long td1 = __builtin_amdgcn_s_memtime();
      if ((int)(threadIdx.x & 63) == (int)__builtin_ctzll(__ballot(true))) dbg_add(dbg, kDbgCyclesDiel, td1 - td0);
    }
  } else {  // LambertianWorklet
    const unsigned long long tg0 = stamp(dbg != nullptr);
    if (dbg) dbg_region(dbg, kDbgGenVisits);
    f3 gen;
    float sph_ctm = -1.0f;  // sqrt(1 - R^2/|c-hp|^2) when the generator made it (sphere_pdf_value reuses it)
    // The three generators as one branch-free pass.  Cosine (PdfWorklet.h:
    // 63-79) and light-sphere (:193-213) directions share the ONB, the
    // sincos of phi = 2*pi*r1 and local(); they differ in w, in which draw
    // is r1 (g++ evaluates the sphere generator's draws right to left), and
    // in z and the radial factor.  The light-quad point (:112-137) needs a
    // third draw, taken only by its lanes (drawn above).
    const f3 rp = mk(L.gx0 + ra * L.gdx, L.gy0 + rb * L.gdy, L.gz0 + rc * L.gdz);
    const f3 genq = sub(rp, hp);
    const f3 direction = sub(ld3(L.sc), hp);
    const float r1 = is_cos ? ra : rb, r2 = is_cos ? rb : ra;
    const f3 wdir = is_cos ? hn : direction;
    const Onb guvw = build_from_w(wdir);
    const float phi = (float)(2 * kPi * r1);
    float sphi, cphi;
    rtp_sincosf(phi, &sphi, &cphi);
    // cosine: z = sqrt(1-r2), x = (cos(phi)*2)*sqrt(r2); sphere: z = 1 + r2*(sqrt(1-R^2/d^2)-1),
    // x = cos(phi)*sqrt(1-z*z) (and (c*1)*s == c*s exactly)
    const float dist2 = dot(direction, direction);
    const float q = sqrt_exact(is_cos ? 1 - r2 : 1 - L.srr / dist2);
    sph_ctm = is_cos ? -1.0f : q;
    const float z = is_cos ? q : 1 + r2 * (q - 1);
    const float rad = sqrt_exact(is_cos ? r2 : 1 - z * z);
    const float m = is_cos ? 2.0f : 1.0f;
    const f3 gcs = de_nan(local(guvw, mk(cphi * m * rad, sphi * m * rad, z)));
    gen = is_quad ? genq : gcs;
    const unsigned long long tg1 = stamp(dbg != nullptr);
    // applyPDFs: QuadPDFWorklet, SpherePDFWorklet (1 discarded draw)
    const float weight = 0.5f;
    float sum = 0;
    // 1/|gen| once: QuadPDFWorklet's rmag and both unit_vector(gen) below
    const float rg = rmag(gen);
    sum += weight * quad_pdf_value(L, hp, gen, rg);
    sum += weight * sphere_pdf_value(L, hp, gen, sph_ctm);  // (its discarded draw: above)
    // PDFCosineWorklet (ScatterWorklet.h:96-112): mixture in double
    const f3 ug = scl(gen, rg);       // unit_vector(gen)
    const f3 w_hn = unit_vector(hn);  // build_from_w(hn).w (u and v are unused here)
    float cv;
    {
      float cosine = dot(ug, w_hn);
      cv = (cosine > 0) ? cos_over_pi(cosine) : 0.f;
    }
    double pdf_val = 0.5 * (double)sum + 0.5 * (double)cv;
    float sp;
    {
      float cosine = dot(hn, ug);
      sp = (cosine < 0) ? 0.f : cos_over_pi(cosine);
    }
    double sctr = (double)sp / pdf_val;
    atten = mk((float)(alb.x * sctr), (float)(alb.y * sctr), (float)(alb.z * sctr));
    ps.org = hp;
    ps.dir = gen;
    if (dbg) {  // (wave cycles: added once, by the first active lane)
      const unsigned long long tg2 = __builtin_amdgcn_s_memtime();
      if ((int)(threadIdx.x & 63) == (int)__builtin_ctzll(__ballot(true))) {
        dbg_add(dbg, kDbgCyclesGen, tg1 - tg0);
        dbg_add(dbg, kDbgCyclesPdf, tg2 - tg1);
      }
    }
  }
  if (d <= D - 2) {
    *hist_d = make_float4(atten.x, atten.y, atten.z, 0.f);
    ps.nonfinite |= !(__builtin_isfinite(atten.x) && __builtin_isfinite(atten.y) && __builtin_isfinite(atten.z));
  }
  return kAlive;
}

// Back-to-front radiance (MapperPathTracer.cxx:328-348) of a finished path:
// s = E[D-1]+0; s = A[d]*s; s = E[d]+s for d = D-2..0.  Depths after the end
// contribute A=1, E=0 exactly, so for a light hit at depth k this is
// s = E_k (+0), then s = 0 + A[d]*s for d = k-1..0; for any other ending it
// is +0, or NaN if some stored A was not finite (Inf*0 / NaN propagation).
RTP_DEV f3 path_radiance(int result, int k, f3 emit, bool nonfinite, const float4* __restrict__ hist,
                         int64_t stride) {
  if (result != kLight) {
    const float v = nonfinite ? __builtin_nanf("") : 0.0f;
    return mk(v, v, v);
  }
  float sx = emit.x + 0.0f, sy = emit.y + 0.0f, sz = emit.z + 0.0f;
  for (int dd = k - 1; dd >= 0; dd--) {
    float4 a = hist[(int64_t)dd * stride];
    sx = a.x * sx;
    sy = a.y * sy;
    sz = a.z * sz;
    sx = 0.0f + sx;
    sy = 0.0f + sy;
    sz = 0.0f + sz;
  }
  return mk(sx, sy, sz);
}

// a / b (0 <= a, 0 < b) from a float reciprocal, then one correction each
// way: exact where the estimate is off by at most one before the correction;
// the caller states the bound that makes it so.
RTP_DEV int rcp_quotient(int a, int b) {
  int q = (int)((float)a * __builtin_amdgcn_rcpf((float)b));
  q += (q + 1) * b <= a;
  q -= q * b > a;
  return q;
}
// Tile-deal entry k: row ty and column tx of its 16 x 16 tile among the
// frame's tiles (tile index ti < 2^24: rcp_quotient's bound); returns the
// pixel's place inside the tile, row-major.
template <class KP>
RTP_DEV int tile_of(const KP& p, int k, int& ty, int& tx) {
  const int ti = (k >> 8) * p.tile_world + p.tile_rank;
  ty = rcp_quotient(ti, p.tile_tx);
  tx = ti - ty * p.tile_tx;
  return k & 255;
}
// The pixel's column and row directly (refill): the tile deal gives them
// without forming the linear index; a pixel index is split by a float
// reciprocal quotient with one correction each way, exact while every index
// is below 2^24 (the estimate is then off by at most one), else by integer
// division (a wave-uniform branch).  The compiler's signed % and / cost ~40
// VALU per refill.
template <bool kTiles = false, class KP>
RTP_DEV void pixel_xy(const KP& p, int k, int& pi, int& pj) {
  if constexpr (kTiles) {
    int ty, tx;
    const int within = tile_of(p, k, ty, tx);
    pj = ty * 16 + (within >> 4);
    pi = tx * 16 + (within & 15);
  } else {
    const int u = (int)(p.pixel_ids ? p.pixel_ids[k] : p.pixel_begin + k);  // in [0, nx * ny)
    const int nx = p.nx;
    if ((int64_t)nx * p.ny <= (int64_t)1 << 24) {
      const int q = rcp_quotient(u, nx);
      pj = q;
      pi = u - q * nx;
    } else {
      pj = (int)((uint32_t)u / (uint32_t)nx);
      pi = u - pj * nx;
    }
  }
}
// the tile deal's linear pixel index (not through pixel_xy<true>: summed in
// another order, the stealing tile instances compiled to other code)
template <class KP>
RTP_DEV int64_t tile_pixel(const KP& p, int k) {
  int ty, tx;
  const int within = tile_of(p, k, ty, tx);
  return (int64_t)(ty * 16 + (within >> 4)) * p.nx + tx * 16 + (within & 15);
}
// kViews (batched views, KParams::views): entry k of the view-major list ->
// its view v = k / (nx*ny) and the pixel u = k % (nx*ny) inside it.  The same
// shape as above: a float reciprocal quotient with one correction each way
// while the launch has at most 2^22 entries, else integer division (a
// wave-uniform branch).  With k < 2^22 the product k * rcp(npv) carries a
// relative error below 1.5 * 2^-23 (v_rcp_f32: 1 ulp, the product's rounding:
// half an ulp; k and npv are exact floats), so the estimate is within
// 0.75 / npv < 1 of the real quotient for every npv >= 1 and its floor is off
// by at most one.  (At the other modes' 2^24 bound the error reaches 1 for
// npv = 3.)  Exact for every k < 2^31: (q + 1) * npv <= k + 2 * npv stays
// inside 32 bits on the float path, and the fallback divides integers.
template <class KP>
RTP_DEV void view_split(const KP& p, int k, int& v, int& u) {
  const int npv = p.nx * p.ny;  // (<= npix <= INT32_MAX: the host checks)
  if (p.npix <= (int64_t)1 << 22) {
    v = rcp_quotient(k, npv);
  } else {
    v = (int)((uint32_t)k / (uint32_t)npv);
  }
  u = k - v * npv;
}
// the pixel's column and row inside its view (pixel_xy's split of u)
template <class KP>
RTP_DEV void view_pixel_xy(const KP& p, int u, int& pi, int& pj) {
  const int nx = p.nx;
  if ((int64_t)nx * p.ny <= (int64_t)1 << 24) {
    pj = rcp_quotient(u, nx);
  } else {
    pj = (int)((uint32_t)u / (uint32_t)nx);
  }
  pi = u - pj * nx;
}
// the first seed of entry k: views[v].seed_base + u (each view an independent
// reference render, seeds[i] = i: MapperPathTracer.cxx:265-267)
template <class KP>
RTP_DEV uint32_t view_seed(const KP& p, int k) {
  int v, u;
  view_split(p, k, v, u);
  return p.views[v].seed_base + (uint32_t)u;
}

// kTiles: a separate kernel instance (rtp_render_tiles_device).  A runtime
// branch here changed the compiler's code for the whole scheduling loop of
// the other modes (+9% time), as other additions to the refill path did.
template <bool kTiles = false, class KP>
RTP_DEV int64_t pixel_of(const KP& p, int k) {  // k < npix <= INT32_MAX (launch() checks)
  if constexpr (kTiles) return tile_pixel(p, k);
  else return p.pixel_ids ? p.pixel_ids[k] : p.pixel_begin + k;
}


}  // namespace rtp
