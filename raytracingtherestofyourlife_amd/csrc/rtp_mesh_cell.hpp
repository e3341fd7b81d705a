// rtp_mesh_cell.hpp -- the arithmetic of one mesh cell, stated once for the
// host builder (rtp_mesh_host.cpp), the device builder (rtp_mesh_gpu.hip) and
// the inline scene's quads (rtp_scene_host.cpp): the float helpers whose results the
// two builders must share bit for bit, a cell's pad and padded box
// (rtp_layout.hpp kMeshCosMin has the derivation), its DevQuad record, and the
// outward rounding to half precision of the walks' compact nodes.
//
// Every function is host + device, as rtp_layout.hpp bvh_sphere_pad is.  All
// of it is compiled without contraction, and sqrt, sqrtf, fabs and the
// divisions are correctly rounded on both sides, so a value computed here is
// the same bits wherever it is computed.  The order of the operations is part
// of the contract: the records feed the reference's per-ray arithmetic.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rtp_layout.hpp"

#ifdef __HIP__
#define RTP_HD __attribute__((host)) __attribute__((device))
#else
#define RTP_HD
#endif

namespace rtp {

// ---------------------------------------------------------------- floats ---
RTP_HD inline uint32_t float_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
RTP_HD inline float bits_float(uint32_t b) { return __builtin_bit_cast(float, b); }
// a float as an unsigned key of the same order (atomic min / max apply), and back
RTP_HD inline uint32_t mesh_float_key(float f) {
  const uint32_t b = float_bits(f);
  return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
RTP_HD inline float mesh_key_float(uint32_t k) { return bits_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// std::min / std::max, the sign of a zero included
template <class T>
RTP_HD inline T min_of(T a, T b) {
  return (b < a) ? b : a;
}
template <class T>
RTP_HD inline T max_of(T a, T b) {
  return (a < b) ? b : a;
}
// std::nextafter(x, +inf) and (x, -inf) of a float that is not NaN
RTP_HD inline float next_up(float x) {
  const uint32_t b = float_bits(x);
  if ((b & 0x7fffffffu) == 0) return bits_float(1u);
  if (b == 0x7f800000u) return x;
  return bits_float((b & 0x80000000u) ? b - 1 : b + 1);
}
RTP_HD inline float next_down(float x) { return -next_up(-x); }
RTP_HD inline bool finite_f(float x) { return (float_bits(x) & 0x7f800000u) != 0x7f800000u; }
RTP_HD inline bool finite_d(double x) {
  return (__builtin_bit_cast(uint64_t, x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// f32 -> f16 bits rounded outward, the smallest half >= x (up) or the largest
// <= x: the nearest half, stepped toward +inf or -inf until its value (decoded
// as the walk decodes it) is on the right side of x; an infinity for a NaN.
RTP_HD inline uint32_t half_outward(float x, bool up) {
  uint32_t b = __builtin_bit_cast(uint16_t, (_Float16)x);
  for (int i = 0; i < 4; i++) {
    const float v = (float)__builtin_bit_cast(_Float16, (uint16_t)b);
    if (up ? v >= x : v <= x) return b;
    const bool neg = (b & 0x8000u) != 0, zero = (b & 0x7fffu) == 0;
    if (zero) b = up ? 0x0001u : 0x8001u;
    else if (up) b = neg ? b - 1 : b + 1;
    else b = neg ? b + 1 : b - 1;
  }
  return up ? 0x7c00u : 0xfc00u;
}

// ------------------------------------------------------------- 3-vectors ---
template <class T>
struct vec3 {
  T x, y, z;
};
using f3 = vec3<float>;
using d3 = vec3<double>;
template <class T>
RTP_HD inline vec3<T> sub(vec3<T> a, vec3<T> b) {
  return {a.x - b.x, a.y - b.y, a.z - b.z};
}
template <class T>
RTP_HD inline T dot(vec3<T> a, vec3<T> b) {
  return a.x * b.x + a.y * b.y + a.z * b.z;
}
template <class T>
RTP_HD inline vec3<T> cross(vec3<T> a, vec3<T> b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
RTP_HD inline double len(d3 a) { return sqrt(dot(a, a)); }
RTP_HD inline d3 to_double(f3 a) { return {a.x, a.y, a.z}; }
RTP_HD inline f3 load_f3(const float* p) { return {p[0], p[1], p[2]}; }

// ------------------------------------------------------------------ pads ---
// The scene's reach: kBvhReachFactor diagonals of its bounding box.
RTP_HD inline float scene_reach(const float lo[3], const float hi[3]) {
  const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
  return kBvhReachFactor * sqrtf(ex * ex + ey * ey + ez * ez);
}

// what both pads end with: the slab terms, the refusal of a pad beyond the reach, one step up
RTP_HD inline float finish_pad(double rounded, double reach, double amax) {
  const double slab = 1e-5 + 0x1p-16 * amax + 0x1p-18 * reach;
  const double pad = rounded / (double)kMeshCosMin + slab;
  if (!(pad < reach)) return kMeshHuge;
  return next_up((float)pad);
}

// The pad of one quad (v00 = q, v10 = r, v11 = s, v01 = t), in double:
// (kMeshRound reach / sine + h) / kMeshCosMin + the slab terms, or kMeshHuge
// for a strongly non-planar or degenerate quad (rtp_layout.hpp).
RTP_HD inline float quad_pad(d3 q, d3 r, d3 s, d3 t, double reach, double amax) {
  const d3 e01 = sub(r, q), e03 = sub(t, q), e21 = sub(r, s), e23 = sub(t, s);
  const d3 n1 = cross(e01, e03);
  const double A1 = len(n1), A2 = len(cross(e21, e23));
  const double l1 = len(e01) * len(e03), l2 = len(e21) * len(e23);
  if (!(A1 > 0) || !(A2 > 0) || !finite_d(A1) || !finite_d(A2)) return kMeshHuge;
  const double sine = min_of(A1 / l1, A2 / l2);
  if (!(sine >= kMeshMinSine)) return kMeshHuge;
  const double h = fabs(dot(sub(s, q), n1)) / A1;  // v11 off the first triangle's plane
  if (h > 0) {
    // the fold: v11's projection lies w beyond the diagonal (v10, v01), away from v00
    const d3 diag = sub(t, r);
    const d3 u1 = cross(n1, diag);
    const double lu = len(u1);
    if (!(lu > 0)) return kMeshHuge;
    const double side = dot(sub(q, r), u1) < 0 ? 1.0 : -1.0;  // u1 points away from v00
    const double w = side * dot(sub(s, r), u1) / lu;
    if (!(w > 0) || !(h / w < 0.5 * kMeshCosMin)) return kMeshHuge;
  }
  return finish_pad((double)kMeshRound * reach / sine + h, reach, amax);
}

// The pad of a triangle cell (v11 == v01: the reference's test accepts only
// its first triangle v00 = q, v10 = r, v01 = t): the roundings and the slab
// terms of quad_pad over the sine of the corner at v00 alone, no h and no fold
// (rtp_layout.hpp kMeshCosMin, "Triangle cells").
RTP_HD inline float tri_pad(d3 q, d3 r, d3 t, double reach, double amax) {
  const d3 e01 = sub(r, q), e03 = sub(t, q);
  const double A1 = len(cross(e01, e03));
  const double l1 = len(e01) * len(e03);
  if (!(A1 > 0) || !finite_d(A1)) return kMeshHuge;
  const double sine = A1 / l1;
  if (!(sine >= kMeshMinSine)) return kMeshHuge;
  return finish_pad((double)kMeshRound * reach / sine, reach, amax);
}

// ------------------------------------------------------------- a cell's box ---
// One cell's pad, padded box and box centre.  A triangle cell (v11 and v01
// compare equal, include/rtp_mesh.h) is bounded by its three vertices; a quad
// by its four and by v00 + e01 + e03 with the records' float edges.
struct MeshCellBox {
  float pad;  // kMeshHuge: the unbounded box
  float lo[3], hi[3], cen[3];
  bool tri;
};
RTP_HD inline MeshCellBox mesh_cell_box(f3 v00, f3 v10, f3 v11, f3 v01, float reach) {
  MeshCellBox c;
  c.tri = mesh_is_triangle(&v11.x, &v01.x);
  float mn[3], mx[3];
  for (int k = 0; k < 3; k++) {
    const float a = (&v00.x)[k], b = (&v10.x)[k], s = (&v11.x)[k], d = (&v01.x)[k];
    if (c.tri) {
      mn[k] = min_of(min_of(a, b), d);
      mx[k] = max_of(max_of(a, b), d);
      continue;
    }
    const float far = a + (b - a) + (d - a);
    mn[k] = min_of(min_of(min_of(a, b), min_of(s, d)), far);
    mx[k] = max_of(max_of(max_of(a, b), max_of(s, d)), far);
  }
  double amax = 0;
  for (int k = 0; k < 3; k++) amax = max_of(amax, (double)max_of(fabsf(mn[k]), fabsf(mx[k])));
  c.pad = c.tri ? tri_pad(to_double(v00), to_double(v10), to_double(v01), reach, amax)
                : quad_pad(to_double(v00), to_double(v10), to_double(v11), to_double(v01), reach, amax);
  for (int k = 0; k < 3; k++) {
    // (one step outward: the float sums may round toward the cell)
    c.lo[k] = next_down(mn[k] - c.pad);
    c.hi[k] = next_up(mx[k] + c.pad);
    c.cen[k] = 0.5f * mn[k] + 0.5f * mx[k];
  }
  return c;
}

// ---------------------------------------------------------- a cell's record ---
// What a DevQuad holds of the geometry (v00 = q, v10 = r, v11 = s, v01 = t),
// with the reference's float operations in its order.
struct MeshCellRecord {
  f3 e01, e03, e21, e23;  // e01 = v10 - v00, e03 = v01 - v00, e21 = v10 - v11, e23 = v01 - v11
  f3 n;                   // Normalize(TriangleNormal(q, r, s)), Surface.h:182-183, unflipped
  int32_t para;           // e23 == -e01 and e21 == -e03 (exact parallelogram)
  int32_t kind;           // index into kQuadKind, or kMeshKindTri
};
// mesh: a mesh scene's record, in which a triangle cell carries kMeshKindTri
// (rtp_trace.hpp mesh_quad_test); the inline scene's records never do.
RTP_HD inline MeshCellRecord mesh_cell_record(f3 q, f3 r, f3 s, f3 t, bool mesh) {
  MeshCellRecord c;
  c.e01 = sub(r, q), c.e03 = sub(t, q), c.e21 = sub(r, s), c.e23 = sub(t, s);
  const f3 x = cross(sub(r, q), sub(s, q));
  const float inv = 1.f / sqrtf(dot(x, x));  // vtkm::Normalize: a * (1 / sqrt(dot)), both correctly rounded
  c.n = {x.x * inv, x.y * inv, x.z * inv};
  // zero-structure kind (exact zeros only; see quad_hit_masked)
  auto mask_of = [](f3 e) { return (e.x != 0.0f ? 1 : 0) | (e.y != 0.0f ? 2 : 0) | (e.z != 0.0f ? 4 : 0); };
  const int m01 = mask_of(c.e01), m03 = mask_of(c.e03), m21 = mask_of(c.e21), m23 = mask_of(c.e23);
  // exact parallelogram (see quad_hit_masked): value equality; the sign of a
  // zero component only ever changes the sign of a zero intermediate
  c.para = (-c.e01.x == c.e23.x && -c.e03.x == c.e21.x && -c.e01.y == c.e23.y && -c.e03.y == c.e21.y &&
            -c.e01.z == c.e23.z && -c.e03.z == c.e21.z)
               ? 1
               : 0;
  // Kinds 1..6 are axis-plane rectangles: their masks force s = (r_I, t_J),
  // so e23 == -e01 and e21 == -e03 exactly and they are always exact
  // parallelograms (the prefilter's exact test, quad_hit_axis, relies on it;
  // setup_prefilter re-checks para).  An in-plane quad that is not a
  // parallelogram has a non-rectangular mask set and is kind 0.
  c.kind = 0;
#pragma unroll
  for (int k = 1; k < kQuadKinds; k++)
    if (kQuadKind[k].m01 == m01 && kQuadKind[k].m03 == m03 && kQuadKind[k].m21 == m21 && kQuadKind[k].m23 == m23)
      c.kind = k;
  if (mesh && mesh_is_triangle(&s.x, &t.x)) c.kind = kMeshKindTri;
  return c;
}

}  // namespace rtp
