// rtp_mesh_gpu.hip -- device-side build of a mesh scene's quad BVH
// (rtp_set_scene_mesh_device): what rtp_mesh_host.cpp and rtp_set_scene_mesh
// do on the host, from vertices and connectivity that stay on the device.
//
//   1. k_validate   mesh_validate's per-quad checks (the first failure by
//                   lowest quad index) and the min / max of the vertices;
//   2. k_boxes      each quad's pad (double, quad_pad's operations; tri_pad's
//                   for a triangle cell, v11 == v01), padded box and box
//                   centre; the centres' bounds; the counts of rtp_mesh_counts;
//   3. k_morton     30-bit Morton code of the centre, bit 30 for a quad with
//                   the unbounded box: those sort behind all others and the
//                   radix tree splits them off near its root;
//   4. rocPRIM's radix sort of (key, quad) over 31 bits (hipCUB);
//   5. k_karras     Karras' binary radix tree (equal keys split by position);
//   6. k_leaves     every node whose range holds at most kMeshLeaf quads of
//                   one class becomes one leaf; nothing below it is emitted;
//   7. k_round      boxes and emitted-subtree sizes bottom-up, ONE LAUNCH PER
//                   LEVEL: a node is merged in the round after both children.
//                   No value is handed from one workgroup to another inside a
//                   launch (a node merged in round r is read as "not yet" by
//                   every thread of round r), so no fence is needed;
//   8. k_flatten    each emitted node finds its depth-first position in all 8
//                   octant orders in one climb to the root and writes its
//                   16-byte compact node (half-precision box rounded outward);
//   9. k_quads      the DevQuad record of each quad, computed in leaf order
//                   and written with 16-byte stores, and its mesh_shade row.
//
// Everything a pixel depends on (edges, normal, albedo) repeats fill_quad's
// float operations in its order with correctly rounded sqrt and division and
// no contraction, so the records equal the host's bit for bit; so do the pads
// (IEEE double add, multiply, divide and sqrt) and the boxes.
#include <hip/hip_runtime.h>

#include <cstring>

#include <hipcub/hipcub.hpp>

#include "rtp_layout.hpp"
#include "rtp_mesh_gpu.hpp"

#pragma clang fp contract(off)

namespace rtp {
namespace {

constexpr int kTb = 256;
// the radix tree's height: 31 key bits, then positions below 2^22
constexpr int kMaxRounds = 31 + 22;
// k_leaves / k_round: a node's level (height among the emitted nodes)
constexpr int kNotEmitted = -2, kPending = -1;

// ------------------------------------------------------------- helpers ---
__device__ __forceinline__ uint32_t float_key(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float key_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// std::min / std::max as the host's compile evaluates them (the sign of a zero)
__device__ __forceinline__ float hmin(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float hmax(float a, float b) { return (a < b) ? b : a; }
__device__ __forceinline__ double hmind(double a, double b) { return (b < a) ? b : a; }
__device__ __forceinline__ double hmaxd(double a, double b) { return (a < b) ? b : a; }
// std::nextafter(x, +inf) and (x, -inf) of a float that is not NaN
__device__ __forceinline__ float next_up(float x) {
  const uint32_t b = __float_as_uint(x);
  if ((b & 0x7fffffffu) == 0) return __uint_as_float(1u);
  if (b == 0x7f800000u) return x;
  return __uint_as_float((b & 0x80000000u) ? b - 1 : b + 1);
}
__device__ __forceinline__ float next_down(float x) { return -next_up(-x); }
__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool finite_d(double x) {
  return ((uint64_t)__double_as_longlong(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

struct f3 {
  float x, y, z;
};
__device__ __forceinline__ f3 sub(f3 a, f3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ f3 cross(f3 a, f3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
struct d3 {
  double x, y, z;
};
__device__ __forceinline__ d3 subd(d3 a, d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dotd(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ d3 crossd(d3 a, d3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double lend(d3 a) { return sqrt(dotd(a, a)); }
__device__ __forceinline__ d3 todouble(f3 a) { return {a.x, a.y, a.z}; }

__device__ __forceinline__ f3 load_point(const float* __restrict__ points, int32_t id) {
  const float* p = points + 3 * (int64_t)id;
  return {p[0], p[1], p[2]};
}

// rtp_mesh_host.cpp quad_pad, operation for operation
__device__ float quad_pad(d3 q, d3 r, d3 s, d3 t, double reach, double amax) {
  const d3 e01 = subd(r, q), e03 = subd(t, q), e21 = subd(r, s), e23 = subd(t, s);
  const d3 n1 = crossd(e01, e03);
  const double A1 = lend(n1), A2 = lend(crossd(e21, e23));
  const double l1 = lend(e01) * lend(e03), l2 = lend(e21) * lend(e23);
  if (!(A1 > 0) || !(A2 > 0) || !finite_d(A1) || !finite_d(A2)) return kMeshHuge;
  const double sine = hmind(A1 / l1, A2 / l2);
  if (!(sine >= kMeshMinSine)) return kMeshHuge;
  const double h = fabs(dotd(subd(s, q), n1)) / A1;
  if (h > 0) {
    const d3 diag = subd(t, r);
    const d3 u1 = crossd(n1, diag);
    const double lu = lend(u1);
    if (!(lu > 0)) return kMeshHuge;
    const double side = dotd(subd(q, r), u1) < 0 ? 1.0 : -1.0;
    const double w = side * dotd(subd(s, r), u1) / lu;
    if (!(w > 0) || !(h / w < 0.5 * kMeshCosMin)) return kMeshHuge;
  }
  const double slab = 1e-5 + 0x1p-16 * amax + 0x1p-18 * reach;
  const double pad = ((double)kMeshRound * reach / sine + h) / (double)kMeshCosMin + slab;
  if (!(pad < reach)) return kMeshHuge;
  return next_up((float)pad);
}
// rtp_mesh_host.cpp tri_pad, operation for operation
__device__ float tri_pad(d3 q, d3 r, d3 t, double reach, double amax) {
  const d3 e01 = subd(r, q), e03 = subd(t, q);
  const double A1 = lend(crossd(e01, e03));
  const double l1 = lend(e01) * lend(e03);
  if (!(A1 > 0) || !finite_d(A1)) return kMeshHuge;
  const double sine = A1 / l1;
  if (!(sine >= kMeshMinSine)) return kMeshHuge;
  const double slab = 1e-5 + 0x1p-16 * amax + 0x1p-18 * reach;
  const double pad = ((double)kMeshRound * reach / sine) / (double)kMeshCosMin + slab;
  if (!(pad < reach)) return kMeshHuge;
  return next_up((float)pad);
}

// a block's min / max of three floats per thread into six global keys
struct BlockBounds {
  uint32_t lo[3], hi[3];
};
__device__ __forceinline__ void bounds_init(BlockBounds& s) {
  if (threadIdx.x < 3) s.lo[threadIdx.x] = 0xffffffffu, s.hi[threadIdx.x] = 0u;
  __syncthreads();
}
__device__ __forceinline__ void bounds_add(BlockBounds& s, f3 v) {
  atomicMin(&s.lo[0], float_key(v.x)), atomicMax(&s.hi[0], float_key(v.x));
  atomicMin(&s.lo[1], float_key(v.y)), atomicMax(&s.hi[1], float_key(v.y));
  atomicMin(&s.lo[2], float_key(v.z)), atomicMax(&s.hi[2], float_key(v.z));
}
__device__ __forceinline__ void bounds_flush(BlockBounds& s, uint32_t* lo, uint32_t* hi) {
  __syncthreads();
  if (threadIdx.x < 3) atomicMin(&lo[threadIdx.x], s.lo[threadIdx.x]), atomicMax(&hi[threadIdx.x], s.hi[threadIdx.x]);
}

// ------------------------------------------------------------ 1 validate ---
__global__ void k_validate(MeshGpuIn in, MeshGpuInfo* __restrict__ info) {
  __shared__ BlockBounds sb;
  bounds_init(sb);
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < in.n_quads) {
    int32_t id[4];
    bool ids_ok = true;
    for (int k = 0; k < 4; k++) {
      id[k] = in.quad_points[4 * (int64_t)q + k];
      ids_ok = ids_ok && id[k] >= 0 && id[k] < in.n_points;
    }
    const int32_t m = in.quad_mat[q], t = in.quad_tex[q];
    const bool mat_ok = m >= 0 && m < in.n_mat && in.mat_chk[m] >= 0;
    const bool tex_ok = t >= 0 && t < in.n_tex_type && in.tex_chk[t] >= 0;
    uint32_t fail = kMeshNoFail;
    if (!ids_ok) {
      fail = kMeshFailPoint;
    } else {
      f3 v[4];
      bool fin = true;
      for (int k = 0; k < 4; k++) {
        v[k] = load_point(in.points, id[k]);
        fin = fin && finite_f(v[k].x) && finite_f(v[k].y) && finite_f(v[k].z);
      }
      if (!mat_ok || !tex_ok) fail = kMeshFailMaterial;
      else if (!fin) fail = kMeshFailFinite;
      else
        for (int k = 0; k < 4; k++) bounds_add(sb, v[k]);
    }
    if (fail != kMeshNoFail) atomicMin(&info->first_fail, (uint32_t)q << 2 | fail);
  }
  bounds_flush(sb, info->lo, info->hi);
}

// --------------------------------------------------------------- 2 boxes ---
__global__ void k_boxes(MeshGpuIn in, float reach, float* __restrict__ boxes, float* __restrict__ pads,
                        float* __restrict__ cen, MeshGpuInfo* __restrict__ info) {
  __shared__ BlockBounds sb;
  __shared__ uint32_t counts[2];  // this block's triangle cells and unbounded boxes (rtp_mesh_counts)
  if (threadIdx.x < 2) counts[threadIdx.x] = 0u;
  bounds_init(sb);
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < in.n_quads) {
    f3 v[4];
    for (int k = 0; k < 4; k++) v[k] = load_point(in.points, in.quad_points[4 * (int64_t)q + k]);
    const bool tri = mesh_is_triangle(&v[2].x, &v[3].x);
    float mn[3], mx[3];
    for (int k = 0; k < 3; k++) {
      const float a = (&v[0].x)[k], b = (&v[1].x)[k], c = (&v[2].x)[k], d = (&v[3].x)[k];
      if (tri) {  // a triangle cell: its three vertices
        mn[k] = hmin(hmin(a, b), d);
        mx[k] = hmax(hmax(a, b), d);
        continue;
      }
      const float far = a + (b - a) + (d - a);  // v00 + e01 + e03 with the records' float edges
      mn[k] = hmin(hmin(hmin(a, b), hmin(c, d)), far);
      mx[k] = hmax(hmax(hmax(a, b), hmax(c, d)), far);
    }
    double amax = 0;
    for (int k = 0; k < 3; k++) amax = hmaxd(amax, (double)hmax(fabsf(mn[k]), fabsf(mx[k])));
    const float pad = tri ? tri_pad(todouble(v[0]), todouble(v[1]), todouble(v[3]), reach, amax)
                          : quad_pad(todouble(v[0]), todouble(v[1]), todouble(v[2]), todouble(v[3]), reach, amax);
    pads[q] = pad;
    if (tri) atomicAdd(&counts[0], 1u);
    if (pad == kMeshHuge) atomicAdd(&counts[1], 1u);
    f3 c;
    for (int k = 0; k < 3; k++) {
      boxes[6 * (int64_t)q + k] = next_down(mn[k] - pad);
      boxes[6 * (int64_t)q + 3 + k] = next_up(mx[k] + pad);
      (&c.x)[k] = 0.5f * mn[k] + 0.5f * mx[k];
      cen[3 * (int64_t)q + k] = (&c.x)[k];
    }
    bounds_add(sb, c);
  }
  bounds_flush(sb, info->clo, info->chi);  // (its barrier also closes this block's counts)
  if (threadIdx.x == 0 && counts[0]) atomicAdd(&info->n_triangles, counts[0]);
  if (threadIdx.x == 1 && counts[1]) atomicAdd(&info->n_unbounded, counts[1]);
}

// -------------------------------------------------------------- 3 morton ---
__device__ __forceinline__ uint32_t expand_bits(uint32_t v) {
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}
__global__ void k_morton(const float* __restrict__ cen, const float* __restrict__ pads,
                         const MeshGpuInfo* __restrict__ info, int n, uint32_t* __restrict__ code,
                         uint32_t* __restrict__ idx) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  uint32_t cell[3];
  for (int k = 0; k < 3; k++) {
    const float lo = key_float(info->clo[k]), ext = key_float(info->chi[k]) - lo;
    const float inv = ext > 0.f ? 1.f / ext : 0.f;  // an axis of zero extent contributes 0
    cell[k] = (uint32_t)fminf(fmaxf((cen[3 * (int64_t)q + k] - lo) * inv * 1024.0f, 0.0f), 1023.0f);
  }
  const uint32_t huge = pads[q] == kMeshHuge ? 1u << 30 : 0u;
  code[q] = huge | (expand_bits(cell[0]) * 4u + expand_bits(cell[1]) * 2u + expand_bits(cell[2]));
  idx[q] = (uint32_t)q;
}

// -------------------------------------------------------------- 5 karras ---
// common-prefix length of sorted keys i and j (-1 outside); equal keys compare
// their positions, so every key is distinct (rtp_bvh_gpu.hip delta)
__device__ __forceinline__ int delta(const uint32_t* __restrict__ code, int n, int i, int j) {
  if (j < 0 || j >= n) return -1;
  const uint32_t a = code[i], b = code[j];
  if (a != b) return __clz(a ^ b);
  return 32 + __clz((uint32_t)i ^ (uint32_t)j);
}

// Node ids: internal nodes 0..n-2 (root 0), the radix tree's leaf j (sorted
// position) = n-1+j.  range: the node's first and last sorted position.
__global__ void k_karras(const uint32_t* __restrict__ code, int n, int2* __restrict__ child, int* __restrict__ parent,
                         int8_t* __restrict__ axis, int2* __restrict__ range) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n - 1) return;
  const int d = (delta(code, n, i, i + 1) - delta(code, n, i, i - 1)) >= 0 ? 1 : -1;
  const int dmin = delta(code, n, i, i - d);
  int lmax = 2;
  while (delta(code, n, i, i + lmax * d) > dmin) lmax <<= 1;
  int l = 0;
  for (int t = lmax >> 1; t >= 1; t >>= 1)
    if (delta(code, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = delta(code, n, i, j);
  int s = 0;
  for (int div = 2;; div <<= 1) {
    const int t = (l + div - 1) / div;
    if (delta(code, n, i, i + (s + t) * d) > dnode) s += t;
    if (t == 1) break;
  }
  const int gamma = i + s * d + min(d, 0);
  const int first = min(i, j), last = max(i, j);
  const int left = (first == gamma) ? (n - 1 + gamma) : gamma;
  const int right = (last == gamma + 1) ? (n - 1 + gamma + 1) : gamma + 1;
  child[i] = make_int2(left, right);
  range[i] = make_int2(first, last);
  parent[left] = i;
  parent[right] = i;
  // split axis: the Morton bit the range splits on (x at bits 3k+2, y 3k+1,
  // z 3k); bit 30 (bounded | unbounded) and equal keys split by position: x
  const int bit = 31 - dnode;
  axis[i] = (int8_t)((dnode >= 32 || bit == 30) ? 0 : (bit % 3 == 2 ? 0 : (bit % 3 == 1 ? 1 : 2)));
  if (i == 0) parent[0] = -1;
}

// -------------------------------------------------------------- 6 leaves ---
// first sorted position and count of node x, and whether it may be one leaf:
// at most kMeshLeaf quads, all bounded or all unbounded
__device__ __forceinline__ bool leafable(const uint32_t* __restrict__ code, const int2* __restrict__ range, int n, int x,
                                         int& first, int& count) {
  if (x >= n - 1) {
    first = x - (n - 1), count = 1;
    return true;
  }
  const int2 r = range[x];
  first = r.x, count = r.y - r.x + 1;
  return count <= kMeshLeaf && (((code[r.x] ^ code[r.y]) >> 30) & 1u) == 0;
}

// A node is emitted when it is the root or its parent is no leaf.  An emitted
// node that may be a leaf is one (level 0: box = union of its quads' boxes,
// size 1); the other emitted nodes wait for k_round.
__global__ void k_leaves(const uint32_t* __restrict__ code, const uint32_t* __restrict__ idx,
                         const int2* __restrict__ range, const int* __restrict__ parent,
                         const float* __restrict__ boxes, int n, float4* __restrict__ blo, float4* __restrict__ bhi,
                         int* __restrict__ size, int* __restrict__ level, uint32_t* __restrict__ word) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= 2 * n - 1) return;
  int first, count, pf, pc;
  const bool leaf = leafable(code, range, n, x, first, count);
  const int p = parent[x];
  if (p >= 0 && leafable(code, range, n, p, pf, pc)) {
    level[x] = kNotEmitted;
    return;
  }
  if (!leaf) {
    level[x] = kPending;
    word[x] = 0;
    return;
  }
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int j = first; j < first + count; j++) {
    const float* b = boxes + 6 * (int64_t)idx[j];
    for (int k = 0; k < 3; k++) lo[k] = fminf(lo[k], b[k]), hi[k] = fmaxf(hi[k], b[3 + k]);
  }
  blo[x] = make_float4(lo[0], lo[1], lo[2], 0.f);
  bhi[x] = make_float4(hi[0], hi[1], hi[2], 0.f);
  size[x] = 1;
  word[x] = kCBvhLeafBit | (uint32_t)first << 3 | (uint32_t)count;
  level[x] = 0;
}

// --------------------------------------------------------------- 7 round ---
// Round r merges every pending node whose children were finished by an
// earlier launch (level in [0, r)).  A level written in this launch is r, so
// whether or not another workgroup's store is visible yet, the node waits for
// round r + 1, when the launch boundary has made box and size visible.
__global__ void k_round(int r, int n, const int2* __restrict__ child, float4* __restrict__ blo, float4* __restrict__ bhi,
                        int* __restrict__ size, int* __restrict__ level) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n - 1 || level[i] != kPending) return;
  const int2 c = child[i];
  const int lx = level[c.x], ly = level[c.y];
  if (lx < 0 || lx >= r || ly < 0 || ly >= r) return;
  const float4 al = blo[c.x], ah = bhi[c.x], bl = blo[c.y], bh = bhi[c.y];
  blo[i] = make_float4(fminf(al.x, bl.x), fminf(al.y, bl.y), fminf(al.z, bl.z), 0.f);
  bhi[i] = make_float4(fmaxf(ah.x, bh.x), fmaxf(ah.y, bh.y), fmaxf(ah.z, bh.z), 0.f);
  size[i] = 1 + size[c.x] + size[c.y];
  level[i] = r;
}

// ------------------------------------------------------------- 8 flatten ---
// f32 -> f16 bits rounded outward (half_outward's rule, rtp_bvh_gpu.hip): the
// nearest half, stepped outward until its value is on the right side of x
__device__ uint32_t half_outward(float x, bool up) {
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

// one thread per emitted node: its depth-first position in each of the 8
// octant orders (near child first on the parent's split axis) by one climb to
// the root, then the compact node into each copy
__global__ void k_flatten(int n, int n_nodes, const int2* __restrict__ child, const int* __restrict__ parent,
                          const int8_t* __restrict__ axis, const float4* __restrict__ blo,
                          const float4* __restrict__ bhi, const int* __restrict__ size, const int* __restrict__ level,
                          const uint32_t* __restrict__ word, uint4* __restrict__ out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= 2 * n - 1 || level[x] < 0) return;
  int pos[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int c = x, p = parent[x]; p >= 0; c = p, p = parent[p]) {
    const int2 ch = child[p];
    const int ax = axis[p];
    const int sl = size[ch.x], sr = size[ch.y];
#pragma unroll
    for (int oct = 0; oct < 8; oct++) {
      const bool neg = (oct >> ax) & 1;  // moving toward lower coordinates: right (upper) child first
      const int near = neg ? ch.y : ch.x;
      pos[oct] += (c == near) ? 1 : 1 + (neg ? sr : sl);
    }
  }
  const float4 l = blo[x], h = bhi[x];
  uint4 w;
  w.x = half_outward(l.x, false) | half_outward(l.y, false) << 16;
  w.y = half_outward(l.z, false) | half_outward(h.x, true) << 16;
  w.z = half_outward(h.y, true) | half_outward(h.z, true) << 16;
  const uint32_t leaf = word[x];
  const int sz = size[x];
#pragma unroll
  for (int oct = 0; oct < 8; oct++) {
    if (pos[oct] < 0 || pos[oct] >= n_nodes) continue;  // (a closed tree never gets here)
    w.w = leaf ? leaf : (uint32_t)(pos[oct] + sz);
    out[(int64_t)oct * n_nodes + pos[oct]] = w;
  }
}

// --------------------------------------------------------------- 9 quads ---
__device__ __forceinline__ float4 f4(float a, float b, float c, float d) { return make_float4(a, b, c, d); }
__device__ __forceinline__ float fi(int32_t v) { return __int_as_float(v); }
static_assert(offsetof(DevQuad, e01) == 24 && offsetof(DevQuad, key_lo) == 48 && offsetof(DevQuad, e21) == 64 &&
                  offsetof(DevQuad, n) == 88 && offsetof(DevQuad, alb) == 100 && offsetof(DevQuad, mt) == 112,
              "k_quads writes a DevQuad as eight float4s");

// fill_quad (rtp_host.cpp) and rtp_set_scene_mesh's record of stored quad j,
// the caller's quad idx[j]
__global__ void k_quads(MeshGpuIn in, const uint32_t* __restrict__ idx, float4* __restrict__ quads,
                        float4* __restrict__ shade) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= in.n_quads) return;
  const int32_t qi = (int32_t)idx[j];
  const int32_t* id = in.quad_points + 4 * (int64_t)qi;
  const f3 q = load_point(in.points, id[0]), r = load_point(in.points, id[1]), s = load_point(in.points, id[2]),
           t = load_point(in.points, id[3]);
  const f3 e01 = sub(r, q), e03 = sub(t, q), e21 = sub(r, s), e23 = sub(t, s);
  const f3 c = cross(sub(r, q), sub(s, q));
  const float inv = 1.f / sqrtf(dot(c, c));  // vtkm::Normalize: a * (1 / sqrt(dot)), both correctly rounded
  const f3 nrm = {c.x * inv, c.y * inv, c.z * inv};
  auto mask_of = [](f3 e) { return (e.x != 0.0f ? 1 : 0) | (e.y != 0.0f ? 2 : 0) | (e.z != 0.0f ? 4 : 0); };
  const int m01 = mask_of(e01), m03 = mask_of(e03), m21 = mask_of(e21), m23 = mask_of(e23);
  const int32_t para = (-e01.x == e23.x && -e03.x == e21.x && -e01.y == e23.y && -e03.y == e21.y && -e01.z == e23.z &&
                        -e03.z == e21.z)
                           ? 1
                           : 0;
  int32_t kind = 0;
#pragma unroll
  for (int k = 1; k < kQuadKinds; k++)
    if (kQuadKind[k].m01 == m01 && kQuadKind[k].m03 == m03 && kQuadKind[k].m21 == m21 && kQuadKind[k].m23 == m23)
      kind = k;
  if (mesh_is_triangle(&s.x, &t.x)) kind = kMeshKindTri;  // a triangle cell's mark (rtp_set_scene_mesh's record)
  const int32_t mt = in.mat_chk[in.quad_mat[qi]];
  const float* rgb = in.tex_rgb + 3 * in.tex_chk[in.quad_tex[qi]];
  const float a0 = rgb[0], a1 = rgb[1], a2 = rgb[2];
  float4* Q = quads + 8 * (int64_t)j;
  Q[0] = f4(q.x, s.x, q.y, s.y);
  Q[1] = f4(q.z, s.z, e01.x, e01.y);
  Q[2] = f4(e01.z, e03.x, e03.y, e03.z);
  Q[3] = f4(fi(qi), fi(para), fi(qi), fi(kind));  // key_lo = orig = the caller's index
  Q[4] = f4(e21.x, e21.y, e21.z, e23.x);
  Q[5] = f4(e23.y, e23.z, nrm.x, nrm.y);
  Q[6] = f4(nrm.z, a0, a1, a2);
  Q[7] = f4(fi(mt), 0.f, 0.f, 0.f);
  float4* S = shade + 2 * (int64_t)qi;
  S[0] = f4(nrm.x, nrm.y, nrm.z, a0);
  S[1] = f4(a1, a2, fi(mt), 0.f);
}

template <typename T>
hipError_t dalloc(T** p, size_t count) {
  return hipMalloc(reinterpret_cast<void**>(p), (count ? count : 1) * sizeof(T));
}
unsigned blocks(int64_t work) { return (unsigned)((work + kTb - 1) / kTb); }

}  // namespace
}  // namespace rtp

extern "C" hipError_t rtp_mesh_gpu_validate(const rtp::MeshGpuIn* in, rtp::MeshGpuInfo* info, hipStream_t stream) {
  using namespace rtp;
  MeshGpuInfo init;
  std::memset(&init, 0, sizeof(init));
  init.first_fail = kMeshNoFail;
  for (int k = 0; k < 3; k++) init.lo[k] = init.clo[k] = 0xffffffffu;
  MeshGpuInfo* d_info = nullptr;
  hipError_t e = dalloc(&d_info, 1);
  if (e != hipSuccess) return e;
  e = hipMemcpyAsync(d_info, &init, sizeof(init), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_validate, dim3(blocks(in->n_quads)), dim3(kTb), 0, stream, *in, d_info);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(info, d_info, sizeof(*info), hipMemcpyDeviceToHost, stream);
  const hipError_t es = hipStreamSynchronize(stream);  // (also before the free: the kernel may be running)
  if (e == hipSuccess) e = es;
  (void)hipFree(d_info);
  return e;
}

extern "C" void rtp_mesh_gpu_free(rtp::MeshGpuOut* out) {
  for (void* p : {(void*)out->nodes, (void*)out->quads, (void*)out->shade, (void*)out->boxes, (void*)out->pads})
    if (p) (void)hipFree(p);
  *out = rtp::MeshGpuOut();
}

extern "C" hipError_t rtp_mesh_gpu_build(const rtp::MeshGpuIn* in, float reach, rtp::MeshGpuOut* out, int32_t* status,
                                         hipStream_t stream) {
  using namespace rtp;
  const int n = in->n_quads;
  *out = MeshGpuOut();
  *status = 0;
  if (n < 1 || n > kMaxQuadsMesh) return hipErrorInvalidValue;
  const int nn = 2 * n - 1;
  MeshGpuInfo* d_info = nullptr;
  float* cen = nullptr;
  uint32_t *code = nullptr, *code2 = nullptr, *idx = nullptr, *idx2 = nullptr, *word = nullptr;
  int2 *child = nullptr, *range = nullptr;
  int *parent = nullptr, *size = nullptr, *level = nullptr;
  int8_t* axis = nullptr;
  float4 *blo = nullptr, *bhi = nullptr;
  void* temp = nullptr;
  size_t temp_bytes = 0;
  hipError_t e = hipSuccess;
  auto cleanup = [&](bool keep_out) {
    (void)hipStreamSynchronize(stream);  // nothing queued may still read what is freed
    for (void* p : {(void*)d_info, (void*)cen, (void*)code, (void*)code2, (void*)idx, (void*)idx2, (void*)word,
                    (void*)child, (void*)range, (void*)parent, (void*)size, (void*)level, (void*)axis, (void*)blo,
                    (void*)bhi, temp})
      if (p) (void)hipFree(p);
    if (!keep_out) rtp_mesh_gpu_free(out);
  };
#define MESH_TRY(x)         \
  do {                      \
    e = (x);                \
    if (e != hipSuccess) {  \
      cleanup(false);       \
      return e;             \
    }                       \
  } while (0)
  MESH_TRY(dalloc(&out->quads, (size_t)n));
  MESH_TRY(dalloc(&out->shade, (size_t)8 * n));
  MESH_TRY(dalloc(&out->boxes, (size_t)6 * n));
  MESH_TRY(dalloc(&out->pads, (size_t)n));
  MESH_TRY(dalloc(&d_info, 1));
  MESH_TRY(dalloc(&cen, (size_t)3 * n));
  MESH_TRY(dalloc(&code, (size_t)n));
  MESH_TRY(dalloc(&code2, (size_t)n));
  MESH_TRY(dalloc(&idx, (size_t)n));
  MESH_TRY(dalloc(&idx2, (size_t)n));
  MESH_TRY(dalloc(&word, (size_t)nn));
  MESH_TRY(dalloc(&child, (size_t)n));
  MESH_TRY(dalloc(&range, (size_t)n));
  MESH_TRY(dalloc(&parent, (size_t)nn));
  MESH_TRY(dalloc(&size, (size_t)nn));
  MESH_TRY(dalloc(&level, (size_t)nn));
  MESH_TRY(dalloc(&axis, (size_t)n));
  MESH_TRY(dalloc(&blo, (size_t)nn));
  MESH_TRY(dalloc(&bhi, (size_t)nn));
  MeshGpuInfo init;
  std::memset(&init, 0, sizeof(init));
  for (int k = 0; k < 3; k++) init.lo[k] = init.clo[k] = 0xffffffffu;
  MESH_TRY(hipMemcpyAsync(d_info, &init, sizeof(init), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(k_boxes, dim3(blocks(n)), dim3(kTb), 0, stream, *in, reach, out->boxes, out->pads, cen, d_info);
  MESH_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_morton, dim3(blocks(n)), dim3(kTb), 0, stream, cen, out->pads, d_info, n, code, idx);
  MESH_TRY(hipGetLastError());
  MESH_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, code, code2, idx, idx2, n, 0, 31, stream));
  MESH_TRY(hipMalloc(&temp, temp_bytes ? temp_bytes : 1));
  MESH_TRY(hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, code, code2, idx, idx2, n, 0, 31, stream));
  if (n >= 2) {
    hipLaunchKernelGGL(k_karras, dim3(blocks(n - 1)), dim3(kTb), 0, stream, code2, n, child, parent, axis, range);
    MESH_TRY(hipGetLastError());
  } else {
    MESH_TRY(hipMemsetAsync(parent, 0xff, sizeof(int), stream));  // one quad: node 0 is the root and a leaf
  }
  hipLaunchKernelGGL(k_leaves, dim3(blocks(nn)), dim3(kTb), 0, stream, code2, idx2, range, parent, out->boxes, n, blo, bhi,
                     size, level, word);
  MESH_TRY(hipGetLastError());
  const int rounds = n - 1 < kMaxRounds ? n - 1 : kMaxRounds;
  for (int r = 1; r <= rounds; r++) {
    hipLaunchKernelGGL(k_round, dim3(blocks(n - 1)), dim3(kTb), 0, stream, r, n, child, blo, bhi, size, level);
    MESH_TRY(hipGetLastError());
  }
  // the root (node 0 in both cases): its level says whether the tree closed, its size is the node count
  int root[2] = {kPending, 0};
  MESH_TRY(hipMemcpyAsync(&root[0], level, sizeof(int), hipMemcpyDeviceToHost, stream));
  MESH_TRY(hipMemcpyAsync(&root[1], size, sizeof(int), hipMemcpyDeviceToHost, stream));
  MeshGpuInfo counted;  // the 64-byte record again, for k_boxes' two counts
  MESH_TRY(hipMemcpyAsync(&counted, d_info, sizeof(counted), hipMemcpyDeviceToHost, stream));
  MESH_TRY(hipStreamSynchronize(stream));
  if (root[0] < 0 || root[1] < 1 || root[1] > nn) {
    *status = 1;
    cleanup(false);
    return hipSuccess;
  }
  out->n_nodes = root[1];
  out->n_triangles = (int32_t)counted.n_triangles;
  out->n_unbounded = (int32_t)counted.n_unbounded;
  MESH_TRY(dalloc(&out->nodes, (size_t)8 * 4 * out->n_nodes));
  hipLaunchKernelGGL(k_flatten, dim3(blocks(nn)), dim3(kTb), 0, stream, n, out->n_nodes, child, parent, axis, blo, bhi,
                     size, level, word, reinterpret_cast<uint4*>(out->nodes));
  MESH_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_quads, dim3(blocks(n)), dim3(kTb), 0, stream, *in, idx2, reinterpret_cast<float4*>(out->quads),
                     reinterpret_cast<float4*>(out->shade));
  MESH_TRY(hipGetLastError());
  MESH_TRY(hipStreamSynchronize(stream));
#undef MESH_TRY
  cleanup(true);
  return hipSuccess;
}
