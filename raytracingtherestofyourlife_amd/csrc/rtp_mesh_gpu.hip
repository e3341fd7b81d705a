// rtp_mesh_gpu.hip -- device-side build of a mesh scene's quad BVH
// (rtp_set_scene_mesh_device): what rtp_mesh_host.cpp and rtp_set_scene_mesh
// do on the host, from vertices and connectivity that stay on the device.
//
//   1. k_validate   mesh_validate's per-quad checks (the first failure by
//                   lowest quad index) and the min / max of the vertices;
//   2. k_boxes      each quad's pad, padded box and box centre
//                   (rtp_mesh_cell.hpp mesh_cell_box, the host builder's own
//                   function); the centres' bounds; the counts of rtp_mesh_counts;
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
// Everything a pixel depends on (edges, normal, albedo) and every pad and box
// comes from the functions of rtp_mesh_cell.hpp that the host builder calls,
// compiled here with correctly rounded sqrt and division and no contraction,
// so the records, pads and boxes equal the host's bit for bit.  What is left
// here is the device's own: atomics, LDS bounds, 16-byte stores.  The radix
// tree and the octant climb are rtp_lbvh.hpp's, shared with rtp_bvh_gpu.hip.
#include <hip/hip_runtime.h>

#include <cstring>

#include <hipcub/hipcub.hpp>

#include "rtp_layout.hpp"
#include "rtp_lbvh.hpp"
#include "rtp_mesh_cell.hpp"
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
__device__ __forceinline__ f3 load_point(const float* __restrict__ points, int32_t id) {
  return load_f3(points + 3 * (int64_t)id);
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
  atomicMin(&s.lo[0], mesh_float_key(v.x)), atomicMax(&s.hi[0], mesh_float_key(v.x));
  atomicMin(&s.lo[1], mesh_float_key(v.y)), atomicMax(&s.hi[1], mesh_float_key(v.y));
  atomicMin(&s.lo[2], mesh_float_key(v.z)), atomicMax(&s.hi[2], mesh_float_key(v.z));
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
    const MeshCellBox c = mesh_cell_box(v[0], v[1], v[2], v[3], reach);
    pads[q] = c.pad;
    if (c.tri) atomicAdd(&counts[0], 1u);
    if (c.pad == kMeshHuge) atomicAdd(&counts[1], 1u);
    for (int k = 0; k < 3; k++) {
      boxes[6 * (int64_t)q + k] = c.lo[k];
      boxes[6 * (int64_t)q + 3 + k] = c.hi[k];
      cen[3 * (int64_t)q + k] = c.cen[k];
    }
    bounds_add(sb, load_f3(c.cen));
  }
  bounds_flush(sb, info->clo, info->chi);  // (its barrier also closes this block's counts)
  if (threadIdx.x == 0 && counts[0]) atomicAdd(&info->n_triangles, counts[0]);
  if (threadIdx.x == 1 && counts[1]) atomicAdd(&info->n_unbounded, counts[1]);
}

// -------------------------------------------------------------- 3 morton ---
__global__ void k_morton(const float* __restrict__ cen, const float* __restrict__ pads,
                         const MeshGpuInfo* __restrict__ info, int n, uint32_t* __restrict__ code,
                         uint32_t* __restrict__ idx) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  uint32_t cell[3];
  for (int k = 0; k < 3; k++) {
    const float lo = mesh_key_float(info->clo[k]), ext = mesh_key_float(info->chi[k]) - lo;
    const float inv = ext > 0.f ? 1.f / ext : 0.f;  // an axis of zero extent contributes 0
    cell[k] = (uint32_t)fminf(fmaxf((cen[3 * (int64_t)q + k] - lo) * inv * 1024.0f, 0.0f), 1023.0f);
  }
  const uint32_t huge = pads[q] == kMeshHuge ? 1u << 30 : 0u;
  code[q] = huge | (expand_bits(cell[0]) * 4u + expand_bits(cell[1]) * 2u + expand_bits(cell[2]));
  idx[q] = (uint32_t)q;
}

// -------------------------------------------------------------- 5 karras ---
// Node ids: internal nodes 0..n-2 (root 0), the radix tree's leaf j (sorted
// position) = n-1+j.  range: the node's first and last sorted position.  Key
// bit 30 (bounded | unbounded) splits by position like equal keys: axis x.
__global__ void k_karras(const uint32_t* __restrict__ code, int n, int2* __restrict__ child, int* __restrict__ parent,
                         int8_t* __restrict__ axis, int2* __restrict__ range) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n - 1) return;
  const KarrasNode k = karras_node(code, n, i);
  child[i] = make_int2(k.left, k.right);
  range[i] = make_int2(k.first, k.last);
  parent[k.left] = i;
  parent[k.right] = i;
  axis[i] = (int8_t)k.axis;
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
// one thread per emitted node: its depth-first position in each of the 8
// octant orders (rtp_lbvh.hpp octant_positions), then the compact node
// (rtp_mesh_cell.hpp half_outward) into each copy
__global__ void k_flatten(int n, int n_nodes, const int2* __restrict__ child, const int* __restrict__ parent,
                          const int8_t* __restrict__ axis, const float4* __restrict__ blo,
                          const float4* __restrict__ bhi, const int* __restrict__ size, const int* __restrict__ level,
                          const uint32_t* __restrict__ word, uint4* __restrict__ out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= 2 * n - 1 || level[x] < 0) return;
  int pos[8];
  octant_positions(x, 0, child, parent, axis, size, pos);
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

// mesh_records' (rtp_mesh_host.cpp) record of stored quad j, the caller's quad
// idx[j]: mesh_cell_record's values as eight 16-byte stores
__global__ void k_quads(MeshGpuIn in, const uint32_t* __restrict__ idx, float4* __restrict__ quads,
                        float4* __restrict__ shade) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= in.n_quads) return;
  const int32_t qi = (int32_t)idx[j];
  const int32_t* id = in.quad_points + 4 * (int64_t)qi;
  const f3 q = load_point(in.points, id[0]), r = load_point(in.points, id[1]), s = load_point(in.points, id[2]),
           t = load_point(in.points, id[3]);
  const MeshCellRecord c = mesh_cell_record(q, r, s, t, true);
  const f3 e01 = c.e01, e03 = c.e03, e21 = c.e21, e23 = c.e23, nrm = c.n;
  const int32_t mt = in.mat_chk[in.quad_mat[qi]];
  const float* rgb = in.tex_rgb + 3 * in.tex_chk[in.quad_tex[qi]];
  const float a0 = rgb[0], a1 = rgb[1], a2 = rgb[2];
  float4* Q = quads + 8 * (int64_t)j;
  Q[0] = f4(q.x, s.x, q.y, s.y);
  Q[1] = f4(q.z, s.z, e01.x, e01.y);
  Q[2] = f4(e01.z, e03.x, e03.y, e03.z);
  Q[3] = f4(fi(qi), fi(c.para), fi(qi), fi(c.kind));  // key_lo = orig = the caller's index
  Q[4] = f4(e21.x, e21.y, e21.z, e23.x);
  Q[5] = f4(e23.y, e23.z, nrm.x, nrm.y);
  Q[6] = f4(nrm.z, a0, a1, a2);
  Q[7] = f4(fi(mt), 0.f, 0.f, 0.f);
  float4* S = shade + 2 * (int64_t)qi;
  S[0] = f4(nrm.x, nrm.y, nrm.z, a0);
  S[1] = f4(a1, a2, fi(mt), 0.f);
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
