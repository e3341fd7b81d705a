// rtp_host.cpp -- host side of librtp.so: the C ABI declared in include/rtp.h.
//
// Mirrors vtkm::rendering::MapperPathTracer (MapperPathTracer.cxx:94-538):
// the scene/material tables, the camera set-up of pathtracing::Camera
// (Camera.cxx:437-474, 624-776, 879-960) and the render entry point.  All
// ray-independent quantities are precomputed here with the reference's own
// float operations (compiled with -ffp-contract=off; x86-64 SSE2 arithmetic
// is IEEE single/double, the same as the reference's g++ build).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rtp.h"
#include "../../include/rtp_mesh.h"
#include "rtp_context.hpp"
#include "rtp_bvh_host.hpp"
#include "rtp_host_util.hpp"
#include "rtp_layout.hpp"
#include "rtp_mesh.hpp"
#include "rtp_mesh_gpu.hpp"

extern "C" const char* rtp_instance_name(int variant, int stats, int walk, int tiles, int plan, int steal, int views,
                                         int resume);
extern "C" int64_t rtp_plan_history_lanes(int64_t npix, int spp, int bvh, int stats, int* variant_out, int* waves_out);
extern "C" int rtp_plan_steal(int64_t npix, int bvh);
extern "C" hipError_t rtp_launch_render(const rtp::DevScene* scene, const rtp::KParams* p, int variant, int waves, int bvh,
                                        int stats, int steal, hipStream_t stream, int lds_bytes);
extern "C" int rtp_lds_walk_capacity(void);
extern "C" hipError_t rtp_launch_eval_primitive(int kind, const void* in, void* out, int64_t n, const uint32_t* tab,
                                                uint32_t t1, uint32_t t2, hipStream_t stream);
extern "C" hipError_t rtp_launch_build_ff_tables(const rtp::FfBuildOut* out, int max_r, uint32_t t1, uint32_t t2,
                                                 hipStream_t stream);
extern "C" hipError_t rtp_compact_bvh(const rtp::BvhNode* d_nodes, int64_t total, uint32_t* d_cn, int32_t* d_cidx,
                                      hipStream_t stream);
extern "C" hipError_t rtp_build_bvh_gpu(const float4* d_cr, int n, float3 lo, float3 ext, float reach,
                                        rtp::BvhNode* d_nodes, rtp::DevSphereG* d_geom, hipStream_t stream);
extern "C" hipError_t rtp_launch_eval_closest(const rtp::DevScene* scene, const float* rays, uint32_t* out,
                                              int64_t n, int bvh, hipStream_t stream);
extern "C" hipError_t rtp_launch_eval_bounce(const rtp::DevScene* scene, const float* rays, const uint32_t* seeds,
                                             uint32_t* out, int64_t n, int bvh, hipStream_t stream);
extern "C" hipError_t rtp_launch_eval_raygen(const rtp::DevCamera* cam, int nx, int ny, const int64_t* pixels,
                                             const uint32_t* seeds, uint32_t* out, int64_t n, hipStream_t stream);
extern "C" hipError_t rtp_launch_guides(const rtp::DevScene* scene, const rtp::GuideParams* p, int bvh,
                                        hipStream_t stream);
extern "C" hipError_t rtp_launch_verify_fast_math(int kind, uint32_t lo, uint64_t count, unsigned long long* bad,
                                                  uint32_t* first_bad, hipStream_t stream);

using namespace rtp_host;

namespace {

thread_local std::string g_err;

// which = min(3, int(r*3+1)), r = float(t)/4294967295.f  (PdfWorklet.h:20)
int which_of_hash(uint32_t t) {
  float r = (float)t / 4294967295.f;
  int w = (int)(r * 3 + 1);
  return w < 3 ? w : 3;
}
// smallest hash value with which >= w (which is monotone in t)
uint32_t which_threshold(int w) {
  uint64_t lo = 0, hi = 0x100000000ull;  // answer in [lo, hi]
  while (lo < hi) {
    uint64_t mid = (lo + hi) / 2;
    if (which_of_hash((uint32_t)mid) >= w)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo > 0xffffffffull ? 0xffffffffu : (uint32_t)lo;
}

bool bit_equal(const float* a, const float* b, int n) { return std::memcmp(a, b, sizeof(float) * n) == 0; }

// Closest-hit prefilter tables (rtp_kernels.hip closest_hit):
// the quads of groups 0..5 (kinds 1..6, edges along two axes) lie in a plane
// x[axis] = const, bit for bit.  Each gets that plane and a box around its
// vertices in the other two coordinates, widened outward by a few ulps so
// that the float box contains the real one.  Enabled only when every such
// quad qualifies, they fit kMaxPre, and the scene is within the coordinate
// range the kernel's error margins assume (|x| <= kPreLim).
constexpr float kPreLim = 16.0f;
void setup_prefilter(rtp::DevScene* h, const rtp_scene_desc* s, const std::vector<int>& kept) {
  h->n_pre = 0;
  for (int a = 0; a <= 3; a++) h->pre_begin[a] = 0;
  h->pre_scale = 0.0f;
  const int n = h->kind_begin[6];
  if (n <= 0 || n > rtp::kMaxPre) return;
  if (env_is("RTP_PREFILTER", '0')) return;
  std::vector<int> axis_of(n);
  std::vector<rtp::PreQuad> pq(n);
  float scale = 0.0f;
  for (int q = 0; q < n; q++) {
    const rtp::DevQuad& Q = h->quads[q];
    const rtp::QuadKindMasks& K = rtp::kQuadKind[Q.kind];
    const int flat = 7 & ~(K.m01 | K.m03);
    if (Q.kind < 1 || Q.kind > 6 || (flat != 1 && flat != 2 && flat != 4)) return;
    const int a = flat == 1 ? 0 : flat == 2 ? 1 : 2, b = (a + 1) % 3, c = (a + 2) % 3;
    if (!Q.para) return;  // (unreachable: kinds 1..6 are exact parallelograms, see mesh_cell_record)
    {
      const int ei = K.m01 == 1 ? 0 : K.m01 == 2 ? 1 : 2, ej = K.m03 == 1 ? 0 : K.m03 == 2 ? 1 : 2;
      const int ea = 3 - ei - ej;
      rtp::PreExact& E = h->prex[q];
      std::memset(&E, 0, sizeof(E));
      E.i = ei;
      E.s = (ej == (ei + 1) % 3) ? 1 : -1;
      E.b = Q.e01[ei], E.c = Q.e03[ej];
      E.bs = E.s > 0 ? E.b : -E.b, E.cs = E.s > 0 ? E.c : -E.c;
      E.vi = Q.vv[ei][0], E.va = Q.vv[ea][0], E.vj = Q.vv[ej][0];
      E.wi = Q.vv[ei][1], E.wa = Q.vv[ea][1], E.wj = Q.vv[ej][1];
      E.key_lo = Q.key_lo;
    }
    const int32_t* id = s->quad_points + 4 * kept[Q.orig];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const float x = s->points[3 * id[0] + a];
    for (int k = 0; k < 4; k++) {
      const float* v = s->points + 3 * id[k];
      if (!(v[a] == x)) return;  // not in one axis plane
      for (int j = 0; j < 3; j++) {
        if (!std::isfinite(v[j])) return;
        lo[j] = std::min(lo[j], (double)v[j]);
        hi[j] = std::max(hi[j], (double)v[j]);
        scale = std::max(scale, std::fabs(v[j]));
      }
    }
    auto centre_half = [&](int j, float& cen, float& half) {
      cen = (float)(0.5 * (lo[j] + hi[j]));
      const double need = std::max(hi[j] - (double)cen, (double)cen - lo[j]);
      half = (float)need;
      for (int u = 0; u < 2; u++) half = std::nextafter(half, INFINITY);  // >= need after rounding
    };
    rtp::PreQuad& P = pq[q];
    std::memset(&P, 0, sizeof(P));
    P.x = x;
    centre_half(b, P.cb, P.rb);
    centre_half(c, P.cc, P.rc);
    P.qpos = q;
    axis_of[q] = a;
  }
  if (!(scale <= kPreLim)) return;
  int pos = 0;
  for (int a = 0; a < 3; a++) {
    h->pre_begin[a] = pos;
    for (int q = 0; q < n; q++)
      if (axis_of[q] == a) h->pre[pos++] = pq[q];
  }
  h->pre_begin[3] = pos;
  h->pre_scale = scale;
  h->n_pre = n;
}

// RNG jump tables.  A dead depth consumes 1 + {2,3,2} draws chosen by the
// `which` draw against two constant thresholds (lightables = 2,
// MapperPathTracer.cxx:218; PdfWorklet.h:20), so "advance the state over k
// dead depths" is a fixed map of the 32-bit state.  Chain table j tabulates
// it for k = 32 >> j over all 2^32 states (16 GiB each), and the direct
// tables for each k in [d_first, d_first + d_count): a finished sample whose
// remaining count falls in the direct block is fast-forwarded by ONE gather,
// others by a chain of gathers plus a few hashed depths (rtp_render_pool).
// Defaults: 4 chain tables (32, 16, 8, 4) and direct tables 41..50 (the
// counts a depth-50 render's samples mostly have), 224 GiB in all;
// RTP_FF_TABLES=n (0..6) / RTP_FF_DIRECT=n / RTP_FF_DIRECT_FIRST=r change
// the set, and it shrinks to the free device memory (8 GiB kept free).
// The tables are per device and process, shared by every context, and built
// by the policy of rtp_set_ff_tables (include/rtp.h): what they cost
// (allocation + build, measured here) against what they save per sample.
struct FfTables {
  uint32_t* t[rtp::kFfTables] = {};
  uint32_t* direct = nullptr;  // d_count tables of 2^32 entries, contiguous
  int d_first = 0, d_count = 0, n_chain = 0;
  int stage = 0;  // built so far: 1 chain tables, 2 + direct tables
  double alloc_ms = 0, build_ms = 0;
  double chain_alloc_ms = -1;  // the chain stage's own allocation time (-1: not built)
  uint64_t chain_at = 0;       // samples_seen when the chain stage was built
  uint64_t bytes = 0;
  uint64_t samples_seen = 0;  // samples launched on this device (the AUTO policy's count)
};
std::mutex g_ff_mu;
FfTables g_ff[64];

int ff_policy_default() {
  const char* e = getenv("RTP_FF_POLICY");
  if (e && !std::strcmp(e, "on")) return RTP_FF_TABLES_ON;
  if (e && !std::strcmp(e, "off")) return RTP_FF_TABLES_OFF;
  return RTP_FF_TABLES_AUTO;
}

// AUTO builds in two stages, each once the samples launched on the device
// (this launch included) reach its break-even count: setup time over the
// kernel time it saves per sample (C2 on MI355X; round 5,
// profiles/r05z_ff_policy.txt: no tables 126.0 ms, chain tables 106.8 ms,
// all 98.9 ms per 6.4e8 samples):
//  - chain tables (64 GiB): 0.12 s build + an allocation that takes 1 ms to
//    ~1.5 s depending on the box (the driver clearing the memory), saving
//    3.0e-11 s/sample: 7.5e9 samples, ~12 C2 renders (allows ~0.1 s of
//    allocation);
//  - direct tables (+160 GiB): 0.07 s more build + 2.5x the chain stage's
//    measured allocation time, saving 1.23e-11 s/sample: counted from the
//    chain stage, ~9 C2 renders where allocation is fast, ~450 where the
//    chain's 64 GiB took 1.4 s; 3e11 samples before the chain stage is built.
// RTP_FF_AUTO_SAMPLES=chain[,direct] overrides (absolute counts).
constexpr double kFfChainSavePerSample = 3.0e-11, kFfDirectSavePerSample = 1.23e-11;
constexpr double kFfDirectBuildS = 0.07, kFfDirectAllocRatio = 160.0 / 64.0;
void ff_auto_samples(uint64_t& chain, uint64_t& direct, const FfTables* T = nullptr) {
  chain = 7500000000ull;
  direct = 300000000000ull;
  if (const char* e = getenv("RTP_FF_AUTO_SAMPLES")) {
    char* end = nullptr;
    chain = std::strtoull(e, &end, 10);
    direct = (end && *end == ',') ? std::strtoull(end + 1, nullptr, 10) : chain;
    return;
  }
  if (T && T->chain_alloc_ms >= 0) {
    const double setup_s = kFfDirectBuildS + kFfDirectAllocRatio * T->chain_alloc_ms / 1e3;
    direct = std::min<uint64_t>(direct, T->chain_at + (uint64_t)(setup_s / kFfDirectSavePerSample));
  }
  (void)kFfChainSavePerSample;
}

// Allocate and build the tables of a device up to `stage` (caller holds
// g_ff_mu): 1 the chain tables, 2 also the direct block.  The new tables are
// allocated and built through local pointers and published into T only once
// the build kernel has finished: a launch that took its snapshot (FfSnap)
// earlier, and may still be running on another stream, never sees a table
// that is half built, and a failed build frees only what it allocated.
void ff_build(FfTables& T, int stage) {
  if (T.stage >= stage) return;
  int want = 4, nd = 10, first = 41;
  if (const char* env = getenv("RTP_FF_TABLES")) want = std::max(0, std::min(rtp::kFfTables, atoi(env)));
  if (const char* env = getenv("RTP_FF_DIRECT")) nd = std::max(0, std::min(32, atoi(env)));
  if (const char* env = getenv("RTP_FF_DIRECT_FIRST")) first = std::max(1, atoi(env));
  if (first + nd > rtp::kFfMaxSteps) nd = std::max(0, rtp::kFfMaxSteps - first);
  if (want == 0) nd = 0;  // (RTP_FF_TABLES=0: no tables at all)
  const size_t bytes = (size_t)4 << 32, reserve = 8ull << 30;
  auto fits = [&](size_t n) {
    size_t free_b = 0, total_b = 0;
    return hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= n + reserve;
  };
  rtp::FfBuildOut out{};
  uint32_t* chain[rtp::kFfTables] = {};
  uint32_t* direct = nullptr;
  int n_chain = 0, d_count = 0;
  int max_r = 0;
  const auto t0 = std::chrono::steady_clock::now();
  if (T.stage < 1) {
    for (int j = 0; j < want; j++) {
      if (!fits(bytes) || hipMalloc(&chain[j], bytes) != hipSuccess) {
        chain[j] = nullptr;
        break;
      }
      n_chain = j + 1;
      out.t[32 >> j] = chain[j];
      max_r = std::max(max_r, 32 >> j);
    }
  }
  if (stage >= 2 && nd > 0) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
      nd = std::min<int>(nd, free_b > reserve ? (int)((free_b - reserve) / bytes) : 0);
    else
      nd = 0;
    if (nd > 0 && hipMalloc(&direct, bytes * (size_t)nd) == hipSuccess) {
      d_count = nd;
      for (int k = 0; k < nd; k++) {
        out.t[first + k] = direct + (size_t)k * (bytes / 4);
        max_r = std::max(max_r, first + k);
      }
    } else {
      direct = nullptr;
    }
  }
  (void)hipGetLastError();
  const double alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  T.alloc_ms += alloc_ms;
  if (T.stage < 1 && stage == 1 && n_chain > 0) {  // the AUTO policy's estimate of the direct stage's cost
    T.chain_alloc_ms = alloc_ms;
    T.chain_at = T.samples_seen;
  }
  T.stage = stage;  // (a failed stage is not retried)
  if (max_r > 0) {
    const uint32_t t1 = which_threshold(2), t2 = which_threshold(3);
    hipEvent_t a = nullptr, b = nullptr;
    bool ok = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess;
    ok = ok && hipEventRecord(a, nullptr) == hipSuccess;
    ok = ok && rtp_launch_build_ff_tables(&out, max_r, t1, t2, nullptr) == hipSuccess;
    ok = ok && hipEventRecord(b, nullptr) == hipSuccess && hipEventSynchronize(b) == hipSuccess;
    float ms = 0;
    if (ok) (void)hipEventElapsedTime(&ms, a, b);
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    (void)hipGetLastError();
    if (!ok) {  // nothing was published: free this stage's own allocations
      for (uint32_t* p : chain)
        if (p) (void)hipFree(p);
      if (direct) (void)hipFree(direct);
      return;
    }
    T.build_ms += ms;
  }
  // publish (the build has completed)
  for (int j = 0; j < n_chain; j++) T.t[j] = chain[j];
  if (n_chain > 0) T.n_chain = n_chain;
  if (d_count > 0) {
    T.direct = direct;
    T.d_first = first;
    T.d_count = d_count;
  }
  T.bytes = bytes * (size_t)(T.n_chain + T.d_count);
}

// What one launch reads of a device's tables: a copy taken under g_ff_mu,
// so a later stage being built by another thread cannot change it.
struct FfSnap {
  const uint32_t* t[rtp::kFfTables] = {};
  const uint32_t* direct = nullptr;
  int d_first = 0, d_count = 0;
};

// The tables a launch of `samples` samples on `device` uses under `policy`
// (built first when the policy says so).  The tables, once published, stay
// until the process ends.
FfSnap ff_tables(int device, int policy, uint64_t samples) {
  std::lock_guard<std::mutex> lk(g_ff_mu);
  FfTables& T = g_ff[device & 63];
  T.samples_seen += samples;
  if (policy == RTP_FF_TABLES_ON) {
    ff_build(T, 2);
  } else if (policy == RTP_FF_TABLES_AUTO) {
    uint64_t chain = 0, direct = 0;
    ff_auto_samples(chain, direct, &T);
    if (T.samples_seen >= direct) ff_build(T, 2);
    else if (T.samples_seen >= chain) ff_build(T, 1);
  }
  FfSnap s;
  if (policy == RTP_FF_TABLES_OFF) return s;
  for (int j = 0; j < rtp::kFfTables; j++) s.t[j] = T.t[j];
  s.direct = T.direct;
  s.d_first = T.d_first;
  s.d_count = T.d_count;
  return s;
}

// Sphere BVH (replaces the VTK-m LinearBVH of buildBVH, MapperPathTracer.cxx:
// 437-449, for scenes with many spheres).  Binned SAH (16 bins per axis) with
// deterministic partitions, leaves of <= kBvhLeafSize spheres.  The tree is
// flattened eight times, once per ray-direction octant: each copy is a
// depth-first "threaded" array (hit: next node; miss or leaf done: skip) that
// visits the child on the near side of the split axis first, so a lane walks
// near-to-far without a stack and the closest-hit bound culls early.  Boxes
// only cull: each sphere box is padded (rtp_layout.hpp bvh_sphere_pad, from
// the roundings of the device's float sphere test) so that every ray that
// test accepts, and the point it returns, lie inside it, and the kernel
// compares against a slack-widened [0, t_best] interval.  The
// closest hit is the lexicographic min of (t, kind, index) whatever the order.
// (BvhPrim, TNode, bvh_build and the threaded flattening: rtp_bvh_host.hpp, shared with the mesh BVH)

// inner nodes of the sphere BVH above this depth are dropped from the walks'
// arrays (bvh_flatten below)
constexpr int kBvhDropDepth = 2;
constexpr float kBvhDropArea = 0.6f;  // (0: off)

// threaded flattening for one octant (bit k set: direction component k < 0)
// A one-sphere leaf carries the sphere itself (rtp::kBvhLeafSphere): lo =
// centre, hi[0] = r*r, hi[1] = the sphere's index (as int bits), so the walk
// runs the exact root test without a box test or a second dependent load.
// Inner nodes above depth `drop` are not emitted: their children take their
// place in the order (the skip of the node before them then lands on their
// first emitted descendant), so the walk treats their boxes as hit.  A box
// only culls, so this changes which nodes a ray visits, never its hit.  The
// top boxes (the whole sphere cloud, its halves) are hit by nearly every ray
// from inside the room: each one dropped is one dependent gather and box test
// fewer per walk.
// Below that, with drop_sa > 0, an inner node with two inner children is
// dropped too when its surface area exceeds drop_sa of its parent's (a ray
// that reaches it would hit its box with about that probability: dropping it
// saves one visit when it would be hit and costs one when it would not).
void bvh_flatten(const std::vector<TNode>& T, int t, int oct, const std::vector<int32_t>& order,
                 const std::vector<rtp::DevSphere>& sph, std::vector<rtp::BvhNode>& out, int drop = 0,
                 float drop_sa = 0.f) {
  bvh_thread(
      T, t, oct, out,
      [&](const TNode& s, rtp::BvhNode& nd) {
        if (RTP_BVH_EMBED && s.count == 1) {
          const rtp::DevSphere& S = sph[order[s.first]];
          std::memcpy(nd.lo, S.c, sizeof(nd.lo));
          nd.hi[0] = S.rr;
          int32_t orig = order[s.first];
          std::memcpy(&nd.hi[1], &orig, sizeof(orig));
          nd.hi[2] = 0.f;
          nd.leaf = rtp::kBvhLeafSphere;
        } else {
          nd.leaf = (s.first << 3) | s.count;
        }
      },
      [&](const TNode& n, int depth, float area, float parent_area) {
        const bool inner2 = T[n.left].left >= 0 && T[n.right].left >= 0;
        return !(depth < drop || (drop_sa > 0.f && inner2 && parent_area > 0.f && area > drop_sa * parent_area));
      });
}

}  // namespace

// error reporting for the other translation units of librtp.so
rtp_status rtp_internal_fail(rtp_status st, const std::string& msg) {
  g_err = msg;
  return st;
}

namespace {
// the device buffers and events every context owns from rtp_create on
rtp_status create_resources(rtp_context* c) {
  HIP_TRY_AS("hipMalloc(scene)", hipMalloc(&c->d_scene, sizeof(rtp::DevScene)));
  HIP_TRY_AS("hipMalloc(progress)", hipMalloc(&c->d_progress, 16));
  HIP_TRY(hipEventCreate(&c->ev0));
  HIP_TRY(hipEventCreate(&c->ev1));
  HIP_TRY(hipEventCreateWithFlags(&c->done, hipEventDisableTiming));
  return RTP_OK;
}
}  // namespace

extern "C" {

const char* rtp_last_error(void) { return g_err.c_str(); }
int32_t rtp_abi_version(void) { return RTP_ABI_VERSION; }

rtp_status rtp_create(int32_t device, rtp_context** out) {
  if (!out) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_create: out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) return fail(RTP_ERR_DEVICE, "rtp_create: no HIP device available");
  if (device < 0 || device >= n) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_create: device ordinal out of range");
  HIP_TRY(hipSetDevice(device));
  rtp_context* c = new rtp_context();
  c->device = device;
  c->ff_policy = ff_policy_default();
  const rtp_status rs = create_resources(c);
  if (rs != RTP_OK) rtp_destroy(c);  // (the one clean-up path: releases what was made, keeps the message)
  else *out = c;
  return rs;
}

void rtp_destroy(rtp_context* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)drain(c);
  for (void* p : {(void*)c->d_scene, (void*)c->d_hist, (void*)c->d_dbg, (void*)c->d_progress, (void*)c->d_nodes,
                  (void*)c->d_sph_geom, (void*)c->d_sph_all, (void*)c->d_lw_nodes, (void*)c->d_lw_cidx,
                  (void*)c->d_lw_sph, (void*)c->d_lw_orig, (void*)c->d_cnodes, (void*)c->d_cidx, (void*)c->d_direct,
                  (void*)c->d_mesh_nodes, (void*)c->d_mesh_quads, (void*)c->d_mesh_shade, (void*)c->d_mesh_boxes,
                  (void*)c->d_mesh_pads, c->d_adapt_sel, c->d_adapt_state})
    if (p) (void)hipFree(p);
  for (hipEvent_t e : {c->ev0, c->ev1, c->done})
    if (e) (void)hipEventDestroy(e);
  for (rtp_context::ViewTable& t : c->view_tables) {  // (drained above: no launch reads them any more)
    if (t.host) (void)hipHostFree(t.host);
    if (t.dev) (void)hipFree(t.dev);
    if (t.used) (void)hipEventDestroy(t.used);
  }
  delete c;
}

}  // extern "C"

// rtp_set_scene in steps: extract + buildBVH (MapperPathTracer.cxx:178-197,
// 437-449) and the light coupling of the constructor (:141-148).  Every step
// but the last works on the host only and may refuse the description; the
// upload then replaces the context's scene.
namespace {

// what the steps hand on
struct SceneBuild {
  std::unique_ptr<rtp::DevScene> h{new rtp::DevScene()};  // the host image of the device scene
  std::vector<int> kept;                                   // reference index of each kept quad
  float blo[3], bhi[3];                                    // the quads' shape bounds (-direct mode)
  std::vector<rtp::DevSphere> sph;
  bool use_bvh = false, gpu_build = false;
  float bvh_reach = 0.f;
  std::vector<rtp::BvhNode> nodes;  // the host-built sphere BVH: 8 octant copies, and its leaf order's records
  std::vector<rtp::DevSphereG> geom;
  // the LDS walk's tree (kLdsWalkLeaf) in BvhNode form, its leaf order and size
  std::vector<rtp::BvhNode> lw_nodes;
  std::vector<int32_t> lw_order;
  int lw_per_oct = 0;
  // a mesh scene: its BVH (rtp_mesh_host.cpp) and the records it is uploaded as
  bool mesh = false;
  MeshBuild mb;
  std::vector<uint32_t> mesh_cnodes;       // 8 * n_nodes compact nodes
  std::vector<rtp::DevQuad> mesh_quads;    // leaf order
  std::vector<float> mesh_shade;           // 8 floats per quad, the caller's order
  // or, built on the device (rtp_mesh_gpu.hip): the arrays themselves, which scene_upload adopts
  bool mesh_on_device = false;
  rtp::MeshGpuOut mesh_dev;

  // the host image zeroed, every octant its own walk order (the device LBVH
  // build keeps all 8; the host SAH build may narrow it, RTP_BVH_OCT_MASK)
  rtp::DevScene* fresh() {
    std::memset(h.get(), 0, sizeof(*h));
    h->oct_mask = 7;
    return h.get();
  }
};

// (pt_ok, mat_ok, tex_ok: rtp_host_util.hpp, shared with the mesh builder)

// The quads: validated, de-duplicated, grouped by kind, with the prefilter
// tables and the -direct mode's bounds.  Quads that repeat an earlier quad
// bit-for-bit (same vertices in the same order, same material and texture --
// buildBox emits two such pairs per box, CornellBox.cpp:114-137) are dropped:
// under the strict '<' closest test the later copy can never win, so the hit
// record is unchanged.
rtp_status scene_quads(const rtp_scene_desc* s, SceneBuild& B) {
  if (s->n_points <= 0 || !s->points) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: no points");
  if (s->n_quads < 0 || s->n_spheres < 0 || s->n_spheres > rtp::kMaxSpheresBvh)
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: bad primitive counts");
  if (s->n_spheres < 1)
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: the light sphere radius is SphereRadii[0]; need >= 1 sphere");
  rtp::DevScene* h = B.fresh();
  std::vector<int>& kept = B.kept;
  std::vector<rtp::DevQuad> built;
  for (int q = 0; q < s->n_quads; q++) {
    const int32_t* id = s->quad_points + 4 * q;
    for (int k = 0; k < 4; k++)
      if (!pt_ok(s, id[k])) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: quad point id out of range");
    if (!mat_ok(s, s->quad_mat[q]) || !tex_ok(s, s->quad_tex[q]))
      return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: quad material/texture index out of range");
    bool dup = false;
    for (int j : kept) {
      const int32_t* jd = s->quad_points + 4 * j;
      bool same = s->quad_mat[j] == s->quad_mat[q] && s->quad_tex[j] == s->quad_tex[q];
      for (int k = 0; k < 4 && same; k++) same = bit_equal(s->points + 3 * jd[k], s->points + 3 * id[k], 3);
      if (same) {
        dup = true;
        break;
      }
    }
    if (dup) continue;
    if ((int)kept.size() >= rtp::kMaxQuads)
      return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: too many distinct quads");
    rtp::DevQuad Q;
    fill_quad(Q, s->points + 3 * id[0], s->points + 3 * id[1], s->points + 3 * id[2], s->points + 3 * id[3], false);
    Q.mt = s->mat_type[s->quad_mat[q]];
    st(Q.alb, ld(s->tex_rgb + 3 * s->tex_type[s->quad_tex[q]]));
    Q.orig = (int32_t)kept.size();  // rank in the reference's (index) order
    kept.push_back(q);
    built.push_back(Q);
  }
  // group by kind (scan order 1..kQuadKinds-1, then 0); the device scan
  // compares (t, orig) lexicographically, which is exactly the reference's
  // index-order strict '<' scan, so the grouping changes no result.
  {
    int pos = 0;
    for (int g = 0; g < rtp::kQuadKinds; g++) {
      const int kind = (g + 1) % rtp::kQuadKinds;
      h->kind_begin[g] = pos;
      for (const rtp::DevQuad& Q : built)
        if (Q.kind == kind) {
          h->quads[pos] = Q;
          h->quads[pos].key_lo = ((uint32_t)Q.orig << 8) | (uint32_t)pos;  // both < kMaxQuads = 256
          pos++;
        }
    }
    h->kind_begin[rtp::kQuadKinds] = pos;
    if (env_is("RTP_VERBOSE", '1')) {
      fprintf(stderr, "rtp: %d quads by scan group (kind: count / exact parallelograms):", pos);
      for (int g = 0; g < rtp::kQuadKinds; g++) {
        int np = 0;
        for (int i = h->kind_begin[g]; i < h->kind_begin[g + 1]; i++) np += h->quads[i].para ? 1 : 0;
        fprintf(stderr, " %d: %d/%d", (g + 1) % rtp::kQuadKinds, h->kind_begin[g + 1] - h->kind_begin[g], np);
      }
      fprintf(stderr, "\n");
    }
  }
  setup_prefilter(h, s, kept);
  h->n_quads = (int32_t)kept.size();
  // the -direct mode's shape bounds (union of the quads' padded AABBs,
  // AABBSurface.h:36-78)
  float* blo = B.blo;
  float* bhi = B.bhi;
  for (int k = 0; k < 3; k++) blo[k] = INFINITY, bhi[k] = -INFINITY;
  for (int q = 0; q < s->n_quads; q++) {
    const int32_t* id = s->quad_points + 4 * q;
    float mn[3], mx[3];
    for (int k = 0; k < 3; k++) mn[k] = mx[k] = s->points[3 * id[0] + k];
    for (int c2 = 1; c2 < 4; c2++)
      for (int k = 0; k < 3; k++) {
        const float v = s->points[3 * id[c2] + k];
        mn[k] = (v < mn[k]) ? v : mn[k];  // vtkm::Min / Max: (std::min)/(std::max)
        mx[k] = (mx[k] < v) ? v : mx[k];
      }
    for (int k = 0; k < 3; k++) {
      const float ext = 1.0e-4f * (mx[k] - mn[k]);
      const float eps = (1e-6f < ext) ? ext : 1e-6f;
      mn[k] -= eps;
      mx[k] += eps;
      blo[k] = std::min(blo[k], mn[k]);
      bhi[k] = std::max(bhi[k], mx[k]);
    }
  }
  return RTP_OK;
}

// The sphere records, whether they get a BVH, its pad's reach and its builder.
rtp_status scene_spheres(const rtp_scene_desc* s, SceneBuild& B) {
  std::vector<rtp::DevSphere>& sph = B.sph;
  sph.resize(s->n_spheres);
  for (int k = 0; k < s->n_spheres; k++) {
    if (!pt_ok(s, s->sphere_point[k]) || !mat_ok(s, s->sphere_mat[k]) || !tex_ok(s, s->sphere_tex[k]) ||
        !(s->sphere_radius[k] > 0.0f))
      return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: sphere index or radius out of range");
    rtp::DevSphere& S = sph[k];
    std::memset(&S, 0, sizeof(S));
    st(S.c, ld(s->points + 3 * s->sphere_point[k]));
    S.r = s->sphere_radius[k];
    S.rr = S.r * S.r;
    S.mt = s->mat_type[s->sphere_mat[k]];
    st(S.alb, ld(s->tex_rgb + 3 * s->tex_type[s->sphere_tex[k]]));
  }
  const bool use_bvh = B.use_bvh = s->n_spheres >= rtp::kBvhMinSpheres;
  // The reach of the sphere boxes' pad (rtp_layout.hpp bvh_sphere_pad):
  // kBvhReachFactor diagonals of the scene's bounding box -- every quad
  // vertex, every sphere's c -+ r.
  if (use_bvh) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    scene_bounds(s, true, lo, hi);
    B.bvh_reach = rtp::scene_reach(lo, hi);
  }
  // which builder makes the sphere BVH: the host's binned SAH (better trees,
  // O(n log n) on one core) or the device LBVH (rtp_bvh_gpu.hip) for large
  // scenes; RTP_BVH_BUILD=host|gpu overrides
  bool& gpu_build = B.gpu_build;
  gpu_build = use_bvh && s->n_spheres >= rtp::kBvhGpuMinSpheres;
  if (const char* bb = getenv("RTP_BVH_BUILD")) {
    if (!std::strcmp(bb, "gpu")) gpu_build = use_bvh;
    if (!std::strcmp(bb, "host")) gpu_build = false;
  }
  return RTP_OK;
}

// Where the spheres go: into the scene itself (few), or behind a BVH built on
// the device at upload (many) or here -- the global walk's tree and, opt-in,
// the LDS walk's.
void scene_sphere_bvh(const rtp_scene_desc* s, SceneBuild& B) {
  rtp::DevScene* h = B.h.get();
  const std::vector<rtp::DevSphere>& sph = B.sph;
  const float bvh_reach = B.bvh_reach;
  std::vector<rtp::BvhNode>& nodes = B.nodes;
  std::vector<rtp::DevSphereG>& geom = B.geom;
  std::vector<rtp::BvhNode>& lw_nodes = B.lw_nodes;
  std::vector<int32_t>& lw_order = B.lw_order;
  int& lw_per_oct = B.lw_per_oct;
  if (!B.use_bvh) {
    for (int k = 0; k < s->n_spheres; k++) h->spheres[k] = sph[k];
  } else if (B.gpu_build) {
    h->n_nodes = 2 * s->n_spheres - 1;  // nodes and sphere records are built on the device (scene_upload)
  } else {
    std::vector<BvhPrim> P(s->n_spheres);
    for (int k = 0; k < s->n_spheres; k++) {
      const rtp::DevSphere& S = sph[k];
      // (the slab test's margin and what float32 sphere_root accepts beyond
      // the sphere: derived in rtp_layout.hpp; the same call in k_boxes)
      const float pad = rtp::bvh_sphere_pad(S.c[0], S.c[1], S.c[2], S.r, bvh_reach);
      for (int a = 0; a < 3; a++) {
        P[k].lo[a] = S.c[a] - S.r - pad;
        P[k].hi[a] = S.c[a] + S.r + pad;
        P[k].cen[a] = S.c[a];
      }
      P[k].idx = k;
    }
    const std::vector<BvhPrim> P0 = P;  // (bvh_build reorders P)
    std::vector<int32_t> order;
    std::vector<TNode> tree;
    bvh_build(P, 0, s->n_spheres, tree, order);
    // inner nodes above this depth are not emitted (bvh_flatten; RTP_BVH_DROP overrides)
    int drop = kBvhDropDepth;
    float drop_sa = kBvhDropArea;
    if (const char* dd = getenv("RTP_BVH_DROP")) drop = std::max(0, std::min(16, atoi(dd)));
    if (const char* da = getenv("RTP_BVH_DROP_SA")) drop_sa = (float)atof(da);
    // the copies the walk reads: octant o walks copy (o & oct_mask)
    // (RTP_BVH_OCT_MASK; the other copies are built the same and never read)
    int oct_mask = 7;
    if (const char* om = getenv("RTP_BVH_OCT_MASK")) oct_mask = atoi(om) & 7;
    h->oct_mask = oct_mask;
    int per_oct = 0;
    for (int oct = 0; oct < 8; oct++) {  // 8 copies of n_nodes entries, indices local to each copy
      std::vector<rtp::BvhNode> one;
      bvh_flatten(tree, 0, oct & oct_mask, order, sph, one, drop, drop_sa);
      per_oct = (int)one.size();  // (the same nodes are dropped in every octant's order)
      nodes.insert(nodes.end(), one.begin(), one.end());
    }
    // The LDS walk's tree (opt-in, RTP_BVH_LDS=1): leaves of up to
    // kLdsWalkLeaf spheres, flattened the same way, used when its 8 copies
    // plus the leaf spheres fit the block's LDS (the stats build and planned
    // launches walk the global tree).  On C3 at 16 spp (r04h/r04i, kernel ms):
    // LDS walk 324, the global walk over the same leaves-of-6 tree 349, the
    // global walk over the leaves-of-1 tree 186 -- the LDS copy saves 7% of the
    // texture-path gathers' cost, the bigger leaves it needs to fit cost 88%
    // (10 exact sphere tests per ray instead of 4: DESIGN.md 4.2).
    if (env_is("RTP_BVH_LDS", '1')) {
      std::vector<BvhPrim> P2 = P0;
      std::vector<TNode> tree2;
      bvh_build(P2, 0, s->n_spheres, tree2, lw_order, rtp::kLdsWalkLeaf);
      for (int oct = 0; oct < 8; oct++) {
        std::vector<rtp::BvhNode> one;
        bvh_flatten(tree2, 0, oct, lw_order, sph, one, drop, drop_sa);
        lw_per_oct = (int)one.size();
        lw_nodes.insert(lw_nodes.end(), one.begin(), one.end());
      }
      const int64_t bytes = (int64_t)16 * (8 * (int64_t)lw_per_oct + (int64_t)lw_order.size());
      if (bytes > rtp_lds_walk_capacity()) {
        lw_nodes.clear();
        lw_order.clear();
        lw_per_oct = 0;
      }
    }
    geom.resize(order.size());
    for (size_t j = 0; j < order.size(); j++) {
      const rtp::DevSphere& S = sph[order[j]];
      std::memset(&geom[j], 0, sizeof(geom[j]));
      std::memcpy(geom[j].c, S.c, sizeof(S.c));
      geom[j].rr = S.rr;
      geom[j].orig = order[j];
    }
    h->n_nodes = (int32_t)per_oct;
  }
  h->n_spheres = s->n_spheres;
}

// lights (MapperPathTracer.cxx:141-148): light quad = light_box_pointids[1..4];
// the glass constants and the `which` thresholds
rtp_status scene_lights(const rtp_scene_desc* s, SceneBuild& B) {
  rtp::DevScene* h = B.h.get();
  const int32_t* lq = s->light_quad_points;
  for (int k = 0; k < 4; k++)
    if (!pt_ok(s, lq[k])) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: light quad point id out of range");
  if (!pt_ok(s, s->light_sphere_point))
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: light sphere point id out of range");
  v3 q = ld(s->points + 3 * lq[0]), r = ld(s->points + 3 * lq[1]), ss = ld(s->points + 3 * lq[2]),
     t = ld(s->points + 3 * lq[3]);
  fill_quad(h->light.quad, &q.x, &r.x, &ss.x, &t.x, false);
  {
    float qr = std::sqrt(dot(sub(r, q), sub(r, q)));  // vtkm::Magnitude
    float qt = std::sqrt(dot(sub(t, q), sub(t, q)));
    h->light.area = qr * qt;  // PdfWorklet.h:236-239
  }
  // QuadWorkletGenerateDir uses pts[pointIndex[1]] and pts[pointIndex[3]]
  {
    float x0 = q.x, x1 = ss.x, z0 = q.z, z1 = ss.z, y0 = q.y, y1 = q.y;
    h->light.gx0 = x0, h->light.gdx = x1 - x0;
    h->light.gy0 = y0, h->light.gdy = y1 - y0;
    h->light.gz0 = z0, h->light.gdz = z1 - z0;
  }
  st(h->light.sc, ld(s->points + 3 * s->light_sphere_point));
  h->light.sr = s->sphere_radius[0];  // SphereRadii[0] (PdfWorklet.h:205-210)
  h->light.srr = h->light.sr * h->light.sr;
  h->ior = s->ior;
  {  // schlick's r0^2 and 1/ior with the reference's operations (float, float; double then float)
    float r0 = (1 - h->ior) / (1 + h->ior);
    h->ior_r0sq = r0 * r0;
    h->ior_inv = (float)(1.0 / h->ior);
  }
  h->which_t1 = which_threshold(2);
  h->which_t2 = which_threshold(3);
  return RTP_OK;
}

#define UPLOAD_TRY(expr) HIP_TRY_AS("rtp_set_scene upload", expr)

// the sphere BVH built on the device (rtp_bvh_gpu.hip) from centres and radii
rtp_status upload_bvh_gpu(rtp_context* c, const rtp_scene_desc* s, SceneBuild& B) {
  rtp::DevScene* h = B.h.get();
  const std::vector<rtp::DevSphere>& sph = B.sph;
  const int n = s->n_spheres;
  std::vector<float4> cr(n);
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int k = 0; k < n; k++) {
    cr[k] = make_float4(sph[k].c[0], sph[k].c[1], sph[k].c[2], sph[k].r);
    for (int a = 0; a < 3; a++) lo[a] = std::min(lo[a], sph[k].c[a]), hi[a] = std::max(hi[a], sph[k].c[a]);
  }
  DevBufs tmp;
  float4* d_cr = nullptr;
  UPLOAD_TRY(hipMalloc(&c->d_nodes, (size_t)8 * h->n_nodes * sizeof(rtp::BvhNode)));
  UPLOAD_TRY(hipMalloc(&c->d_sph_geom, (size_t)n * sizeof(rtp::DevSphereG)));
  UPLOAD_TRY(hipMalloc(&c->d_sph_all, sph.size() * sizeof(rtp::DevSphere)));
  UPLOAD_TRY(tmp.get(&d_cr, (size_t)n * sizeof(float4), cr.data()));
  UPLOAD_TRY(rtp_build_bvh_gpu(d_cr, n, make_float3(lo[0], lo[1], lo[2]),
                               make_float3(hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]), B.bvh_reach, c->d_nodes,
                               c->d_sph_geom, nullptr));
  UPLOAD_TRY(hipMemcpy(c->d_sph_all, sph.data(), sph.size() * sizeof(rtp::DevSphere), hipMemcpyHostToDevice));
  return RTP_OK;
}

// the host-built trees: the global walk's and, when it was built, the LDS walk's
rtp_status upload_bvh_host(rtp_context* c, SceneBuild& B) {
  rtp::DevScene* h = B.h.get();
  const std::vector<rtp::DevSphere>& sph = B.sph;
  UPLOAD_TRY(hipMalloc(&c->d_nodes, B.nodes.size() * sizeof(rtp::BvhNode)));
  UPLOAD_TRY(hipMalloc(&c->d_sph_geom, B.geom.size() * sizeof(rtp::DevSphereG)));
  UPLOAD_TRY(hipMalloc(&c->d_sph_all, sph.size() * sizeof(rtp::DevSphere)));
  UPLOAD_TRY(hipMemcpy(c->d_nodes, B.nodes.data(), B.nodes.size() * sizeof(rtp::BvhNode), hipMemcpyHostToDevice));
  UPLOAD_TRY(hipMemcpy(c->d_sph_geom, B.geom.data(), B.geom.size() * sizeof(rtp::DevSphereG), hipMemcpyHostToDevice));
  UPLOAD_TRY(hipMemcpy(c->d_sph_all, sph.data(), sph.size() * sizeof(rtp::DevSphere), hipMemcpyHostToDevice));
  if (B.lw_per_oct <= 0) return RTP_OK;
  // the LDS walk's tree: compacted like the global one
  const int64_t total = (int64_t)8 * B.lw_per_oct, ns = (int64_t)B.lw_order.size();
  std::vector<float> lsph(4 * ns);
  for (int64_t j = 0; j < ns; j++) {
    const rtp::DevSphere& S = sph[B.lw_order[j]];
    lsph[4 * j] = S.c[0], lsph[4 * j + 1] = S.c[1], lsph[4 * j + 2] = S.c[2], lsph[4 * j + 3] = S.rr;
  }
  DevBufs tmp;
  rtp::BvhNode* d_tmp = nullptr;
  UPLOAD_TRY(tmp.get(&d_tmp, (size_t)total * sizeof(rtp::BvhNode)));
  UPLOAD_TRY(hipMalloc(&c->d_lw_nodes, (size_t)total * 16));
  UPLOAD_TRY(hipMalloc(&c->d_lw_cidx, (size_t)total * sizeof(int32_t)));
  UPLOAD_TRY(hipMalloc(&c->d_lw_sph, (size_t)ns * 16));
  UPLOAD_TRY(hipMalloc(&c->d_lw_orig, (size_t)ns * sizeof(int32_t)));
  UPLOAD_TRY(hipMemcpy(d_tmp, B.lw_nodes.data(), (size_t)total * sizeof(rtp::BvhNode), hipMemcpyHostToDevice));
  UPLOAD_TRY(hipMemcpy(c->d_lw_sph, lsph.data(), (size_t)ns * 16, hipMemcpyHostToDevice));
  UPLOAD_TRY(hipMemcpy(c->d_lw_orig, B.lw_order.data(), (size_t)ns * sizeof(int32_t), hipMemcpyHostToDevice));
  UPLOAD_TRY(rtp_compact_bvh(d_tmp, total, c->d_lw_nodes, c->d_lw_cidx, nullptr));
  h->lw_nodes = c->d_lw_nodes;
  h->lw_cidx = c->d_lw_cidx;
  h->lw_sph = c->d_lw_sph;
  h->lw_orig = c->d_lw_orig;
  h->n_lw_nodes = B.lw_per_oct;
  h->n_lw_sph = (int32_t)ns;
  return RTP_OK;
}

// Replace the context's scene by the built one.  From the first freed buffer
// until the new DevScene is on the device the context has no scene: an upload
// that fails leaves it answering RTP_ERR_NO_SCENE (the arrays it did allocate
// stay the context's and go with the next rtp_set_scene or rtp_destroy).
rtp_status scene_upload(rtp_context* c, const rtp_scene_desc* s, SceneBuild& B) {
  rtp::DevScene* h = B.h.get();
  UPLOAD_TRY(hipSetDevice(c->device));
  if (c->pending) {  // a queued render may still read the old scene
    const hipError_t e = hipEventSynchronize(c->done);
    c->pending = false;
    UPLOAD_TRY(e);
  }
  c->has_scene = false;
  c->use_bvh = false;
  c->lw_bytes = 0;
  c->oct_mask = 0;
  c->is_mesh = false;
  for (void** p : {(void**)&c->d_nodes, (void**)&c->d_sph_geom, (void**)&c->d_sph_all, (void**)&c->d_cnodes,
                   (void**)&c->d_cidx, (void**)&c->d_lw_nodes, (void**)&c->d_lw_cidx, (void**)&c->d_lw_sph,
                   (void**)&c->d_lw_orig, (void**)&c->d_mesh_nodes, (void**)&c->d_mesh_quads,
                   (void**)&c->d_mesh_shade, (void**)&c->d_mesh_boxes, (void**)&c->d_mesh_pads})
    if (*p) {
      const hipError_t e = hipFree(*p);
      *p = nullptr;
      UPLOAD_TRY(e);
    }
  if (B.use_bvh) {
    RTP_TRY(B.gpu_build ? upload_bvh_gpu(c, s, B) : upload_bvh_host(c, B));
    h->nodes = c->d_nodes;
    h->sph_geom = c->d_sph_geom;
    h->sph_all = c->d_sph_all;
    // the walks' compact copy of the octant arrays
    const int64_t total = (int64_t)8 * h->n_nodes;
    UPLOAD_TRY(hipMalloc(&c->d_cnodes, (size_t)total * 16));
    UPLOAD_TRY(hipMalloc(&c->d_cidx, (size_t)total * sizeof(int32_t)));
    UPLOAD_TRY(rtp_compact_bvh(c->d_nodes, total, c->d_cnodes, c->d_cidx, nullptr));
    h->cnodes = c->d_cnodes;
    h->cidx = c->d_cidx;
  }
  c->h_mesh_boxes.clear();
  c->h_mesh_pads.clear();
  if (B.mesh && B.mesh_on_device) {
    // built in place while the previous scene was still whole: from here on the arrays are the context's
    c->d_mesh_nodes = B.mesh_dev.nodes;
    c->d_mesh_quads = B.mesh_dev.quads;
    c->d_mesh_shade = B.mesh_dev.shade;
    c->d_mesh_boxes = B.mesh_dev.boxes;
    c->d_mesh_pads = B.mesh_dev.pads;
    B.mesh_dev = rtp::MeshGpuOut();
    h->mesh_nodes = c->d_mesh_nodes;
    h->mesh_quads = c->d_mesh_quads;
    h->mesh_shade = c->d_mesh_shade;
  } else if (B.mesh) {
    c->h_mesh_boxes = std::move(B.mb.boxes);
    c->h_mesh_pads = std::move(B.mb.pads);
    const size_t nb = B.mesh_cnodes.size() * 4, qb = B.mesh_quads.size() * sizeof(rtp::DevQuad),
                 sb = B.mesh_shade.size() * 4;
    UPLOAD_TRY(hipMalloc(&c->d_mesh_nodes, nb));
    UPLOAD_TRY(hipMalloc(&c->d_mesh_quads, qb));
    UPLOAD_TRY(hipMalloc(&c->d_mesh_shade, sb));
    UPLOAD_TRY(hipMemcpy(c->d_mesh_nodes, B.mesh_cnodes.data(), nb, hipMemcpyHostToDevice));
    UPLOAD_TRY(hipMemcpy(c->d_mesh_quads, B.mesh_quads.data(), qb, hipMemcpyHostToDevice));
    UPLOAD_TRY(hipMemcpy(c->d_mesh_shade, B.mesh_shade.data(), sb, hipMemcpyHostToDevice));
    h->mesh_nodes = c->d_mesh_nodes;
    h->mesh_quads = c->d_mesh_quads;
    h->mesh_shade = c->d_mesh_shade;
  }
  UPLOAD_TRY(hipMemcpy(c->d_scene, h, sizeof(*h), hipMemcpyHostToDevice));
  c->is_mesh = B.mesh;
  c->mesh_reach = B.mesh ? B.mb.reach : 0.f;
  c->n_mesh_nodes = B.mesh ? h->n_mesh_nodes : 0;
  c->n_mesh_quads = B.mesh ? h->n_mesh_quads : 0;
  c->n_mesh_triangles = B.mesh ? B.mb.n_triangles : 0;
  c->n_mesh_unbounded = B.mesh ? B.mb.n_unbounded : 0;
  c->lw_bytes = h->n_lw_nodes > 0 ? 16 * (8 * h->n_lw_nodes + h->n_lw_sph) : 0;
  c->use_bvh = B.use_bvh;
  c->oct_mask = B.use_bvh ? h->oct_mask : 0;
  c->kept_quads.assign(B.kept.begin(), B.kept.end());  // the -direct mode's kept quad -> reference index
  c->n_ref_quads = s->n_quads;
  for (int k = 0; k < 3; k++) c->quad_lo[k] = B.blo[k], c->quad_hi[k] = B.bhi[k];
  c->has_scene = true;
  return RTP_OK;
}
// A mesh scene built on the device (include/rtp_mesh.h rtp_set_scene_mesh_device;
// rtp_mesh_gpu.hip): s->points and s->quad_* are device arrays.  The host
// reads back one record (the first failed check, the vertices' bounds), the
// at most 13 points the spheres and lights name, and the node count.  Every
// check, and the whole build, comes before scene_upload frees anything: a
// refused or failed call leaves the previous scene rendering.
rtp_status set_scene_mesh_device(rtp_context* c, const rtp_scene_desc* s, hipStream_t stream) {
  RTP_TRY(mesh_validate_head(s));
  if (!s->quad_points || !s->quad_mat || !s->quad_tex)
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene_mesh_device: NULL device array");
  UPLOAD_TRY(hipSetDevice(c->device));
  // the small tables, as the device's checks and records read them (rtp::MeshGpuIn)
  const int n_mat = std::max(s->n_mat, 0), n_tt = std::max(s->n_tex_type, 0), n_tex = std::max(s->n_tex, 0);
  std::vector<int32_t> tab((size_t)n_mat + n_tt + 1);
  for (int m = 0; m < n_mat; m++) tab[m] = s->mat_type[m] >= 0 && s->mat_type[m] <= 2 ? s->mat_type[m] : -1;
  for (int t = 0; t < n_tt; t++) tab[n_mat + t] = s->tex_type[t] >= 0 && s->tex_type[t] < s->n_tex ? s->tex_type[t] : -1;
  const std::vector<float> no_rgb(3, 0.f);
  DevBufs tmp;
  int32_t* d_tab = nullptr;
  float* d_rgb = nullptr;
  UPLOAD_TRY(tmp.get(&d_tab, tab.size() * sizeof(int32_t), tab.data()));
  UPLOAD_TRY(tmp.get(&d_rgb, (size_t)std::max(n_tex, 1) * 3 * sizeof(float), n_tex ? s->tex_rgb : no_rgb.data()));
  rtp::MeshGpuIn in{s->points, s->n_points, s->quad_points, s->quad_mat, s->quad_tex, s->n_quads,
                    d_tab,     n_mat,       d_tab + n_mat,  n_tt,        d_rgb};
  rtp::MeshGpuInfo info;
  UPLOAD_TRY(rtp_mesh_gpu_validate(&in, &info, stream));
  if (info.first_fail != rtp::kMeshNoFail) return mesh_quad_fail((int)(info.first_fail & 3u));
  RTP_TRY(mesh_validate_tail(s));
  // the points the spheres and the lights name, under ids of their own
  const int ns = s->n_spheres;
  float pts[3 * 13];
  int32_t sphere_point[8];
  rtp_scene_desc hs = *s;
  auto fetch = [&](int slot, int32_t id) {
    return hipMemcpyAsync(pts + 3 * slot, s->points + 3 * (size_t)id, 12, hipMemcpyDeviceToHost, stream);
  };
  for (int k = 0; k < ns; k++) {
    UPLOAD_TRY(fetch(k, s->sphere_point[k]));
    sphere_point[k] = k;
  }
  for (int k = 0; k < 4; k++) {
    UPLOAD_TRY(fetch(ns + k, s->light_quad_points[k]));
    hs.light_quad_points[k] = ns + k;
  }
  UPLOAD_TRY(fetch(ns + 4, s->light_sphere_point));
  hs.light_sphere_point = ns + 4;
  UPLOAD_TRY(hipStreamSynchronize(stream));
  hs.points = pts;
  hs.n_points = ns + 5;
  hs.sphere_point = sphere_point;
  hs.quad_points = hs.quad_mat = hs.quad_tex = nullptr;
  // the reach: mesh_build's, over the device's exact min / max of the quads' vertices and the spheres' c -+ r
  SceneBuild B;
  B.mesh = true;
  {
    float lo[3], hi[3];
    for (int k = 0; k < 3; k++) lo[k] = rtp::mesh_key_float(info.lo[k]), hi[k] = rtp::mesh_key_float(info.hi[k]);
    scene_bounds(&hs, false, lo, hi);
    B.mb.reach = rtp::scene_reach(lo, hi);
    if (!rtp::finite_f(B.mb.reach)) return mesh_bounds_fail();
  }
  rtp::DevScene* h = B.fresh();
  RTP_TRY(scene_spheres(&hs, B));
  scene_sphere_bvh(&hs, B);
  RTP_TRY(scene_lights(&hs, B));
  int32_t open_tree = 0;
  UPLOAD_TRY(rtp_mesh_gpu_build(&in, B.mb.reach, &B.mesh_dev, &open_tree, stream));
  if (open_tree) return fail(RTP_ERR_DEVICE, "rtp_set_scene_mesh_device: the radix tree did not close");
  B.mesh_on_device = true;
  B.mb.n_triangles = B.mesh_dev.n_triangles;
  B.mb.n_unbounded = B.mesh_dev.n_unbounded;
  h->n_mesh_nodes = B.mesh_dev.n_nodes;
  h->n_mesh_quads = s->n_quads;
  h->mesh_scan = env_is("RTP_MESH_SCAN", '1') ? 1 : 0;
  for (int k = 0; k < 3; k++) B.blo[k] = 0.f, B.bhi[k] = 0.f;
  const rtp_status rs = scene_upload(c, s, B);
  rtp_mesh_gpu_free(&B.mesh_dev);  // (what scene_upload did not get to adopt)
  return rs;
}

// RTP_MESH_BUILD=gpu on rtp_set_scene_mesh: its four host arrays go up and the device build runs
rtp_status set_scene_mesh_uploaded(rtp_context* c, const rtp_scene_desc* s) {
  RTP_TRY(mesh_validate_head(s));
  if (!s->quad_points || !s->quad_mat || !s->quad_tex)
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene_mesh: NULL argument");
  UPLOAD_TRY(hipSetDevice(c->device));
  DevBufs tmp;
  rtp_scene_desc ds = *s;
  float* d_points = nullptr;
  int32_t *d_qp = nullptr, *d_qm = nullptr, *d_qt = nullptr;
  const size_t n = (size_t)s->n_quads;
  UPLOAD_TRY(tmp.get(&d_points, (size_t)s->n_points * 12, s->points));
  UPLOAD_TRY(tmp.get(&d_qp, n * 16, s->quad_points));
  UPLOAD_TRY(tmp.get(&d_qm, n * 4, s->quad_mat));
  UPLOAD_TRY(tmp.get(&d_qt, n * 4, s->quad_tex));
  ds.points = d_points, ds.quad_points = d_qp, ds.quad_mat = d_qm, ds.quad_tex = d_qt;
  return set_scene_mesh_device(c, &ds, nullptr);
}
#undef UPLOAD_TRY

}  // namespace

extern "C" {

rtp_status rtp_set_scene(rtp_context* c, const rtp_scene_desc* s) {
  if (!c || !s) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: NULL argument");
  SceneBuild B;
  RTP_TRY(scene_quads(s, B));
  RTP_TRY(scene_spheres(s, B));
  scene_sphere_bvh(s, B);
  RTP_TRY(scene_lights(s, B));
  return scene_upload(c, s, B);
}

// A mesh scene (include/rtp_mesh.h): every quad behind the mesh BVH in global
// memory -- none inline, so the device scene's n_quads is 0 and the inline
// scans and LDS tables are empty -- and at most 8 spheres inline.  Every
// refusal comes before the upload: the previous scene stays.
rtp_status rtp_set_scene_mesh(rtp_context* c, const rtp_scene_desc* s) {
  if (!c || !s) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene_mesh: NULL argument");
  // RTP_MESH_BUILD=gpu: the device build from these host arrays (the A/B handle, like RTP_BVH_BUILD)
  if (const char* mb = getenv("RTP_MESH_BUILD"))
    if (!std::strcmp(mb, "gpu")) return set_scene_mesh_uploaded(c, s);
  SceneBuild B;
  B.mesh = true;
  RTP_TRY(mesh_build(s, B.mb));
  rtp::DevScene* h = B.fresh();
  RTP_TRY(scene_spheres(s, B));  // (fewer than kBvhMinSpheres: no sphere BVH)
  scene_sphere_bvh(s, B);
  RTP_TRY(scene_lights(s, B));
  mesh_records(s, B.mb, B.mesh_quads, B.mesh_shade);
  B.mesh_cnodes.resize((size_t)4 * B.mb.nodes.size());
  mesh_compact(B.mb.nodes.data(), (int64_t)B.mb.nodes.size(), B.mesh_cnodes.data());
  h->n_mesh_nodes = B.mb.n_nodes;
  h->n_mesh_quads = s->n_quads;
  h->mesh_scan = env_is("RTP_MESH_SCAN", '1') ? 1 : 0;
  for (int k = 0; k < 3; k++) B.blo[k] = 0.f, B.bhi[k] = 0.f;  // (-direct mode is refused on a mesh scene)
  return scene_upload(c, s, B);
}

rtp_status rtp_set_scene_mesh_device(rtp_context* c, const rtp_scene_desc* s, void* hip_stream) {
  if (!c || !s) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene_mesh_device: NULL argument");
  return set_scene_mesh_device(c, s, static_cast<hipStream_t>(hip_stream));
}

// test hook (rtp_mesh.hpp): the current mesh scene as its builder left it
rtp_status rtp_debug_mesh_readback(rtp_context* c, int32_t oct, int32_t node_cap, int32_t* n_nodes, void* cnodes,
                                   int32_t* order, float* boxes, float* pads) {
  if (!c || !c->has_scene || !c->is_mesh)
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_debug_mesh_readback: the context holds no mesh scene");
  if (oct < 0 || oct > 7) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_debug_mesh_readback: octant outside 0..7");
  HIP_TRY(hipSetDevice(c->device));
  RTP_TRY(drain(c));
  const size_t nn = (size_t)c->n_mesh_nodes, nq = (size_t)c->n_mesh_quads;
  if (n_nodes) *n_nodes = c->n_mesh_nodes;
  if (cnodes) {
    if (node_cap < c->n_mesh_nodes)
      return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_debug_mesh_readback: node_cap too small");
    HIP_TRY(hipMemcpy(cnodes, c->d_mesh_nodes + 4 * nn * (size_t)oct, 16 * nn, hipMemcpyDeviceToHost));
  }
  if (order)
    HIP_TRY(hipMemcpy2D(order, sizeof(int32_t), reinterpret_cast<const char*>(c->d_mesh_quads) + offsetof(rtp::DevQuad, orig),
                        sizeof(rtp::DevQuad), sizeof(int32_t), nq, hipMemcpyDeviceToHost));
  if (c->d_mesh_boxes) {
    HIP_TRY(DevBufs::back(boxes, c->d_mesh_boxes, 24 * nq));
    HIP_TRY(DevBufs::back(pads, c->d_mesh_pads, 4 * nq));
  } else {
    if (boxes) std::memcpy(boxes, c->h_mesh_boxes.data(), 24 * nq);
    if (pads) std::memcpy(pads, c->h_mesh_pads.data(), 4 * nq);
  }
  return RTP_OK;
}

// test hook (rtp_mesh.hpp): the stored records of the current mesh scene, whole, in leaf order
rtp_status rtp_debug_mesh_records(rtp_context* c, int64_t cap, void* records) {
  if (!c || !c->has_scene || !c->is_mesh)
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_debug_mesh_records: the context holds no mesh scene");
  if (!records || cap < c->n_mesh_quads) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_debug_mesh_records: cap too small");
  HIP_TRY(hipSetDevice(c->device));
  RTP_TRY(drain(c));
  HIP_TRY(hipMemcpy(records, c->d_mesh_quads, sizeof(rtp::DevQuad) * (size_t)c->n_mesh_quads, hipMemcpyDeviceToHost));
  return RTP_OK;
}

rtp_status rtp_mesh_guarantee(rtp_context* c, float* cos_min, float* reach) {
  if (!c || !c->has_scene || !c->is_mesh)
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_mesh_guarantee: the context holds no mesh scene");
  if (cos_min) *cos_min = rtp::kMeshCosMin;
  if (reach) *reach = c->mesh_reach;
  return RTP_OK;
}

rtp_status rtp_mesh_counts(rtp_context* c, int32_t* n_cells, int32_t* n_triangles, int32_t* n_unbounded) {
  if (!c || !c->has_scene || !c->is_mesh)
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_mesh_counts: the context holds no mesh scene");
  if (n_cells) *n_cells = c->n_mesh_quads;
  if (n_triangles) *n_triangles = c->n_mesh_triangles;
  if (n_unbounded) *n_unbounded = c->n_mesh_unbounded;
  return RTP_OK;
}

}  // extern "C"

namespace {

// the entry points a mesh scene does not serve yet (include/rtp_mesh.h): refused before anything is launched
rtp_status refuse_mesh(const rtp_context* c, const char* who) {
  if (c && c->has_scene && c->is_mesh)
    return fail(RTP_ERR_INVALID_ARGUMENT, std::string(who) + ": not available on a mesh scene (rtp_set_scene_mesh)");
  return RTP_OK;
}

// pathtracing::Camera::SetParameters -> CreateRaysImpl -> RayGen ctor
void camera_setup(const rtp_camera* cam, int32_t nx, int32_t ny, rtp::DevCamera* out) {
  v3 up = ld(cam->view_up);
  if (!(up.x == 0.f && up.y == 1.f && up.z == 0.f)) up = normalize(up);  // SetUp (Camera.cxx:767-776)
  v3 pos = ld(cam->position);
  v3 look = normalize(sub(ld(cam->look_at), pos));  // Camera.cxx:908-909
  float thx = tanf((cam->fov_y_deg * kPi180f) * .5f);
  float thy = tanf((cam->fov_y_deg * kPi180f) * .5f);
  v3 u = normalize(cross(look, up));
  v3 v = normalize(cross(u, look));
  st(out->eye, pos);
  st(out->dx, scl(u, (2 * thx / (float)nx)));
  st(out->dy, scl(v, (2 * thy / (float)ny)));
  st(out->nlook, normalize(look));
}

rtp_status check_render_args(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t spp,
                             int32_t depth) {
  if (!c || !cam) return fail(RTP_ERR_INVALID_ARGUMENT, "render: NULL argument");
  RTP_TRY(check_canvas_camera(c, cam, nx, ny, "render"));
  if (spp < 0) return fail(RTP_ERR_INVALID_ARGUMENT, "render: samplecount must be >= 0");
  // depthcount < 1 makes the reference read emitted[(depth-1)*N] out of range
  // (MapperPathTracer.cxx:328-331); rejected here.
  if (depth < 1) return fail(RTP_ERR_INVALID_ARGUMENT, "render: depthcount must be >= 1");
  // device-side bookkeeping limits: the pool kernel packs the remaining dead
  // depths into 14 bits and counts a wave's finished samples (<= 256 * spp)
  // in 32-bit signed cursors
  if (depth > rtp::kMaxDepth) return fail(RTP_ERR_INVALID_ARGUMENT, "render: depthcount must be <= 16383");
  if (spp > rtp::kMaxSpp) return fail(RTP_ERR_INVALID_ARGUMENT, "render: samplecount must be <= 8388607");
  return RTP_OK;
}

rtp_status ensure_hist(rtp_context* c, size_t bytes) {
  if (bytes <= c->hist_bytes) return RTP_OK;
  RTP_TRY(drain(c));
  if (c->d_hist) HIP_TRY(hipFree(c->d_hist));
  c->d_hist = nullptr;
  c->hist_bytes = 0;
  HIP_TRY(hipMalloc(&c->d_hist, bytes));
  c->hist_bytes = bytes;
  return RTP_OK;
}

// One launch of the render kernel: every caller names the fields it uses.
struct RenderJob {
  const rtp_camera* cam = nullptr;        // the camera, or
  const rtp::DevView* d_views = nullptr;  // batched views: cameras and seed bases in a device table
  int32_t nx = 0, ny = 0, spp = 0, depth = 0;
  uint32_t seed_base = 0;
  int64_t pixel_begin = 0, npix = 0;  // the entries: a range, or
  const int64_t* d_ids = nullptr;     // a pixel list
  float* d_out = nullptr;
  uint32_t *d_seed = nullptr, *d_live = nullptr;  // optional final seeds and live-bounce counts
  hipStream_t stream = nullptr;
  const int32_t* tile = nullptr;          // optional tile deal {tiles per row, world, rank}
  const int32_t* d_wave_begin = nullptr;  // optional wave plan of plan_waves waves
  int plan_waves = 0;
  bool resume = false;  // a pass over a render state: d_out, d_seed, d_live, d_m2 are read and updated
  float* d_m2 = nullptr;
  double* kernel_ms = nullptr;  // where the kernel time goes (the call then waits for it)
};

// how a job runs on the context's scene
struct LaunchPlan {
  int variant = 2, waves = 0, bvh = 0;  // bvh: the sphere walk (plan_launch)
  int64_t lanes = 0;                    // history lanes
  bool stats_on = false, dbg = false;   // RTP_DEBUG_STATS=1: the diagnostics build; 1 or 2: per-wave counters
  bool steal = false;                   // the resident waves steal entries (rtp_plan_steal gave `waves`)
};

rtp_status plan_launch(rtp_context* c, const RenderJob& j, LaunchPlan& pl) {
  // the kernels index a launch's entries with 32-bit integers
  if (j.npix > INT32_MAX) return fail(RTP_ERR_INVALID_ARGUMENT, "render: more than 2^31-1 pixels in one launch");
  HIP_TRY(hipSetDevice(c->device));
  // the sphere BVH's walk: 2 out of LDS when the tree fits (rtp_render_pool_lds),
  // 1 the global threaded walk (also for the diagnostics build and wave plans)
  const char stats_env = env_char("RTP_DEBUG_STATS");
  pl.stats_on = stats_env == '1';
  pl.dbg = stats_env == '1' || stats_env == '2';  // 2: timestamps in the production kernel
  // (a launch whose mode has no LDS-walk instance -- a resume pass, say --
  // takes the global walk, same results: the instance table answers)
  const bool lds_walk = c->lw_bytes > 0 && rtp_instance_name(2, pl.stats_on, 2, j.tile != nullptr, j.d_wave_begin != nullptr,
                                                             0, j.d_views != nullptr, j.resume) != nullptr;
  pl.bvh = c->is_mesh ? 3 : !c->use_bvh ? 0 : lds_walk ? 2 : 1;
  if (c->is_mesh && (pl.stats_on || env_is("RTP_KERNEL", '1')))
    return fail(RTP_ERR_INVALID_ARGUMENT,
                "render: RTP_KERNEL=1 and RTP_DEBUG_STATS=1 are not available on a mesh scene (rtp_set_scene_mesh)");
  pl.lanes = rtp_plan_history_lanes(j.npix, j.spp, pl.bvh, pl.stats_on, &pl.variant, &pl.waves);
  if (j.d_wave_begin) {  // a planned launch: the caller's waves
    if (pl.variant != 2 || c->use_bvh || j.tile)
      return fail(RTP_ERR_INVALID_ARGUMENT, "render: a wave plan needs the pool kernel, no BVH, no tile deal");
    pl.waves = j.plan_waves;
    pl.lanes = (int64_t)j.plan_waves * 128;
  }
  // more entries than the resident waves' pools hold: the resident waves
  // steal entries (RTP_STEAL=0: waves of 128 entries in generations)
  if (pl.variant == 2 && !j.d_wave_begin && !pl.stats_on && j.spp > 0) {
    const int sw = env_is("RTP_STEAL", '0') ? 0 : rtp_plan_steal(j.npix, pl.bvh);
    if (sw > 0) {
      pl.steal = true;
      pl.waves = sw;
      pl.lanes = (int64_t)sw * 128;
    }
  }
  pl.dbg = pl.dbg && pl.variant == 2;
  return RTP_OK;
}

rtp_status launch(rtp_context* c, const RenderJob& j) {
  LaunchPlan pl;
  RTP_TRY(plan_launch(c, j, pl));
  rtp::KParams p{};
  if (j.tile) p.tile_tx = j.tile[0], p.tile_world = j.tile[1], p.tile_rank = j.tile[2];
  if (j.d_views) p.views = j.d_views;
  else camera_setup(j.cam, j.nx, j.ny, &p.cam);
  p.nx = j.nx, p.ny = j.ny, p.spp = j.spp, p.depth = j.depth;
  p.seed_base = j.seed_base;
  p.pixel_begin = j.pixel_begin, p.pixel_ids = j.d_ids, p.npix = j.npix;
  p.out = j.d_out, p.seed_out = j.d_seed, p.live_out = j.d_live;
  p.resume = j.resume ? 1 : 0, p.m2 = j.d_m2;
  p.wave_begin = j.d_wave_begin;
  // D rows per lane (row k of a light hit holds E_k), rounded up to 8 (a
  // slot-major history pads each slot to whole 128-byte lines)
  size_t hist_need = (size_t)((j.depth + 7) & ~7) * (size_t)pl.lanes * 16;
  RTP_TRY(ensure_hist(c, hist_need));
  p.hist = c->d_hist;
  p.dbg = nullptr;
  p.progress = c->d_progress;
  if (pl.variant == 2) {
    const FfSnap ft = ff_tables(c->device, c->ff_policy, (uint64_t)j.npix * (uint64_t)j.spp);
    for (int k = 0; k < rtp::kFfTables; k++) p.ff[k] = ft.t[k];
    p.ffd = ft.direct, p.ffd_first = ft.d_first, p.ffd_count = ft.d_count;
  }
  if (c->pending) HIP_TRY(hipStreamWaitEvent(j.stream, c->done, 0));
  HIP_TRY(hipMemsetAsync(c->d_progress, 0, 16, j.stream));  // [0] progress, [1] entries stolen (kSteal)
  if (pl.dbg) {
    if (c->d_dbg) (void)hipFree(c->d_dbg);
    c->d_dbg = nullptr;
    HIP_TRY(hipMalloc(&c->d_dbg, (size_t)pl.waves * rtp::kDbgCounters * 8));
    HIP_TRY(hipMemsetAsync(c->d_dbg, 0, (size_t)pl.waves * rtp::kDbgCounters * 8, j.stream));
    c->dbg_waves = pl.waves;
    p.dbg = c->d_dbg;
  }
  return timed_launch(c, j.stream, j.kernel_ms, true, [&]() -> rtp_status {
    HIP_TRY(rtp_launch_render(c->d_scene, &p, pl.variant, pl.waves, pl.bvh, pl.stats_on, pl.steal, j.stream, c->lw_bytes));
    return RTP_OK;
  });
}

// host-buffer render of an optional pixel list (nullptr: contiguous range)
rtp_status render_host(rtp_context* c, RenderJob j, const int64_t* ids, float* rgba_out, const rtp_pixel_aux* aux,
                       rtp_stats* stats) {
  HIP_TRY(hipSetDevice(c->device));
  if (j.npix == 0) {
    fill_stats(stats, 0, 0);
    return RTP_OK;
  }
  const size_t n = (size_t)j.npix;
  DevBufs b;
  HIP_TRY_AS("render: device buffers", b.get(&j.d_out, n * 16));
  HIP_TRY_AS("render: device buffers", b.get(&j.d_live, n * 4));
  if (aux && aux->final_seed) HIP_TRY_AS("render: device buffers", b.get(&j.d_seed, n * 4));
  int64_t* d_ids = nullptr;
  if (ids) HIP_TRY_AS("render: device buffers", b.get(&d_ids, n * 8, ids));
  double ms = 0;
  j.d_ids = d_ids, j.kernel_ms = &ms;
  std::vector<uint32_t> live(n);
  RTP_TRY(launch(c, j));
  HIP_TRY_AS("render: copy back", DevBufs::back(rgba_out, j.d_out, n * 16));
  HIP_TRY_AS("render: copy back", DevBufs::back(live.data(), j.d_live, n * 4));
  HIP_TRY_AS("render: copy back", DevBufs::back(aux ? aux->final_seed : nullptr, j.d_seed, n * 4));
  if (aux && aux->live_bounces) std::memcpy(aux->live_bounces, live.data(), n * 4);
  fill_stats(stats, (uint64_t)j.npix * (uint64_t)j.spp, ms);
  sum_stats(stats, rgba_out, live.data(), j.npix);
  return RTP_OK;
}

// the job fields every render entry takes from its arguments
RenderJob job_of(const rtp_camera* cam, int32_t nx, int32_t ny, int32_t spp, int32_t depth, uint32_t seed_base) {
  RenderJob j;
  j.cam = cam, j.nx = nx, j.ny = ny, j.spp = spp, j.depth = depth, j.seed_base = seed_base;
  return j;
}
// one more pass over a device render state (its seeds continue: no seed base)
RenderJob resume_job(const rtp_camera* cam, int32_t nx, int32_t ny, int32_t spp, int32_t depth,
                     const rtp_render_state& st) {
  RenderJob j = job_of(cam, nx, ny, spp, depth, 0u);
  j.d_out = st.rgba, j.d_seed = st.seed, j.d_live = st.live_bounces, j.d_m2 = st.m2;
  j.resume = true;
  return j;
}
// the tail of a _device entry: the job on the caller's stream, timed when stats are asked for
rtp_status launch_device(rtp_context* c, RenderJob& j, const rtp_pixel_aux* aux, void* hip_stream, rtp_stats* stats) {
  double ms = 0;
  if (aux) j.d_seed = aux->final_seed, j.d_live = aux->live_bounces;
  j.stream = (hipStream_t)hip_stream;
  j.kernel_ms = stats ? &ms : nullptr;
  RTP_TRY(launch(c, j));
  fill_stats(stats, (uint64_t)j.npix * (uint64_t)j.spp, ms);
  return RTP_OK;
}

// the checks of rtp_render_resume* before their pixel sets
rtp_status check_resume_args(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t spp,
                             int32_t depth, const rtp_render_state* st, const char* who) {
  RTP_TRY(check_render_args(c, cam, nx, ny, spp, depth));
  if (!st || !st->rgba || !st->seed)
    return fail(RTP_ERR_INVALID_ARGUMENT, std::string(who) + ": state, state->rgba and state->seed are required");
  if (env_is("RTP_KERNEL", '1'))
    return fail(RTP_ERR_INVALID_ARGUMENT, std::string(who) + ": not available with RTP_KERNEL=1");
  if (env_is("RTP_DEBUG_STATS", '1'))
    return fail(RTP_ERR_INVALID_ARGUMENT, std::string(who) + ": not available with RTP_DEBUG_STATS=1");
  return RTP_OK;
}

}  // namespace

extern "C" {

rtp_status rtp_render(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t spp, int32_t depth,
                      uint32_t seed_base, float* rgba_out, rtp_stats* stats) {
  RTP_TRY(check_render_args(c, cam, nx, ny, spp, depth));
  if (!rgba_out) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_render: rgba_out is NULL");
  RenderJob j = job_of(cam, nx, ny, spp, depth, seed_base);
  j.npix = (int64_t)nx * ny;
  return render_host(c, j, nullptr, rgba_out, nullptr, stats);
}

rtp_status rtp_render_pixels(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t spp,
                             int32_t depth, uint32_t seed_base, const int64_t* pixel_ids, int64_t pixel_count,
                             float* rgba_out, const rtp_pixel_aux* aux, rtp_stats* stats) {
  RTP_TRY(check_render_args(c, cam, nx, ny, spp, depth));
  if (pixel_count < 0 || (pixel_count > 0 && (!pixel_ids || !rgba_out)))
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_render_pixels: bad pixel list / output");
  const int64_t npx = (int64_t)nx * ny;
  for (int64_t i = 0; i < pixel_count; i++)
    if (pixel_ids[i] < 0 || pixel_ids[i] >= npx)
      return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_render_pixels: pixel id out of range");
  RenderJob j = job_of(cam, nx, ny, spp, depth, seed_base);
  j.npix = pixel_count;
  return render_host(c, j, pixel_ids, rgba_out, aux, stats);
}

rtp_status rtp_render_device(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t spp,
                             int32_t depth, uint32_t seed_base, int64_t pixel_begin, int64_t pixel_count,
                             const int64_t* d_pixel_ids, float* d_rgba_out, const rtp_pixel_aux* aux,
                             void* hip_stream, rtp_stats* stats) {
  RTP_TRY(check_render_args(c, cam, nx, ny, spp, depth));
  if (pixel_count < 0 || (pixel_count > 0 && !d_rgba_out))
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_render_device: bad output");
  if (!d_pixel_ids && (pixel_begin < 0 || pixel_begin + pixel_count > (int64_t)nx * ny))
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_render_device: pixel range outside the canvas");
  if (pixel_count == 0) return RTP_OK;
  RenderJob j = job_of(cam, nx, ny, spp, depth, seed_base);
  j.pixel_begin = pixel_begin, j.npix = pixel_count, j.d_ids = d_pixel_ids;
  j.d_out = d_rgba_out;
  return launch_device(c, j, aux, hip_stream, stats);
}

// rtp_render_device with a wave plan (include/rtp.h).
rtp_status rtp_render_planned_device(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t spp,
                                     int32_t depth, uint32_t seed_base, int64_t pixel_begin, int64_t pixel_count,
                                     const int64_t* d_pixel_ids, const int32_t* d_wave_begin, int32_t n_waves,
                                     float* d_rgba_out, const rtp_pixel_aux* aux, void* hip_stream, rtp_stats* stats) {
  RTP_TRY(check_render_args(c, cam, nx, ny, spp, depth));
  RTP_TRY(refuse_mesh(c, "rtp_render_planned_device"));
  if (pixel_count <= 0 || !d_rgba_out || !d_wave_begin || n_waves <= 0 || n_waves > (1 << 24))
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_render_planned_device: bad plan / output");
  if (!d_pixel_ids && (pixel_begin < 0 || pixel_begin + pixel_count > (int64_t)nx * ny))
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_render_planned_device: pixel range outside the canvas");
  {  // the plan must cover [0, pixel_count) exactly, in order, <= 128 entries per wave (one pool)
    HIP_TRY(hipSetDevice(c->device));
    std::vector<int32_t> plan((size_t)n_waves + 1);
    HIP_TRY(hipMemcpyAsync(plan.data(), d_wave_begin, plan.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                           (hipStream_t)hip_stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
    bool ok = plan[0] == 0 && plan[n_waves] == pixel_count;
    for (int32_t w = 0; ok && w < n_waves; w++) ok = plan[w] <= plan[w + 1] && plan[w + 1] - plan[w] <= rtp::kPoolSlots;
    if (!ok)
      return fail(RTP_ERR_INVALID_ARGUMENT,
                  "rtp_render_planned_device: wave_begin must rise from 0 to pixel_count in steps of at most 128");
  }
  RenderJob j = job_of(cam, nx, ny, spp, depth, seed_base);
  j.pixel_begin = pixel_begin, j.npix = pixel_count, j.d_ids = d_pixel_ids;
  j.d_out = d_rgba_out;
  j.d_wave_begin = d_wave_begin, j.plan_waves = n_waves;
  return launch_device(c, j, aux, hip_stream, stats);
}

// rtp_render_device over the rank's tiles of a round-robin 16x16 tile deal
// (shard.tile_pixels) without a pixel list: the kernel computes each entry's
// pixel, which saves the refill's gather of its id (C4's 1/8 share: 263 vs
// 276 ms on the same pixels, profiles/r04y_tiles_vs_list.txt).  Clipped edge
// tiles are rendered whole; their entries outside the canvas are ignored by
// the caller (shard.tile_entries): 0.7% more work on C4's 1080 rows.
rtp_status rtp_render_tiles_device(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t spp,
                                   int32_t depth, uint32_t seed_base, int32_t rank, int32_t world, float* d_rgba_out,
                                   void* hip_stream, rtp_stats* stats) {
  RTP_TRY(check_render_args(c, cam, nx, ny, spp, depth));
  RTP_TRY(refuse_mesh(c, "rtp_render_tiles_device"));
  if (world < 1 || rank < 0 || rank >= world)
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_render_tiles_device: rank outside [0, world)");
  const int64_t tx = (nx + 15) / 16, ty = (ny + 15) / 16;
  const int64_t tiles = tx * ty;
  // (the entries' pixel indices, up to 16 ty * nx, stay 32-bit in the kernel)
  if (tiles >= (1 << 24) || 16 * ty * (int64_t)nx >= ((int64_t)1 << 31))
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_render_tiles_device: canvas too large");
  const int64_t mine = tiles / world + (rank < tiles % world ? 1 : 0);
  if (mine == 0) return RTP_OK;
  if (!d_rgba_out) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_render_tiles_device: bad output");
  const int32_t tile[3] = {(int32_t)tx, world, rank};
  RenderJob j = job_of(cam, nx, ny, spp, depth, seed_base);
  j.npix = mine * 256, j.tile = tile;
  j.d_out = d_rgba_out;
  return launch_device(c, j, nullptr, hip_stream, stats);
}

// One more pass of spp samples over a render state (include/rtp.h): the pool
// kernel's kResume instances gather each entry's state and write it back.
rtp_status rtp_render_resume_device(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t spp,
                                    int32_t depth, int64_t pixel_begin, int64_t pixel_count,
                                    const int64_t* d_pixel_ids, const rtp_render_state* d_state, void* hip_stream,
                                    rtp_stats* stats) {
  RTP_TRY(check_resume_args(c, cam, nx, ny, spp, depth, d_state, "rtp_render_resume_device"));
  if (pixel_count < 0) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_render_resume_device: pixel_count < 0");
  if (!d_pixel_ids && (pixel_begin < 0 || pixel_begin + pixel_count > (int64_t)nx * ny))
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_render_resume_device: pixel range outside the canvas");
  if (stats) *stats = rtp_stats{};
  if (pixel_count == 0 || spp == 0) return RTP_OK;  // (no samples: the state stays as it is)
  RenderJob j = resume_job(cam, nx, ny, spp, depth, *d_state);
  j.pixel_begin = pixel_begin, j.npix = pixel_count, j.d_ids = d_pixel_ids;
  return launch_device(c, j, nullptr, hip_stream, stats);
}

// Host arrays, synchronous: the state is uploaded, resumed and copied back.
rtp_status rtp_render_resume(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t spp,
                             int32_t depth, const int64_t* pixel_ids, int64_t pixel_count,
                             const rtp_render_state* host_state, rtp_stats* stats) {
  RTP_TRY(check_resume_args(c, cam, nx, ny, spp, depth, host_state, "rtp_render_resume"));
  const int64_t npx = (int64_t)nx * ny;
  if (pixel_count < 0 || (!pixel_ids && pixel_count != npx))
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_render_resume: without a pixel list pixel_count must be nx * ny");
  for (int64_t i = 0; pixel_ids && i < pixel_count; i++)
    if (pixel_ids[i] < 0 || pixel_ids[i] >= npx)
      return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_render_resume: pixel id out of range");
  if (stats) *stats = rtp_stats{};
  if (pixel_count == 0 || spp == 0) return RTP_OK;
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)pixel_count;
  const rtp_render_state& hs = *host_state;
  DevBufs b;
  int64_t* d_ids = nullptr;
  rtp_render_state d{};
  HIP_TRY_AS("render_resume: device buffers", b.get(&d.rgba, n * 16, (const float*)hs.rgba));
  HIP_TRY_AS("render_resume: device buffers", b.get(&d.seed, n * 4, (const uint32_t*)hs.seed));
  if (hs.live_bounces)
    HIP_TRY_AS("render_resume: device buffers", b.get(&d.live_bounces, n * 4, (const uint32_t*)hs.live_bounces));
  if (hs.m2) HIP_TRY_AS("render_resume: device buffers", b.get(&d.m2, n * 4, (const float*)hs.m2));
  if (pixel_ids) HIP_TRY_AS("render_resume: device buffers", b.get(&d_ids, n * 8, pixel_ids));
  double ms = 0;
  RenderJob j = resume_job(cam, nx, ny, spp, depth, d);
  j.npix = pixel_count, j.d_ids = d_ids;
  j.kernel_ms = &ms;
  RTP_TRY(launch(c, j));
  HIP_TRY_AS("render_resume: copy back", DevBufs::back(hs.rgba, d.rgba, n * 16));
  HIP_TRY_AS("render_resume: copy back", DevBufs::back(hs.seed, d.seed, n * 4));
  HIP_TRY_AS("render_resume: copy back", DevBufs::back(hs.live_bounces, d.live_bounces, n * 4));
  HIP_TRY_AS("render_resume: copy back", DevBufs::back(hs.m2, d.m2, n * 4));
  fill_stats(stats, (uint64_t)pixel_count * (uint64_t)spp, ms);
  return RTP_OK;
}

}  // extern "C"

namespace {

// A free view-table slot of at least n views (rtp_context::ViewTable): one
// whose last launch has completed, else a new one; past 16 slots the call
// waits for the queued launches instead of growing further.
rtp_status acquire_view_table(rtp_context* c, int32_t n, size_t* slot) {
  auto usable = [&](rtp_context::ViewTable& t) {
    if (t.in_flight && hipEventQuery(t.used) == hipSuccess) t.in_flight = false;
    return !t.in_flight;
  };
  size_t pick = c->view_tables.size();
  for (size_t i = 0; i < c->view_tables.size() && pick == c->view_tables.size(); i++)
    if (usable(c->view_tables[i]) && c->view_tables[i].capacity >= n) pick = i;
  for (size_t i = 0; i < c->view_tables.size() && pick == c->view_tables.size(); i++)
    if (usable(c->view_tables[i])) pick = i;  // (too small: reallocated below)
  if (pick == c->view_tables.size() && c->view_tables.size() >= 16) {
    RTP_TRY(drain(c));
    for (rtp_context::ViewTable& t : c->view_tables) t.in_flight = false;
    pick = 0;
    for (size_t i = 1; i < c->view_tables.size(); i++)
      if (c->view_tables[i].capacity > c->view_tables[pick].capacity) pick = i;
  }
  if (pick == c->view_tables.size()) c->view_tables.emplace_back();
  rtp_context::ViewTable& t = c->view_tables[pick];
  if (!t.used) HIP_TRY(hipEventCreateWithFlags(&t.used, hipEventDisableTiming));
  if (t.capacity < n) {
    if (t.host) (void)hipHostFree(t.host);
    if (t.dev) (void)hipFree(t.dev);
    t.host = nullptr, t.dev = nullptr, t.capacity = 0;
    const int32_t cap = std::max(n, 256);
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&t.host), (size_t)cap * sizeof(rtp::DevView), hipHostMallocDefault));
    HIP_TRY(hipMalloc(&t.dev, (size_t)cap * sizeof(rtp::DevView)));
    t.capacity = cap;
  }
  *slot = pick;
  return RTP_OK;
}

// the batched launch unless the scene or the environment asks for the
// per-view loop (include/rtp.h rtp_render_views_device)
bool views_batched(const rtp_context* c) {
  return !c->use_bvh && !c->is_mesh && !env_is("RTP_KERNEL", '1') && !env_is("RTP_DEBUG_STATS", '1') &&
         !env_is("RTP_VIEWS_BATCH", '0');
}

rtp_status check_views_args(rtp_context* c, const rtp_view* views, int32_t n_views, int32_t nx, int32_t ny,
                            int32_t spp, int32_t depth) {
  if (!c || !views) return fail(RTP_ERR_INVALID_ARGUMENT, "render_views: NULL argument");
  if (n_views < 1) return fail(RTP_ERR_INVALID_ARGUMENT, "render_views: n_views must be >= 1");
  for (int32_t v = 0; v < n_views; v++) {
    RTP_TRY(check_render_args(c, &views[v].camera, nx, ny, spp, depth));
  }
  // (entries are 32-bit in the kernel)
  if ((int64_t)n_views * nx * ny > INT32_MAX)
    return fail(RTP_ERR_INVALID_ARGUMENT, "render_views: n_views * nx * ny exceeds 2^31-1 entries; render in batches");
  return RTP_OK;
}

// rtp_render_views_device behind its argument checks
rtp_status render_views_device(rtp_context* c, const rtp_view* views, int32_t n_views, int32_t nx, int32_t ny,
                               int32_t spp, int32_t depth, float* d_out, uint32_t* d_seed, uint32_t* d_live,
                               hipStream_t stream, double* kernel_ms) {
  const int64_t N = (int64_t)nx * ny;
  if (!views_batched(c)) {  // the per-view loop: one rtp_render_device each, at offset v * N
    double total = 0;
    for (int32_t v = 0; v < n_views; v++) {
      double ms = 0;
      RenderJob j = job_of(&views[v].camera, nx, ny, spp, depth, views[v].seed_base);
      j.npix = N;
      j.d_out = d_out + 4 * N * v;
      j.d_seed = d_seed ? d_seed + N * v : nullptr, j.d_live = d_live ? d_live + N * v : nullptr;
      j.stream = stream, j.kernel_ms = kernel_ms ? &ms : nullptr;
      RTP_TRY(launch(c, j));
      total += ms;
    }
    if (kernel_ms) *kernel_ms = total;
    return RTP_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  size_t slot = 0;
  RTP_TRY(acquire_view_table(c, n_views, &slot));
  rtp::DevView* const host = c->view_tables[slot].host;
  rtp::DevView* const dev = c->view_tables[slot].dev;
  for (int32_t v = 0; v < n_views; v++) {
    host[v] = rtp::DevView{};
    camera_setup(&views[v].camera, nx, ny, &host[v].cam);  // the host code of a single render
    host[v].seed_base = views[v].seed_base;
  }
  HIP_TRY(hipMemcpyAsync(dev, host, (size_t)n_views * sizeof(rtp::DevView), hipMemcpyHostToDevice, stream));
  c->view_tables[slot].in_flight = true;  // (from the upload on: the event below closes the slot's use)
  RenderJob j = job_of(nullptr, nx, ny, spp, depth, 0u);  // (cameras and seed bases are in the table)
  j.d_views = dev, j.npix = N * n_views;
  j.d_out = d_out, j.d_seed = d_seed, j.d_live = d_live;
  j.stream = stream, j.kernel_ms = kernel_ms;
  const rtp_status rs = launch(c, j);
  HIP_TRY(hipEventRecord(c->view_tables[slot].used, stream));
  return rs;
}

}  // namespace

extern "C" {

// n_views cameras in one launch (include/rtp.h): the pool kernel's kViews
// instances over the view-major entry list, or the per-view loop.
rtp_status rtp_render_views_device(rtp_context* c, const rtp_view* views, int32_t n_views, int32_t nx, int32_t ny,
                                   int32_t spp, int32_t depth, float* d_rgba_out, const rtp_pixel_aux* aux,
                                   void* hip_stream, rtp_stats* stats) {
  RTP_TRY(check_views_args(c, views, n_views, nx, ny, spp, depth));
  if (!d_rgba_out) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_render_views_device: bad output");
  double ms = 0;
  RTP_TRY(render_views_device(c, views, n_views, nx, ny, spp, depth, d_rgba_out, aux ? aux->final_seed : nullptr,
                              aux ? aux->live_bounces : nullptr, (hipStream_t)hip_stream, stats ? &ms : nullptr));
  fill_stats(stats, (uint64_t)n_views * (uint64_t)nx * (uint64_t)ny * (uint64_t)spp, ms);
  return RTP_OK;
}

rtp_status rtp_render_views(rtp_context* c, const rtp_view* views, int32_t n_views, int32_t nx, int32_t ny,
                            int32_t spp, int32_t depth, float* rgba_out, rtp_stats* stats) {
  RTP_TRY(check_views_args(c, views, n_views, nx, ny, spp, depth));
  if (!rgba_out) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_render_views: rgba_out is NULL");
  HIP_TRY(hipSetDevice(c->device));
  const int64_t n = (int64_t)n_views * nx * ny;
  DevBufs b;
  float* d_out = nullptr;
  uint32_t* d_live = nullptr;
  HIP_TRY_AS("render_views: device buffers", b.get(&d_out, (size_t)n * 16));
  HIP_TRY_AS("render_views: device buffers", b.get(&d_live, (size_t)n * 4));
  std::vector<uint32_t> live((size_t)n);
  double ms = 0;
  RTP_TRY(render_views_device(c, views, n_views, nx, ny, spp, depth, d_out, nullptr, d_live, nullptr, &ms));
  HIP_TRY_AS("render_views: copy back", DevBufs::back(rgba_out, d_out, (size_t)n * 16));
  HIP_TRY_AS("render_views: copy back", DevBufs::back(live.data(), d_live, (size_t)n * 4));
  fill_stats(stats, (uint64_t)n * (uint64_t)spp, ms);
  sum_stats(stats, rgba_out, live.data(), n);
  return RTP_OK;
}

// First-hit guides of the path camera (rtp_guides_kernel): one lane per pixel.
namespace {
rtp_status launch_guides(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, float* g0, float* g1,
                         int32_t* prim, hipStream_t stream, double* kernel_ms) {
  HIP_TRY(hipSetDevice(c->device));
  rtp::GuideParams p{};
  camera_setup(cam, nx, ny, &p.cam);
  p.nx = nx, p.ny = ny, p.npix = (int64_t)nx * ny;
  p.g0 = g0, p.g1 = g1, p.prim = prim;
  // (done is recorded: rtp_set_scene waits for it before it frees the scene)
  return timed_launch(c, stream, kernel_ms, true, [&]() -> rtp_status {
    HIP_TRY(rtp_launch_guides(c->d_scene, &p, c->use_bvh ? 1 : 0, stream));
    return RTP_OK;
  });
}
rtp_status check_guides_args(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, bool any_output) {
  RTP_TRY(check_render_args(c, cam, nx, ny, 0, 1));
  RTP_TRY(refuse_mesh(c, "render_guides"));
  if (!any_output) return fail(RTP_ERR_INVALID_ARGUMENT, "render_guides: every output is NULL");
  return RTP_OK;
}
}  // namespace

rtp_status rtp_render_guides_device(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, float* d_g0,
                                    float* d_g1, int32_t* d_prim, void* hip_stream, rtp_stats* stats) {
  RTP_TRY(check_guides_args(c, cam, nx, ny, d_g0 || d_g1 || d_prim));
  double ms = 0;
  RTP_TRY(launch_guides(c, cam, nx, ny, d_g0, d_g1, d_prim, (hipStream_t)hip_stream, stats ? &ms : nullptr));
  fill_stats(stats, (uint64_t)nx * ny, ms);
  return RTP_OK;
}

rtp_status rtp_render_guides(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, float* g0, float* g1,
                             int32_t* prim, rtp_stats* stats) {
  RTP_TRY(check_guides_args(c, cam, nx, ny, g0 || g1 || prim));
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)nx * ny;
  DevBufs b;
  float *d_g0 = nullptr, *d_g1 = nullptr;
  int32_t* d_prim = nullptr;
  if (g0) HIP_TRY_AS("render_guides: device buffers", b.get(&d_g0, 16 * n));
  if (g1) HIP_TRY_AS("render_guides: device buffers", b.get(&d_g1, 16 * n));
  if (prim) HIP_TRY_AS("render_guides: device buffers", b.get(&d_prim, 4 * n));
  double ms = 0;
  RTP_TRY(launch_guides(c, cam, nx, ny, d_g0, d_g1, d_prim, nullptr, &ms));
  HIP_TRY_AS("render_guides: copy back", DevBufs::back(g0, d_g0, 16 * n));
  HIP_TRY_AS("render_guides: copy back", DevBufs::back(g1, d_g1, 16 * n));
  HIP_TRY_AS("render_guides: copy back", DevBufs::back(prim, d_prim, 4 * n));
  fill_stats(stats, n, ms);
  return RTP_OK;
}

// Diagnostics: sums of the pool kernel's per-wave counters from the last launch
// made with RTP_DEBUG_STATS=1 (order of rtp::DbgCounter); returns the number
// of waves, 0 if none were recorded.
int32_t rtp_debug_counters(rtp_context* c, uint64_t* out, int32_t n_out) {
  if (!c || !c->d_dbg || !out) return 0;
  std::vector<unsigned long long> h((size_t)c->dbg_waves * rtp::kDbgCounters);
  if (hipMemcpy(h.data(), c->d_dbg, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  if (n_out < 0) {  // raw per-wave records: out must hold waves * kDbgCounters values
    std::memcpy(out, h.data(), h.size() * 8);
    return c->dbg_waves;
  }
  for (int k = 0; k < n_out && k < rtp::kDbgCounters; k++) {
    uint64_t acc = 0;
    for (int w = 0; w < c->dbg_waves; w++) acc += h[(size_t)w * rtp::kDbgCounters + k];
    out[k] = acc;
  }
  if (n_out > rtp::kDbgCounters) {  // extra slot: max wave lifetime
    uint64_t mx = 0;
    for (int w = 0; w < c->dbg_waves; w++) mx = std::max<uint64_t>(mx, h[(size_t)w * rtp::kDbgCounters + rtp::kDbgCyclesTotal]);
    out[rtp::kDbgCounters] = mx;
  }
  return c->dbg_waves;
}

rtp_status rtp_eval_primitive(rtp_context* c, int32_t kind, const void* in, void* out, int64_t n) {
  if (!c || !in || !out || n < 0 || kind < 0 || kind > 7)
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_eval_primitive: bad arguments");
  if (n == 0) return RTP_OK;
  HIP_TRY(hipSetDevice(c->device));
  const uint32_t* tab = nullptr;
  if (kind == 4 || kind == 5 || kind == 7) {
    const FfSnap ft = ff_tables(c->device, c->ff_policy, 0);
    tab = kind == 4 ? ft.t[1] : kind == 5 ? ft.t[0] : ft.direct;  // 16 / 32 dead depths, direct_first
    if (!tab) return fail(RTP_ERR_DEVICE, "rtp_eval_primitive: RNG jump tables are not built (policy or memory)");
  }
  const int dk = kind <= 3 ? kind : (kind == 6 ? 5 : 4);  // device kinds: 4 gather, 5 one dead step
  DevBufs b;
  void *din = nullptr, *dout = nullptr;
  HIP_TRY_AS("rtp_eval_primitive", b.get(&din, (size_t)n * 4, in));
  HIP_TRY_AS("rtp_eval_primitive", b.get(&dout, (size_t)n * 4));
  HIP_TRY_AS("rtp_eval_primitive",
             rtp_launch_eval_primitive(dk, din, dout, n, tab, which_threshold(2), which_threshold(3), nullptr));
  HIP_TRY_AS("rtp_eval_primitive", DevBufs::back(out, dout, (size_t)n * 4));
  return RTP_OK;
}

// Diagnostics: the closest hit of host rays with and without the quad
// prefilter (rtp_eval_closest_kernel; 7 u32 per ray).
rtp_status rtp_debug_closest_hit(rtp_context* c, const float* rays, int64_t n, uint32_t* out) {
  if (!c || !rays || !out || n < 0) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_debug_closest_hit: bad arguments");
  // (has_scene, not d_scene: the device scene exists from rtp_create on, and
  // names freed arrays after an rtp_set_scene whose upload failed)
  if (!c->has_scene) return fail(RTP_ERR_NO_SCENE, "rtp_debug_closest_hit: no scene set");
  if (n == 0) return RTP_OK;
  HIP_TRY(hipSetDevice(c->device));
  DevBufs b;
  float* din = nullptr;
  uint32_t* dout = nullptr;
  HIP_TRY_AS("rtp_debug_closest_hit", b.get(&din, (size_t)n * 24, rays));
  HIP_TRY_AS("rtp_debug_closest_hit", b.get(&dout, (size_t)n * 28));
  HIP_TRY_AS("rtp_debug_closest_hit", rtp_launch_eval_closest(c->d_scene, din, dout, n, c->is_mesh ? 3 : c->use_bvh ? 1 : 0, nullptr));
  HIP_TRY_AS("rtp_debug_closest_hit", DevBufs::back(out, dout, (size_t)n * 28));
  return RTP_OK;
}

// Diagnostics: one depth of the path kernel's bounce() for host rays and
// seeds (rtp_eval_bounce_kernel; 15 u32 per ray).
rtp_status rtp_debug_bounce(rtp_context* c, const float* rays, const uint32_t* seeds, int64_t n, uint32_t* out) {
  if (!c || !rays || !seeds || !out || n < 0) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_debug_bounce: bad arguments");
  if (!c->has_scene) return fail(RTP_ERR_NO_SCENE, "rtp_debug_bounce: no scene set");
  if (n == 0) return RTP_OK;
  HIP_TRY(hipSetDevice(c->device));
  DevBufs b;
  float* din = nullptr;
  uint32_t* dseed = nullptr;
  uint32_t* dout = nullptr;
  HIP_TRY_AS("rtp_debug_bounce", b.get(&din, (size_t)n * 24, rays));
  HIP_TRY_AS("rtp_debug_bounce", b.get(&dseed, (size_t)n * 4, seeds));
  HIP_TRY_AS("rtp_debug_bounce", b.get(&dout, (size_t)n * 60));
  HIP_TRY_AS("rtp_debug_bounce", rtp_launch_eval_bounce(c->d_scene, din, dseed, dout, n, c->is_mesh ? 3 : c->use_bvh ? 1 : 0, nullptr));
  HIP_TRY_AS("rtp_debug_bounce", DevBufs::back(out, dout, (size_t)n * 60));
  return RTP_OK;
}

// Diagnostics: the render kernels' camera_ray for host rows of (pixel, seed)
// under the DevCamera a render of this camera and canvas would launch with
// (rtp_eval_raygen_kernel; 12 u32 of camera constants, then 5 u32 per row).
rtp_status rtp_debug_raygen(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, const int64_t* pixels,
                            const uint32_t* seeds, int64_t n, uint32_t* out) {
  if (!c || !cam || !out || n < 0 || (n > 0 && (!pixels || !seeds)))
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_debug_raygen: bad arguments");
  RTP_TRY(check_canvas_camera(c, cam, nx, ny, "rtp_debug_raygen"));
  for (int64_t i = 0; i < n; i++)
    if (pixels[i] < 0 || pixels[i] >= (int64_t)nx * ny)
      return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_debug_raygen: pixel outside the canvas");
  rtp::DevCamera dc;
  camera_setup(cam, nx, ny, &dc);
  static_assert(sizeof(dc) == 48, "eye, nlook, delta_x, delta_y");
  std::memcpy(out, &dc, sizeof(dc));
  if (n == 0) return RTP_OK;
  HIP_TRY(hipSetDevice(c->device));
  DevBufs b;
  int64_t* dpix = nullptr;
  uint32_t* dseed = nullptr;
  uint32_t* dout = nullptr;
  HIP_TRY_AS("rtp_debug_raygen", b.get(&dpix, (size_t)n * 8, pixels));
  HIP_TRY_AS("rtp_debug_raygen", b.get(&dseed, (size_t)n * 4, seeds));
  HIP_TRY_AS("rtp_debug_raygen", b.get(&dout, (size_t)n * 20));
  HIP_TRY_AS("rtp_debug_raygen", rtp_launch_eval_raygen(&dc, nx, ny, dpix, dseed, dout, n, nullptr));
  HIP_TRY_AS("rtp_debug_raygen", DevBufs::back(out + 12, dout, (size_t)n * 20));
  return RTP_OK;
}

int32_t rtp_sphere_walk(rtp_context* c) {
  if (!c || !c->has_scene || !c->use_bvh) return 0;
  return c->lw_bytes > 0 ? 2 : 1;
}

int32_t rtp_sphere_walk_oct_mask(rtp_context* c) {
  if (!c || !c->has_scene || !c->use_bvh) return -1;
  // the value the kernels read: DevScene::oct_mask of the device copy (the
  // host field is a mirror, checked against it)
  int32_t dm = -1;
  if (hipSetDevice(c->device) != hipSuccess ||
      hipMemcpy(&dm, reinterpret_cast<const char*>(c->d_scene) + offsetof(rtp::DevScene, oct_mask), sizeof(dm),
                hipMemcpyDeviceToHost) != hipSuccess)
    return -2;
  return dm == c->oct_mask ? dm : -3;
}

// Diagnostics: exhaustive device check of a fast arithmetic sequence (kind,
// see rtp_verify_fast_math_kernel) over float bit patterns [lo_bits, hi_bits].
rtp_status rtp_verify_fast_math(rtp_context* c, int32_t kind, uint32_t lo_bits, uint32_t hi_bits,
                                uint64_t* mismatches, uint32_t* first_bad) {
  if (!c || !mismatches || hi_bits < lo_bits || kind < 0 || kind > 8)
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_verify_fast_math: bad args");
  HIP_TRY(hipSetDevice(c->device));
  unsigned long long* d_bad = nullptr;
  uint32_t* d_first = nullptr;
  HIP_TRY(hipMalloc(&d_bad, 8));
  HIP_TRY(hipMalloc(&d_first, 4));
  HIP_TRY(hipMemset(d_bad, 0, 8));
  HIP_TRY(hipMemset(d_first, 0xff, 4));
  const uint64_t total = (uint64_t)hi_bits - lo_bits + 1;
  const uint64_t chunk = 1ull << 30;
  for (uint64_t off = 0; off < total; off += chunk) {
    const uint64_t n = std::min<uint64_t>(chunk, total - off);
    HIP_TRY(rtp_launch_verify_fast_math(kind, lo_bits + (uint32_t)off, n, d_bad, d_first, nullptr));
  }
  unsigned long long bad = 0;
  uint32_t first = 0;
  HIP_TRY(hipMemcpy(&bad, d_bad, 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&first, d_first, 4, hipMemcpyDeviceToHost));
  (void)hipFree(d_bad);
  (void)hipFree(d_first);
  *mismatches = bad;
  if (first_bad) *first_bad = first;
  return RTP_OK;
}

rtp_status rtp_set_ff_tables(rtp_context* c, int32_t policy) {
  if (!c || policy < RTP_FF_TABLES_AUTO || policy > RTP_FF_TABLES_ON)
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_ff_tables: bad arguments");
  c->ff_policy = policy;
  if (policy == RTP_FF_TABLES_ON) {
    HIP_TRY(hipSetDevice(c->device));
    (void)ff_tables(c->device, policy, 0);  // build now, outside any timed render
  }
  return RTP_OK;
}

rtp_status rtp_get_ff_tables(rtp_context* c, rtp_ff_info* out) {
  if (!c || !out) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_get_ff_tables: bad arguments");
  std::lock_guard<std::mutex> lk(g_ff_mu);
  const FfTables& T = g_ff[c->device & 63];
  *out = rtp_ff_info{};
  out->policy = c->ff_policy;
  out->built = T.d_count > 0 ? 2 : T.n_chain > 0 ? 1 : 0;
  out->chain_tables = T.n_chain;
  out->direct_first = T.d_first;
  out->direct_count = T.d_count;
  out->bytes = T.bytes;
  out->alloc_ms = T.alloc_ms;
  out->build_ms = T.build_ms;
  out->samples_seen = T.samples_seen;
  uint64_t chain = 0, direct = 0;
  ff_auto_samples(chain, direct, &T);
  out->auto_samples = chain;
  out->auto_samples_direct = direct;
  return RTP_OK;
}

// NormalizeFunctor (main.cc:253-287): de-NaN rgb, then sqrt(c / spp) on all
// four channels.
rtp_status rtp_normalize(float* rgba, int64_t n, int32_t spp) {
  if (!rgba || n < 0) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_normalize: bad arguments");
  const float samplecount = (float)spp;
  for (int64_t i = 0; i < n; i++) {
    float* px = rgba + 4 * i;
    for (int k = 0; k < 3; k++)
      if (!(px[k] == px[k])) px[k] = 0;
    for (int k = 0; k < 4; k++) px[k] = std::sqrt(px[k] / samplecount);
  }
  return RTP_OK;
}

// save() (main.cc:325-384): P3 header "nx ny 255", one "r g b" line per
// pixel in buffer order (row 0 = camera bottom), int(255.99*c) unclamped,
// NaN pixels written as 0.
rtp_status rtp_write_pnm(const char* path, const float* rgba, int32_t nx, int32_t ny) {
  if (!path || !rgba || nx <= 0 || ny <= 0) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_write_pnm: bad arguments");
  FILE* f = std::fopen(path, "w");
  if (!f) return fail(RTP_ERR_INVALID_ARGUMENT, std::string("Couldn't save pnm: ") + path);
  std::fprintf(f, "P3\n%d %d 255\n", nx, ny);
  const int64_t n = (int64_t)nx * ny;
  for (int64_t i = 0; i < n; i++) {
    float c[3] = {rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2]};
    if ((c[0] != c[0]) || (c[1] != c[1]) || (c[2] != c[2])) c[0] = c[1] = c[2] = 0.0f;
    std::fprintf(f, "%d %d %d\n", (int)(255.99 * c[0]), (int)(255.99 * c[1]), (int)(255.99 * c[2]));
  }
  std::fclose(f);
  return RTP_OK;
}

}  // extern "C"
