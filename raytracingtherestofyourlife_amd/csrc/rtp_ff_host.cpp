// rtp_ff_host.cpp -- the RNG jump tables of the pool kernel: what is built,
// when (the AUTO policy) and for which launch (rtp_ff.hpp), and the C ABI's
// rtp_set_ff_tables / rtp_get_ff_tables (include/rtp.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "../../include/rtp.h"
#include "rtp_context.hpp"
#include "rtp_ff.hpp"
#include "rtp_host_util.hpp"
#include "rtp_launch_decl.hpp"
#include "rtp_layout.hpp"
#include "rtp_scene.hpp"

namespace rtp_host {

namespace {

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

}  // namespace

int ff_policy_default() {
  const char* e = getenv("RTP_FF_POLICY");
  if (e && !std::strcmp(e, "on")) return RTP_FF_TABLES_ON;
  if (e && !std::strcmp(e, "off")) return RTP_FF_TABLES_OFF;
  return RTP_FF_TABLES_AUTO;
}

namespace {

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

}  // namespace

// (FfSnap, and what ff_tables promises: rtp_ff.hpp)
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

}  // namespace rtp_host

using namespace rtp_host;

extern "C" {

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

}  // extern "C"
