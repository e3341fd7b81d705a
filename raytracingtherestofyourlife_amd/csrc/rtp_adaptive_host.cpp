// rtp_adaptive_host.cpp -- the C ABI of include/rtp_adaptive.h over the
// kernels of rtp_adaptive.hip: argument checks, the context's scratch, and the
// adaptive pass, which composes the selection, the state gather, the existing
// resume launch (rtp_render_resume_device over the id list) and the scatter.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/rtp_adaptive.h"
#include "rtp_adaptive.hpp"
#include "rtp_context.hpp"
#include "rtp_host_util.hpp"
#include "rtp_layout.hpp"

using namespace rtp_host;

namespace {

rtp_status bad(const std::string& msg) { return fail(RTP_ERR_INVALID_ARGUMENT, msg); }

// ------------------------------------------------------------- checks ---
rtp_status check_entries(rtp_context* c, const void* sums, const void* m2, const void* count, int64_t n,
                         const void* out, const char* who) {
  if (!c || !sums || !m2 || !count || !out) return bad(std::string(who) + ": NULL argument");
  if (n < 1 || n > INT32_MAX) return bad(std::string(who) + ": the entry count must be 1..2^31-1");
  return RTP_OK;
}

rtp_status check_params(const rtp_refine_params* q, const char* who) {
  if (!q) return bad(std::string(who) + ": params is NULL");
  if (q->spp < 1 || q->spp > rtp::kMaxSpp) return bad(std::string(who) + ": params->spp must be 1..8388607");
  if (q->max_spp < 1) return bad(std::string(who) + ": params->max_spp must be >= 1");
  if (!(q->threshold >= 0.f)) return bad(std::string(who) + ": params->threshold must be >= 0");
  return RTP_OK;
}

// everything rtp_refine* refuses, before anything is launched
rtp_status check_refine(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t depth,
                        const rtp_render_state* st, const int32_t* count, const rtp_refine_params* q,
                        const int64_t* n_selected, const char* who) {
  if (!c || !cam) return bad(std::string(who) + ": NULL argument");
  RTP_TRY(check_canvas_camera(c, cam, nx, ny, who));
  if (depth < 1 || depth > rtp::kMaxDepth) return bad(std::string(who) + ": depthcount must be 1..16383");
  if (!st || !st->rgba || !st->seed || !st->m2)
    return bad(std::string(who) + ": state, state->rgba, state->seed and state->m2 are required");
  if (!count || !n_selected) return bad(std::string(who) + ": count and n_selected are required");
  RTP_TRY(check_params(q, who));
  if (env_is("RTP_KERNEL", '1')) return bad(std::string(who) + ": not available with RTP_KERNEL=1");
  if (env_is("RTP_DEBUG_STATS", '1')) return bad(std::string(who) + ": not available with RTP_DEBUG_STATS=1");
  return RTP_OK;
}

rtp::SelectParams select_params(const rtp_refine_params& q) {
  rtp::SelectParams p{};
  p.threshold = q.threshold;
  p.any = q.max_spp >= q.spp ? 1 : 0;
  p.count_limit = p.any ? q.max_spp - q.spp : 0;  // (both positive: no overflow)
  return p;
}

// ------------------------------------------------------------ scratch ---
// a context buffer of at least `need` bytes; growing waits for the queued
// launches that may still read the old one
rtp_status ensure(rtp_context* c, void*& p, size_t& have, size_t need) {
  if (need <= have) return RTP_OK;
  RTP_TRY(drain(c));
  if (p) HIP_TRY(hipFree(p));
  p = nullptr;
  have = 0;
  HIP_TRY(hipMalloc(&p, need));
  have = need;
  return RTP_OK;
}

// the selection's scratch: the total, the block counts, and (with_ids) the ids
struct SelScratch {
  int64_t* total = nullptr;
  int32_t* block_count = nullptr;
  int64_t* ids = nullptr;
};
rtp_status select_scratch(rtp_context* c, int64_t n, bool with_ids, SelScratch& s) {
  const size_t counts = ((size_t)rtp::select_blocks(n) * 4 + 7) & ~(size_t)7;
  RTP_TRY(ensure(c, c->d_adapt_sel, c->adapt_sel_bytes, 8 + counts + (with_ids ? (size_t)n * 8 : 0)));
  char* base = static_cast<char*>(c->d_adapt_sel);
  s.total = reinterpret_cast<int64_t*>(base);
  s.block_count = reinterpret_cast<int32_t*>(base + 8);
  s.ids = with_ids ? reinterpret_cast<int64_t*>(base + 8 + counts) : nullptr;
  return RTP_OK;
}

// the compact state of `total` selected entries
rtp_status compact_state(rtp_context* c, int64_t total, bool live, rtp::StatePtrs& s) {
  const size_t t = (size_t)total;
  RTP_TRY(ensure(c, c->d_adapt_state, c->adapt_state_bytes, t * 28));
  char* base = static_cast<char*>(c->d_adapt_state);
  s.rgba = reinterpret_cast<float*>(base);
  s.seed = reinterpret_cast<uint32_t*>(base + t * 16);
  s.m2 = reinterpret_cast<float*>(base + t * 20);
  s.live = live ? reinterpret_cast<uint32_t*>(base + t * 24) : nullptr;
  return RTP_OK;
}

// ---------------------------------------------------------------- jobs ---
// the three launches of the selection on `stream`, behind the context's last launch
rtp_status launch_select(rtp_context* c, const float* sums, const float* m2, const int32_t* count, int64_t n,
                         const rtp_refine_params& q, const SelScratch& s, int64_t* ids, int64_t* total,
                         hipStream_t stream, double* kernel_ms) {
  const rtp::SelectParams p = select_params(q);
  if (c->pending) HIP_TRY(hipStreamWaitEvent(stream, c->done, 0));
  return timed_launch(c, stream, kernel_ms, true, [&]() -> rtp_status {
    HIP_TRY(rtp_launch_select(sums, m2, count, n, &p, s.block_count, ids, total, stream));
    return RTP_OK;
  });
}

// One adaptive pass (rtp_adaptive.h rtp_refine_device); ms4, when given, takes
// the parts' device times and every part is waited for.
rtp_status refine_pass(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t depth,
                       const rtp_render_state& st, int32_t* d_count, const rtp_refine_params& q, int64_t* n_selected,
                       hipStream_t stream, double* ms4) {
  HIP_TRY(hipSetDevice(c->device));
  const int64_t n = (int64_t)nx * ny;
  SelScratch s;
  RTP_TRY(select_scratch(c, n, true, s));
  RTP_TRY(launch_select(c, st.rgba, st.m2, d_count, n, q, s, s.ids, s.total, stream, ms4 ? &ms4[0] : nullptr));
  // the pass's one synchronisation: the resume launch is planned from the total
  int64_t total = -1;
  HIP_TRY(hipMemcpyAsync(&total, s.total, 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (total < 0 || total > n) return fail(RTP_ERR_DEVICE, "rtp_refine: the selection's total is out of range");
  *n_selected = total;
  if (total == 0) return RTP_OK;
  rtp::StatePtrs full{st.rgba, st.seed, st.live_bounces, st.m2}, compact{};
  RTP_TRY(compact_state(c, total, st.live_bounces != nullptr, compact));
  RTP_TRY(timed_launch(c, stream, ms4 ? &ms4[1] : nullptr, true, [&]() -> rtp_status {
    HIP_TRY(rtp_launch_state_gather(s.ids, total, n, &full, &compact, stream));
    return RTP_OK;
  }));
  const rtp_render_state cs{compact.rgba, compact.seed, compact.live, compact.m2};
  rtp_stats rs{};
  RTP_TRY(rtp_render_resume_device(c, cam, nx, ny, q.spp, depth, 0, total, s.ids, &cs, stream, ms4 ? &rs : nullptr));
  if (ms4) ms4[2] = rs.kernel_ms;
  return timed_launch(c, stream, ms4 ? &ms4[3] : nullptr, true, [&]() -> rtp_status {
    HIP_TRY(rtp_launch_state_scatter(s.ids, total, n, &compact, &full, d_count, q.spp, stream));
    return RTP_OK;
  });
}

}  // namespace

extern "C" {

rtp_status rtp_noise_device(rtp_context* c, const float* d_sums, const float* d_m2, const int32_t* d_count,
                            int64_t n, float* d_noise, void* hip_stream, rtp_stats* stats) {
  RTP_TRY(check_entries(c, d_sums, d_m2, d_count, n, d_noise, "rtp_noise_device"));
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t stream = (hipStream_t)hip_stream;
  double ms = 0;
  // (reads no per-context state: rtp_context::done is not recorded)
  RTP_TRY(timed_launch(c, stream, stats ? &ms : nullptr, false, [&]() -> rtp_status {
    HIP_TRY(rtp_launch_noise(d_sums, d_m2, d_count, n, d_noise, stream));
    return RTP_OK;
  }));
  fill_stats(stats, (uint64_t)n, ms);
  return RTP_OK;
}

rtp_status rtp_noise(rtp_context* c, const float* sums, const float* m2, const int32_t* count, int64_t n, float* noise,
                     rtp_stats* stats) {
  RTP_TRY(check_entries(c, sums, m2, count, n, noise, "rtp_noise"));
  HIP_TRY(hipSetDevice(c->device));
  DevBufs b;
  float *ds = nullptr, *dm = nullptr, *dn = nullptr;
  int32_t* dc = nullptr;
  HIP_TRY(b.get(&ds, (size_t)n * 16, sums));
  HIP_TRY(b.get(&dm, (size_t)n * 4, m2));
  HIP_TRY(b.get(&dc, (size_t)n * 4, count));
  HIP_TRY(b.get(&dn, (size_t)n * 4));
  RTP_TRY(rtp_noise_device(c, ds, dm, dc, n, dn, nullptr, stats));
  HIP_TRY(DevBufs::back(noise, dn, (size_t)n * 4));
  return RTP_OK;
}

rtp_status rtp_select_active_device(rtp_context* c, const float* d_sums, const float* d_m2, const int32_t* d_count,
                                    int64_t n, const rtp_refine_params* params, int64_t* d_ids, int64_t* d_n_selected,
                                    void* hip_stream, rtp_stats* stats) {
  RTP_TRY(check_entries(c, d_sums, d_m2, d_count, n, d_ids, "rtp_select_active_device"));
  if (!d_n_selected) return bad("rtp_select_active_device: d_n_selected is NULL");
  RTP_TRY(check_params(params, "rtp_select_active_device"));
  HIP_TRY(hipSetDevice(c->device));
  SelScratch s;
  RTP_TRY(select_scratch(c, n, false, s));
  double ms = 0;
  RTP_TRY(launch_select(c, d_sums, d_m2, d_count, n, *params, s, d_ids, d_n_selected, (hipStream_t)hip_stream,
                        stats ? &ms : nullptr));
  fill_stats(stats, (uint64_t)n, ms);
  return RTP_OK;
}

rtp_status rtp_refine_device(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t depth,
                             const rtp_render_state* d_state, int32_t* d_count, const rtp_refine_params* params,
                             int64_t* n_selected, void* hip_stream, rtp_stats* stats) {
  RTP_TRY(check_refine(c, cam, nx, ny, depth, d_state, d_count, params, n_selected, "rtp_refine_device"));
  double ms4[4] = {0, 0, 0, 0};
  RTP_TRY(refine_pass(c, cam, nx, ny, depth, *d_state, d_count, *params, n_selected, (hipStream_t)hip_stream,
                      stats ? ms4 : nullptr));
  if (stats) {
    for (int k = 0; k < 4; k++) c->adapt_ms[k] = ms4[k];
    fill_stats(stats, (uint64_t)*n_selected * (uint64_t)params->spp, ms4[0] + ms4[1] + ms4[2] + ms4[3]);
  }
  return RTP_OK;
}

rtp_status rtp_refine(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t depth,
                      const rtp_render_state* host_state, int32_t* count, const rtp_refine_params* params,
                      int64_t* n_selected, rtp_stats* stats) {
  RTP_TRY(check_refine(c, cam, nx, ny, depth, host_state, count, params, n_selected, "rtp_refine"));
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)nx * (size_t)ny;
  const rtp_render_state& hs = *host_state;
  DevBufs b;
  rtp_render_state d{};
  int32_t* dc = nullptr;
  HIP_TRY_AS("refine: device buffers", b.get(&d.rgba, n * 16, (const float*)hs.rgba));
  HIP_TRY_AS("refine: device buffers", b.get(&d.seed, n * 4, (const uint32_t*)hs.seed));
  if (hs.live_bounces)
    HIP_TRY_AS("refine: device buffers", b.get(&d.live_bounces, n * 4, (const uint32_t*)hs.live_bounces));
  HIP_TRY_AS("refine: device buffers", b.get(&d.m2, n * 4, (const float*)hs.m2));
  HIP_TRY_AS("refine: device buffers", b.get(&dc, n * 4, (const int32_t*)count));
  int64_t total = 0;
  RTP_TRY(rtp_refine_device(c, cam, nx, ny, depth, &d, dc, params, &total, nullptr, stats));
  HIP_TRY(hipStreamSynchronize(nullptr));
  *n_selected = total;
  if (total == 0) return RTP_OK;  // (nothing changed)
  HIP_TRY_AS("refine: copy back", DevBufs::back(hs.rgba, d.rgba, n * 16));
  HIP_TRY_AS("refine: copy back", DevBufs::back(hs.seed, d.seed, n * 4));
  HIP_TRY_AS("refine: copy back", DevBufs::back(hs.live_bounces, d.live_bounces, n * 4));
  HIP_TRY_AS("refine: copy back", DevBufs::back(hs.m2, d.m2, n * 4));
  HIP_TRY_AS("refine: copy back", DevBufs::back(count, dc, n * 4));
  return RTP_OK;
}

rtp_status rtp_render_adaptive_device(rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t depth,
                                      const rtp_render_state* d_state, int32_t* d_count,
                                      const rtp_refine_params* params, int32_t max_passes, int64_t* selected_per_pass,
                                      int32_t* passes_run, void* hip_stream, rtp_stats* stats) {
  if (!selected_per_pass || !passes_run || max_passes < 1)
    return bad("rtp_render_adaptive_device: selected_per_pass, passes_run and max_passes >= 1 are required");
  RTP_TRY(check_refine(c, cam, nx, ny, depth, d_state, d_count, params, selected_per_pass,
                       "rtp_render_adaptive_device"));
  *passes_run = 0;
  rtp_stats sum{};
  for (int32_t i = 0; i < max_passes; i++) {
    rtp_stats one{};
    RTP_TRY(rtp_refine_device(c, cam, nx, ny, depth, d_state, d_count, params, &selected_per_pass[i], hip_stream,
                              stats ? &one : nullptr));
    sum.samples += one.samples;
    sum.kernel_ms += one.kernel_ms;
    *passes_run = i + 1;
    if (selected_per_pass[i] == 0) break;
  }
  if (stats) *stats = sum;
  return RTP_OK;
}

rtp_status rtp_refine_last_timing(rtp_context* c, double* ms4) {
  if (!c || !ms4) return bad("rtp_refine_last_timing: NULL argument");
  for (int k = 0; k < 4; k++) ms4[k] = c->adapt_ms[k];
  return RTP_OK;
}

// rtp_normalize (NormalizeFunctor, main.cc:253-287) with each pixel's own count
rtp_status rtp_normalize_counts(float* rgba, const int32_t* count, int64_t n) {
  if (!rgba || !count || n < 0) return bad("rtp_normalize_counts: bad arguments");
  for (int64_t i = 0; i < n; i++) {
    float* px = rgba + 4 * i;
    const float samplecount = (float)count[i];
    for (int k = 0; k < 3; k++)
      if (!(px[k] == px[k])) px[k] = 0;
    for (int k = 0; k < 4; k++) px[k] = std::sqrt(px[k] / samplecount);
  }
  return RTP_OK;
}

}  // extern "C"
