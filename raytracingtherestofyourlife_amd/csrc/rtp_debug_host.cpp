// rtp_debug_host.cpp -- the diagnostics and test hooks of the C ABI
// (include/rtp.h, rtp_mesh.hpp): what the tests read out of a context or run
// on the device beside a render.  None of them changes a scene or a render.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/rtp.h"
#include "rtp_context.hpp"
#include "rtp_ff.hpp"
#include "rtp_host_util.hpp"
#include "rtp_launch_decl.hpp"
#include "rtp_layout.hpp"
#include "rtp_mesh.hpp"
#include "rtp_scene.hpp"

using namespace rtp_host;

extern "C" {

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

}  // extern "C"
