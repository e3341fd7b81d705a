// rtp_context.hpp -- the rtp_context behind the C ABI (include/rtp.h),
// shared by the host units that touch a device: rtp_host.cpp (path mode),
// rtp_debug_host.cpp, rtp_direct_host.cpp (-direct mode), rtp_adaptive_host.cpp
// and the host half of rtp_denoise.hip.  (rtp_internal_fail: rtp_host_base.hpp)
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/rtp.h"

#include "rtp_layout.hpp"

struct rtp_context {
  int device = 0;
  rtp::DevScene* d_scene = nullptr;
  bool has_scene = false;
  float* d_hist = nullptr;
  size_t hist_bytes = 0;
  unsigned long long* d_dbg = nullptr;  // RTP_DEBUG_STATS=1: per-wave counters of the last launch
  int dbg_waves = 0;
  unsigned long long* d_progress = nullptr;  // global finished-sample counter of the pool kernel
  // many-sphere scenes: threaded BVH + sphere records (rtp_layout.hpp)
  rtp::BvhNode* d_nodes = nullptr;
  uint32_t* d_cnodes = nullptr;  // compact copy of d_nodes (the walks read it)
  int32_t* d_cidx = nullptr;     // scene index of each compact sphere leaf
  rtp::DevSphereG* d_sph_geom = nullptr;
  rtp::DevSphere* d_sph_all = nullptr;
  // the LDS walk's tree (rtp_layout.hpp kLdsWalkLeaf): compact nodes, their
  // embedded spheres' scene indices, leaf spheres (float4) and their indices
  uint32_t* d_lw_nodes = nullptr;
  int32_t* d_lw_cidx = nullptr;
  float* d_lw_sph = nullptr;
  int32_t* d_lw_orig = nullptr;
  int lw_bytes = 0;  // its LDS footprint (0: the scene has no LDS walk)
  bool use_bvh = false;
  // a mesh scene (rtp_set_scene_mesh): the quads behind their BVH in global
  // memory (DevScene::mesh_*), and the reach of its promise
  bool is_mesh = false;
  uint32_t* d_mesh_nodes = nullptr;
  rtp::DevQuad* d_mesh_quads = nullptr;
  float* d_mesh_shade = nullptr;
  float mesh_reach = 0.f;
  // for rtp_debug_mesh_readback: the tree's size, and each quad's padded box
  // (6 floats) and pad in the caller's order -- on the device after the device
  // build (rtp_set_scene_mesh_device), on the host after the host build
  int32_t n_mesh_nodes = 0, n_mesh_quads = 0;
  // rtp_mesh_counts: the triangle cells, and the cells with the unbounded box
  int32_t n_mesh_triangles = 0, n_mesh_unbounded = 0;
  float* d_mesh_boxes = nullptr;
  float* d_mesh_pads = nullptr;
  std::vector<float> h_mesh_boxes, h_mesh_pads;
  int oct_mask = 0;  // the global walk's octant mask (DevScene::oct_mask) of the current scene
  int ff_policy = 0;  // rtp_ff_policy (RNG jump tables)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // Completion of the last launch.  The history buffer and the progress
  // counter are per-context scratch, so a launch on any stream first waits
  // for the previous one, and the host waits before it frees or rewrites a
  // buffer a queued kernel may still read.
  hipEvent_t done = nullptr;
  bool pending = false;
  // View tables of the batched launches (rtp_render_views_device): a pinned
  // host image and its device copy per slot.  A slot is written by the host
  // and uploaded in stream order, so it is reused only once `used` (recorded
  // behind the launch that read it) has completed; calls queued back to back
  // each take a slot of their own.
  struct ViewTable {
    rtp::DevView* host = nullptr;
    rtp::DevView* dev = nullptr;
    int32_t capacity = 0;
    hipEvent_t used = nullptr;
    bool in_flight = false;
  };
  std::vector<ViewTable> view_tables;
  // -direct mode (rtp_direct_host.cpp): reference index of each kept
  // (de-duplicated) quad in DevQuad::orig order, the reference's quad count,
  // the quads' shape bounds, and device scratch for the per-call scalar
  // table and colour map
  std::vector<int32_t> kept_quads;
  int32_t n_ref_quads = 0;
  float quad_lo[3] = {0, 0, 0}, quad_hi[3] = {0, 0, 0};
  float* d_direct = nullptr;
  size_t direct_bytes = 0;
  // adaptive passes (rtp_adaptive_host.cpp): the selection's scratch (block
  // counts, total, ids) and the compact state of the selected entries; both
  // grow on demand, outlive rtp_set_scene like d_hist, and are ordered by
  // `done` like it.  adapt_ms: the parts of the last timed pass.
  void* d_adapt_sel = nullptr;
  size_t adapt_sel_bytes = 0;
  void* d_adapt_state = nullptr;
  size_t adapt_state_bytes = 0;
  double adapt_ms[4] = {0, 0, 0, 0};
};
