// rtp_mesh_gpu.hpp -- the device builder of a mesh scene's quad BVH
// (rtp_mesh_gpu.hip), used by rtp_set_scene_mesh_device (rtp_host.cpp).
// Internal.  Vertices and connectivity stay on the device; the host sees one
// small record (MeshGpuInfo) and the node count.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rtp_layout.hpp"

namespace rtp {

// the caller's device arrays and the library's small tables (device copies)
struct MeshGpuIn {
  const float* points;  // float3[n_points]
  int32_t n_points;
  const int32_t* quad_points;  // int32[4 * n_quads]
  const int32_t* quad_mat;
  const int32_t* quad_tex;
  int32_t n_quads;
  // mat_type[m] where it is a material type (0..2), else -1; tex_type[t] where
  // it names a texture (0..n_tex-1), else -1: mat_ok / tex_ok are "in range
  // and >= 0"
  const int32_t* mat_chk;
  int32_t n_mat;
  const int32_t* tex_chk;
  int32_t n_tex_type;
  const float* tex_rgb;  // float3[n_tex]
};

// which check of mesh_validate a quad failed (its order per quad)
enum MeshGpuFail : uint32_t { kMeshFailPoint = 0, kMeshFailMaterial = 1, kMeshFailFinite = 2 };
constexpr uint32_t kMeshNoFail = 0xffffffffu;

// The record the device leaves for the host.  Floats are kept as ordered
// unsigned keys (rtp_mesh_cell.hpp mesh_key_float decodes) so that atomic min / max apply.
struct MeshGpuInfo {
  uint32_t first_fail;  // min over the failing quads of (q << 2 | MeshGpuFail); kMeshNoFail: none
  uint32_t lo[3], hi[3];    // min / max over all quad vertices
  uint32_t clo[3], chi[3];  // min / max over the box centres (the Morton codes' frame; device only)
  uint32_t n_triangles;     // k_boxes: the triangle cells (v11 == v01) ...
  uint32_t n_unbounded;     // ... and the cells whose box is unbounded (rtp_mesh_counts)
  uint32_t pad[1];
};
static_assert(sizeof(MeshGpuInfo) == 64, "one small record");

// what the build leaves: the three arrays of DevScene::mesh_* and, for
// rtp_debug_mesh_readback, each quad's padded box and pad (caller's order)
struct MeshGpuOut {
  uint32_t* nodes = nullptr;  // 8 * n_nodes compact nodes
  DevQuad* quads = nullptr;   // n_quads, leaf order
  float* shade = nullptr;     // 8 floats per quad, caller's order
  float* boxes = nullptr;     // 6 floats per quad, caller's order
  float* pads = nullptr;      // 1 float per quad
  int32_t n_nodes = 0;        // per octant copy
  int32_t n_triangles = 0;    // MeshGpuInfo's counts, read back with the root
  int32_t n_unbounded = 0;
};

}  // namespace rtp

// Step 1: validate every quad and bound the vertices (one pass); `info` is
// the record, copied back.  Enqueued on `stream`, which it synchronises.
extern "C" hipError_t rtp_mesh_gpu_validate(const rtp::MeshGpuIn* in, rtp::MeshGpuInfo* info, hipStream_t stream);
// Step 2: records, Morton keys, sort, radix tree, boxes, the 8 flattened
// compact copies and the gathered quads, with `reach` from the host (the
// spheres are folded in there).  Allocates `out`'s arrays; on failure they are
// freed and `out` is cleared.  Temporaries are freed before it returns.
// status: 0, or 1 when the tree did not close within the round limit.
extern "C" hipError_t rtp_mesh_gpu_build(const rtp::MeshGpuIn* in, float reach, rtp::MeshGpuOut* out, int32_t* status,
                                         hipStream_t stream);
extern "C" void rtp_mesh_gpu_free(rtp::MeshGpuOut* out);
