// rtp_mesh.hpp -- the device-free builder of a mesh scene's quad BVH
// (rtp_mesh_host.cpp), used by rtp_set_scene_mesh (rtp_host.cpp).  Internal.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/rtp_mesh.h"
#include "rtp_layout.hpp"
#include "rtp_mesh_cell.hpp"

namespace rtp_host {

struct MeshBuild {
  int n_nodes = 0;                  // nodes per octant copy
  std::vector<rtp::BvhNode> nodes;  // 8 * n_nodes: one threaded copy per ray-direction octant
  std::vector<int32_t> order;       // leaf order: the caller's quad index of each stored quad
  std::vector<float> boxes;         // 6 per quad, the caller's order: the padded box (lo, hi)
  std::vector<float> pads;          // per quad: the pad (kMeshHuge: the unbounded box)
  float reach = 0.f;                // the promise's reach (kBvhReachFactor scene diagonals)
  int32_t n_triangles = 0;          // rtp_mesh_counts: the triangle cells (v11 == v01) ...
  int32_t n_unbounded = 0;          // ... and the cells with the unbounded box
};

// the descriptor checks of rtp_set_scene_mesh (rtp_set_scene's, and the mesh scene's counts)
rtp_status mesh_validate(const rtp_scene_desc* s);
// its parts, for the device build (rtp_set_scene_mesh_device), which makes the
// per-quad checks on the device: the counts; the message of the per-quad check
// that failed (0 point id, 1 material / texture, 2 vertex not finite); the
// spheres and lights; and mesh_build's refusal of bounds that are not finite
rtp_status mesh_validate_head(const rtp_scene_desc* s);
rtp_status mesh_quad_fail(int check);
rtp_status mesh_validate_tail(const rtp_scene_desc* s);
rtp_status mesh_bounds_fail();
// validate, pad, build (binned SAH, leaves of <= leaf_size quads) and thread the 8 octant copies
rtp_status mesh_build(const rtp_scene_desc* s, MeshBuild& out, int leaf_size = rtp::kMeshLeaf);
// BvhNodes -> the walk's 16-byte compact nodes (half-precision boxes rounded outward)
void mesh_compact(const rtp::BvhNode* nodes, int64_t total, uint32_t* out);
// One quad's DevQuad geometry (rtp_mesh_cell.hpp mesh_cell_record; the rest
// zeroed), for the inline scene and the light quad (mesh = false) and for
// mesh_records (true: a triangle cell is marked).
void fill_quad(rtp::DevQuad& Q, const float* q, const float* r, const float* s, const float* t, bool mesh);
// The records a host-built mesh scene is uploaded as: quads, one per quad in
// the build's leaf order, and shade, 8 floats per quad in the caller's order.
void mesh_records(const rtp_scene_desc* s, const MeshBuild& build, std::vector<rtp::DevQuad>& quads,
                  std::vector<float>& shade);
// Grows the box (lo, hi) by every quad vertex (quads) and by every sphere's
// c -+ r: the scene bounds whose diagonals are the reach (scene_reach).
void scene_bounds(const rtp_scene_desc* s, bool quads, float lo[3], float hi[3]);

}  // namespace rtp_host

// The builder for tests and stand-alone programs (exported from librtp.so, not
// part of rtp.h; no device is touched).  nodes (32 bytes each, at most
// node_cap; 2 * n_quads always suffice) receives octant `oct`'s copy, order
// the leaf order, boxes 6 floats per quad, pads one; guarantee: cos_min, reach.
// Every output is optional.
extern "C" rtp_status rtp_mesh_build_host(const rtp_scene_desc* scene, int32_t oct, int32_t node_cap, int32_t* n_nodes,
                                          void* nodes, int32_t* order, float* boxes, float* pads, float* guarantee);
// Internal test hooks, exported beside it and likewise no part of any public
// header: the leaf size the library was built with; mesh_compact over n
// BvhNodes; and a brute-force scan of a descriptor's quads on the host in
// float32 (the reference's quad test restated; tests/test_mesh_host.py holds
// every t it accepts to the oracle's quad_hit stage bit for bit).
extern "C" int32_t rtp_mesh_leaf_size(void);
extern "C" void rtp_mesh_compact_host(const void* nodes, int64_t n, uint32_t* out);
extern "C" rtp_status rtp_mesh_scan_host(const rtp_scene_desc* scene, const float* rays, int64_t n, uint32_t* out);
// The context's current mesh scene as its builder left it, host or device
// (rtp_debug_host.cpp): octant `oct`'s compact nodes (16 bytes each, at most
// node_cap), the leaf order (DevQuad::orig of each stored quad), and each
// quad's padded box (6 floats) and pad in the caller's order.  Every output is
// optional.
extern "C" rtp_status rtp_debug_mesh_readback(rtp_context* ctx, int32_t oct, int32_t node_cap, int32_t* n_nodes,
                                              void* cnodes, int32_t* order, float* boxes, float* pads);
// Likewise: the stored records themselves (rtp::DevQuad, 128 bytes each, at
// most cap of them) in leaf order -- a triangle cell's carries kMeshKindTri in
// its kind word whichever builder wrote it.  A hook of its own: a `records`
// argument on rtp_debug_mesh_readback would change the signature that
// existing callers of that hook bind.
extern "C" rtp_status rtp_debug_mesh_records(rtp_context* ctx, int64_t cap, void* records);

