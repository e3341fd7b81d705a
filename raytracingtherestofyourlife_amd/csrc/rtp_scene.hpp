// rtp_scene.hpp -- the device-free build of an inline scene
// (rtp_scene_host.cpp): rtp_set_scene in steps, each working on the host only
// and free to refuse the description; rtp_host.cpp uploads what they built.
// No HIP header: tests/cpp/scene_build_check.cpp runs the steps without a
// device.  Internal.
#pragma once
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/rtp.h"
#include "rtp_layout.hpp"
#include "rtp_mesh.hpp"

// (internal to librtp.so: these names are no part of what the library exports)
#pragma GCC visibility push(hidden)
namespace rtp_host {

// smallest hash value with which >= w (PdfWorklet.h:20; which is monotone in
// the hash): the scene's thresholds, and the RNG jump tables' (rtp_ff_host.cpp)
uint32_t which_threshold(int w);

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

  // the host image zeroed, every octant its own walk order (the device LBVH
  // build keeps all 8; the host SAH build may narrow it, RTP_BVH_OCT_MASK)
  rtp::DevScene* fresh() {
    std::memset(h.get(), 0, sizeof(*h));
    h->oct_mask = 7;
    return h.get();
  }
};

// The quads: validated, de-duplicated, grouped by kind, with the prefilter
// tables and the -direct mode's bounds.
rtp_status scene_quads(const rtp_scene_desc* s, SceneBuild& B);
// The sphere records, whether they get a BVH, its pad's reach and its builder.
rtp_status scene_spheres(const rtp_scene_desc* s, SceneBuild& B);
// Where the spheres go: into the scene itself (few), or behind a BVH built on
// the device at upload (many) or here.  lds_walk_capacity: the bytes the LDS
// walk's tree may take (rtp_lds_walk_capacity of rtp_launch.hpp, passed in so
// that this unit needs nothing of a .hip file).
void scene_sphere_bvh(const rtp_scene_desc* s, SceneBuild& B, int lds_walk_capacity);
// lights, the glass constants and the `which` thresholds
rtp_status scene_lights(const rtp_scene_desc* s, SceneBuild& B);

}  // namespace rtp_host
#pragma GCC visibility pop
