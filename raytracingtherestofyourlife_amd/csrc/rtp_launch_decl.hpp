// rtp_launch_decl.hpp -- the one declaration of every extern "C" planner and
// launcher that a device unit defines and a host unit calls (none is part of
// a public header).  The defining units (rtp_launch.hpp, rtp_bvh_gpu.hip,
// rtp_direct.hip) include it as well as the callers, so a definition or a call
// that drifts from the declaration fails to compile instead of linking by name.
// Declarations only; what each does is written at its definition.  The mesh
// builders follow the same pattern in rtp_mesh.hpp and rtp_mesh_gpu.hpp, the
// adaptive passes in rtp_adaptive.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rtp_layout.hpp"

extern "C" {

// rtp_launch.hpp (rtp_kernels.hip): the instance table and the occupancy planning ...
const char* rtp_instance_name(int variant, int stats, int walk, int tiles, int plan, int steal, int views, int resume);
int64_t rtp_plan_history_lanes(int64_t npix, int spp, int bvh, int stats, int* variant_out, int* waves_out);
int rtp_plan_steal(int64_t npix, int bvh);
int rtp_lds_walk_capacity(void);
// ... the render and first-hit launches ...
hipError_t rtp_launch_render(const rtp::DevScene* scene, const rtp::KParams* p, int variant, int waves, int bvh,
                             int stats, int steal, hipStream_t stream, int lds_bytes);
hipError_t rtp_launch_guides(const rtp::DevScene* scene, const rtp::GuideParams* p, int bvh, hipStream_t stream);
// ... the stage evaluators of the tests ...
hipError_t rtp_launch_eval_primitive(int kind, const void* in, void* out, int64_t n, const uint32_t* tab, uint32_t t1,
                                     uint32_t t2, hipStream_t stream);
hipError_t rtp_launch_eval_closest(const rtp::DevScene* scene, const float* rays, uint32_t* out, int64_t n, int bvh,
                                   hipStream_t stream);
hipError_t rtp_launch_eval_bounce(const rtp::DevScene* scene, const float* rays, const uint32_t* seeds, uint32_t* out,
                                  int64_t n, int bvh, hipStream_t stream);
hipError_t rtp_launch_eval_raygen(const rtp::DevCamera* cam, int nx, int ny, const int64_t* pixels,
                                  const uint32_t* seeds, uint32_t* out, int64_t n, hipStream_t stream);
hipError_t rtp_launch_verify_fast_math(int kind, uint32_t lo, uint64_t count, unsigned long long* bad,
                                       uint32_t* first_bad, hipStream_t stream);
// ... and the RNG jump tables' build
hipError_t rtp_launch_build_ff_tables(const rtp::FfBuildOut* out, int max_r, uint32_t t1, uint32_t t2,
                                      hipStream_t stream);

// rtp_bvh_gpu.hip: the sphere BVH built and compacted on the device
hipError_t rtp_compact_bvh(const rtp::BvhNode* d_nodes, int64_t total, uint32_t* d_cn, int32_t* d_cidx,
                           hipStream_t stream);
hipError_t rtp_build_bvh_gpu(const float4* d_cr, int n, float3 lo, float3 ext, float reach, rtp::BvhNode* d_nodes,
                             rtp::DevSphereG* d_geom, hipStream_t stream);

// rtp_direct.hip: the -direct mode's render and its powf evaluator
hipError_t rtp_launch_direct(const rtp::DevScene* scene, const rtp::DirectParams* p, hipStream_t stream);
hipError_t rtp_launch_eval_powf(const float* x, float y, float* out, int64_t n, hipStream_t stream);

}  // extern "C"
