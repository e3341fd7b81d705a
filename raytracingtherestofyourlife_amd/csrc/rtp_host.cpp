// rtp_host.cpp -- host side of librtp.so: the contexts of the C ABI declared
// in include/rtp.h, their scenes and their renders.
//
// Mirrors vtkm::rendering::MapperPathTracer (MapperPathTracer.cxx:94-538):
// a context's life cycle, the upload of a built scene (the build itself:
// rtp_scene_host.cpp, rtp_mesh_host.cpp) and the render entry points with the
// camera set-up of pathtracing::Camera (Camera.cxx:437-474, 624-776, 879-960;
// rtp_host_base.hpp camera_setup).  The RNG jump tables are rtp_ff_host.cpp's,
// the diagnostics and test hooks rtp_debug_host.cpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtp.h"
#include "../../include/rtp_mesh.h"
#include "rtp_context.hpp"
#include "rtp_ff.hpp"
#include "rtp_host_util.hpp"
#include "rtp_launch_decl.hpp"
#include "rtp_layout.hpp"
#include "rtp_mesh.hpp"
#include "rtp_mesh_gpu.hpp"
#include "rtp_scene.hpp"

using namespace rtp_host;

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
// but the last works on the host only and may refuse the description
// (rtp_scene_host.cpp); the upload then replaces the context's scene.
namespace {

// what the host steps built (rtp_scene.hpp), and for a mesh scene built on the
// device (rtp_mesh_gpu.hip) the arrays themselves, which scene_upload adopts
struct SceneUpload : SceneBuild {
  bool mesh_on_device = false;
  rtp::MeshGpuOut mesh_dev;
};

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
rtp_status scene_upload(rtp_context* c, const rtp_scene_desc* s, SceneUpload& B) {
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
  SceneUpload B;
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
  scene_sphere_bvh(&hs, B, rtp_lds_walk_capacity());
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
  SceneUpload B;
  RTP_TRY(scene_quads(s, B));
  RTP_TRY(scene_spheres(s, B));
  scene_sphere_bvh(s, B, rtp_lds_walk_capacity());
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
  SceneUpload B;
  B.mesh = true;
  RTP_TRY(mesh_build(s, B.mb));
  rtp::DevScene* h = B.fresh();
  RTP_TRY(scene_spheres(s, B));  // (fewer than kBvhMinSpheres: no sphere BVH)
  scene_sphere_bvh(s, B, rtp_lds_walk_capacity());
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

}  // extern "C"
