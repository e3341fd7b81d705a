// rtp_host_base.hpp -- what every host translation unit of librtp.so shares
// and that needs no device: error reporting, environment switches, the stats
// the entry points fill, the host vector math, the camera set-up and the index
// checks of a scene descriptor.  No HIP header is included here: the
// device-free units (rtp_scene_host.cpp, rtp_mesh_host.cpp, rtp_base_host.cpp)
// include this file and not rtp_host_util.hpp, which adds what touches a device.
// Internal: not installed.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "../../include/rtp.h"
#include "rtp_layout.hpp"

// thread-local last-error message of the C ABI (rtp_base_host.cpp)
rtp_status rtp_internal_fail(rtp_status st, const std::string& msg);

namespace rtp_host {

// --------------------------------------------------------------- errors ---
inline rtp_status fail(rtp_status st, const std::string& msg) { return rtp_internal_fail(st, msg); }
// return from the enclosing function with the status of a failed step of the
// library's own (its message is set)
#define RTP_TRY(expr)                \
  do {                               \
    const rtp_status rs_ = (expr);   \
    if (rs_ != RTP_OK) return rs_;   \
  } while (0)

// ---------------------------------------------------------- environment ---
// first character of an environment variable (0: unset or empty)
inline char env_char(const char* name) {
  const char* e = getenv(name);
  return e ? e[0] : '\0';
}
inline bool env_is(const char* name, char ch) { return env_char(name) == ch; }

// ---------------------------------------------------------------- stats ---
inline void fill_stats(rtp_stats* stats, uint64_t samples, double ms) {
  if (!stats) return;
  *stats = rtp_stats{};
  stats->samples = samples;
  stats->kernel_ms = ms;
}
// adds a copied-back frame's live bounces and NaN pixels (rgb) to the stats
inline void sum_stats(rtp_stats* stats, const float* rgba, const uint32_t* live, int64_t n) {
  if (!stats) return;
  for (int64_t i = 0; i < n; i++) {
    stats->live_bounces += live[i];
    const float* px = rgba + 4 * i;
    stats->nan_pixels += (std::isnan(px[0]) || std::isnan(px[1]) || std::isnan(px[2])) ? 1 : 0;
  }
}

// ----------------------------------------------------- host vector math ---
// (compiled with -ffp-contract=off; these feed bit-exact results: the
// operations and their order are the reference's)
struct v3 {
  float x, y, z;
};
inline v3 add(v3 a, v3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline v3 sub(v3 a, v3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline v3 scl(v3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline float dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline v3 cross(v3 a, v3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline v3 normalize(v3 a) { return scl(a, 1 / std::sqrt(dot(a, a))); }  // vtkm::Normalize (CPU build)
inline v3 ld(const float* p) { return {p[0], p[1], p[2]}; }
inline void st(float* d, v3 a) { d[0] = a.x, d[1] = a.y, d[2] = a.z; }
constexpr float kPi180f = 0.01745329251994329577f;  // vtkm::Pi_180f()

// --------------------------------------------------------- camera set-up ---
// (the render entries of rtp_host.cpp and rtp_debug_raygen of rtp_debug_host.cpp)
// pathtracing::Camera::SetParameters -> CreateRaysImpl -> RayGen ctor
__attribute__((visibility("hidden"))) inline void camera_setup(const rtp_camera* cam, int32_t nx, int32_t ny, rtp::DevCamera* out) {
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

// ------------------------------------------------------ argument checks ---
// the index checks of a scene descriptor (rtp_set_scene and rtp_set_scene_mesh)
inline bool pt_ok(const rtp_scene_desc* s, int32_t id) { return id >= 0 && id < s->n_points; }
inline bool mat_ok(const rtp_scene_desc* s, int32_t m) {
  return m >= 0 && m < s->n_mat && s->mat_type[m] >= 0 && s->mat_type[m] <= 2;
}
inline bool tex_ok(const rtp_scene_desc* s, int32_t t) {
  return t >= 0 && t < s->n_tex_type && s->tex_type[t] >= 0 && s->tex_type[t] < s->n_tex;
}

}  // namespace rtp_host
