// rtp_host_util.hpp -- what the host translation units of librtp.so share
// (rtp_host.cpp, rtp_direct_host.cpp, rtp_adaptive_host.cpp, the host half of
// rtp_denoise.hip):
// error reporting, environment switches, device buffers of the synchronous
// entry points, the stats they fill, the timed launch, and the host vector
// math.  Internal: not installed, nothing here is device code.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "../../include/rtp.h"
#include "rtp_context.hpp"

namespace rtp_host {

// --------------------------------------------------------------- errors ---
inline rtp_status fail(rtp_status st, const std::string& msg) { return rtp_internal_fail(st, msg); }
inline rtp_status hip_fail(hipError_t e, const char* what) {
  return fail(e == hipErrorOutOfMemory ? RTP_ERR_OUT_OF_MEMORY : RTP_ERR_DEVICE,
              std::string(what) + ": " + hipGetErrorString(e));
}
// return from the enclosing function with the status of a failed HIP call,
// named by `what` (HIP_TRY: by its own text)
#define HIP_TRY_AS(what, expr)                        \
  do {                                                \
    hipError_t e_ = (expr);                           \
    if (e_ != hipSuccess) return hip_fail(e_, what);  \
  } while (0)
#define HIP_TRY(expr) HIP_TRY_AS(#expr, expr)
// likewise with the status of a failed step of the library's own (its message is set)
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

// ------------------------------------------------------------- launches ---
// wait for the context's last launch (rtp_context::done)
inline rtp_status drain(rtp_context* c) {
  if (c->pending) {
    HIP_TRY(hipEventSynchronize(c->done));
    c->pending = false;
  }
  return RTP_OK;
}

// One launch on `stream`, timed between the context's ev0 and ev1 when
// kernel_ms is asked for (the call then waits for the kernel).  `enqueue`
// returns an rtp_status.  With record_done the launch reads per-context state
// (the scene, the history): rtp_context::done is recorded behind it.
template <class Enqueue>
rtp_status timed_launch(rtp_context* c, hipStream_t stream, double* kernel_ms, bool record_done, Enqueue&& enqueue) {
  if (kernel_ms) HIP_TRY(hipEventRecord(c->ev0, stream));
  RTP_TRY(enqueue());
  if (record_done) {
    HIP_TRY(hipEventRecord(c->done, stream));
    c->pending = true;
  }
  if (kernel_ms) {
    HIP_TRY(hipEventRecord(c->ev1, stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *kernel_ms = ms;
  }
  return RTP_OK;
}

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

// ------------------------------------------------------- device buffers ---
// device copies of host buffers for the synchronous entry points, freed when
// the entry returns
struct DevBufs {
  static constexpr int kMax = 8;
  void* p[kMax] = {};
  int n = 0;
  DevBufs() = default;
  DevBufs(const DevBufs&) = delete;
  DevBufs& operator=(const DevBufs&) = delete;
  ~DevBufs() {
    for (int i = 0; i < n; i++)
      if (p[i]) (void)hipFree(p[i]);
  }
  // a device buffer of `bytes` in *out, filled from host when host != NULL
  template <class T>
  hipError_t get(T** out, size_t bytes, const T* host = nullptr) {
    if (n >= kMax) return hipErrorInvalidValue;
    hipError_t e = hipMalloc(&p[n], bytes);
    if (e != hipSuccess) return e;
    *out = static_cast<T*>(p[n++]);
    return host ? hipMemcpy(*out, host, bytes, hipMemcpyHostToDevice) : hipSuccess;
  }
  // device -> host (nothing where either is NULL: an output not asked for)
  static hipError_t back(void* host, const void* dev, size_t bytes) {
    return host && dev ? hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) : hipSuccess;
  }
};

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

// ------------------------------------------------------ argument checks ---
// the canvas and camera checks every render entry shares, in the reference's
// own words (Camera.cxx); `who` prefixes the library's own messages
inline rtp_status check_canvas_camera(const rtp_context* c, const rtp_camera* cam, int32_t nx, int32_t ny,
                                      const char* who) {
  if (!c->has_scene) return fail(RTP_ERR_NO_SCENE, std::string(who) + ": rtp_set_scene was not called");
  if (nx <= 0 || ny <= 0) return fail(RTP_ERR_INVALID_ARGUMENT, "Camera width/height must be greater than zero.");
  if ((int64_t)nx * ny > INT32_MAX) return fail(RTP_ERR_INVALID_ARGUMENT, std::string(who) + ": canvas too large");
  if (!(cam->fov_y_deg > 0)) return fail(RTP_ERR_INVALID_ARGUMENT, "Camera feild of view must be greater than zero.");
  if (cam->fov_y_deg > 180) return fail(RTP_ERR_INVALID_ARGUMENT, "Camera feild of view must be less than 180.");
  return RTP_OK;
}

// the index checks of a scene descriptor (rtp_set_scene and rtp_set_scene_mesh)
inline bool pt_ok(const rtp_scene_desc* s, int32_t id) { return id >= 0 && id < s->n_points; }
inline bool mat_ok(const rtp_scene_desc* s, int32_t m) {
  return m >= 0 && m < s->n_mat && s->mat_type[m] >= 0 && s->mat_type[m] <= 2;
}
inline bool tex_ok(const rtp_scene_desc* s, int32_t t) {
  return t >= 0 && t < s->n_tex_type && s->tex_type[t] >= 0 && s->tex_type[t] < s->n_tex;
}

}  // namespace rtp_host
