// rtp_host_util.hpp -- what the host translation units of librtp.so that
// touch a device share (rtp_host.cpp, rtp_ff_host.cpp, rtp_debug_host.cpp,
// rtp_direct_host.cpp, rtp_adaptive_host.cpp, the host half of
// rtp_denoise.hip), on top of the device-free rtp_host_base.hpp: HIP error
// reporting, device buffers of the synchronous entry points, the timed launch
// and the canvas and camera checks of a context.  Internal: not installed,
// nothing here is device code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/rtp.h"
#include "rtp_context.hpp"
#include "rtp_host_base.hpp"

namespace rtp_host {

// --------------------------------------------------------------- errors ---
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

}  // namespace rtp_host
