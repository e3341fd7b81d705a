// rtp_denoise.hip -- the device side of a denoised preview (include/rtp.h):
// rtp_resolve* turns a render state into mean radiance and the variance of the
// mean, rtp_denoise* filters it with a variance-guided, edge-avoiding a-trous
// wavelet (Dammertz et al. 2010, in the style of SVGF's spatial filter) over
// the first-hit guides of rtp_render_guides*.  Kernels and their C ABI.
//
// The arithmetic is the contract (rtp.h states it operation by operation; the
// tests restate it in numpy float32 and compare bits): float only, no
// contraction (-ffp-contract=off), correctly rounded division and sqrt.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/rtp.h"
#include "rtp_context.hpp"
#include "rtp_layout.hpp"

namespace rtp {

// One lane per entry of the state.
__global__ void __launch_bounds__(256) rtp_resolve_kernel(const float4* __restrict__ sums, const float* __restrict__ m2,
                                                          const int32_t* __restrict__ count, int32_t spp, int64_t n,
                                                          float4* __restrict__ cv) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 s = sums[i];
  const int32_t c = count ? count[i] : spp;
  const float m = m2 ? m2[i] : 0.f;
  float4 o = make_float4(0.f, 0.f, 0.f, -1.f);
  const bool ok = c > 0 && __builtin_isfinite(s.x) && __builtin_isfinite(s.y) && __builtin_isfinite(s.z) &&
                  __builtin_isfinite(m);
  if (ok) {
    const float nf = (float)c;
    const float Y = (0.2126f * s.x + 0.7152f * s.y) + 0.0722f * s.z;
    const float l = Y / nf;
    float var;
    if (c == 1 || !m2) {
      var = l * l;
    } else {
      const float spread = m - (Y * Y) / nf;
      var = ((spread > 0.f ? spread : 0.f) / (nf - 1.f)) / nf;
    }
    o = make_float4(s.x / nf, s.y / nf, s.z / nf, var);
  }
  cv[i] = o;
}

// One level of the filter, one lane per pixel, a block = 64 x 4 pixels: each
// wave reads a 64-pixel row segment per tap, 1 KiB per 16-byte load, straight
// from global memory (the 5x5 footprints of a block overlap in L2 at the
// narrow steps; DESIGN.md has the measurements).  No LDS, no atomics.
constexpr int kAtrousBX = 64, kAtrousBY = 4;

template <bool kGuides>
__global__ void __launch_bounds__(kAtrousBX* kAtrousBY) rtp_atrous_kernel(AtrousParams p) {
  const int x = (int)blockIdx.x * kAtrousBX + (int)(threadIdx.x % kAtrousBX);
  const int y = (int)blockIdx.y * kAtrousBY + (int)(threadIdx.x / kAtrousBX);
  if (x >= p.nx || y >= p.ny) return;
  const float4* __restrict__ in = reinterpret_cast<const float4*>(p.in);
  const float4* __restrict__ g0 = reinterpret_cast<const float4*>(p.g0);
  const float4* __restrict__ g1 = reinterpret_cast<const float4*>(p.g1);
  const int64_t ip = (int64_t)y * p.nx + x;
  const float4 cp = in[ip];
  const bool vp = !(cp.w < 0.f);
  const float lp = (0.2126f * cp.x + 0.7152f * cp.y) + 0.0722f * cp.z;
  const float lden = p.sigma_l * __builtin_sqrtf(cp.w) + 1e-4f;  // (an invalid p never uses it)
  float4 np = make_float4(0.f, 0.f, 0.f, 0.f), ap = np;
  if (kGuides) np = g0[ip], ap = g1[ip];
  const bool hp = ap.w != 0.f;
  float sx = 0.f, sy = 0.f, sz = 0.f, sv = 0.f, sw = 0.f;
  constexpr float kH[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + p.step * dx, qy = y + p.step * dy;
      if (qx < 0 || qx >= p.nx || qy < 0 || qy >= p.ny) continue;
      float4 cq;
      float w;
      if (dx == 0 && dy == 0) {
        if (!vp) continue;
        cq = cp;
        w = 0.140625f;  // 9/64
      } else {
        const int64_t iq = (int64_t)qy * p.nx + qx;
        cq = in[iq];
        if (cq.w < 0.f) continue;
        w = kH[dx + 2] * kH[dy + 2];
        if (kGuides) {
          const float4 aq = g1[iq];
          const bool hq = aq.w != 0.f;
          if (hq != hp) {
            w = 0.f;
          } else if (hp) {
            const float4 nq = g0[iq];
            const float m = fmaxf(0.f, (np.x * nq.x + np.y * nq.y) + np.z * nq.z);
            float wn = m;
            for (int k = 0; k < p.normal_log2; k++) wn = wn * wn;
            const float dz = fabsf(np.w - nq.w) / p.sigma_z_step;
            const float wz = 1.f / (1.f + dz * dz);
            const float ax = ap.x - aq.x, ay = ap.y - aq.y, az = ap.z - aq.z;
            const float da = (ax * ax + ay * ay) + az * az;
            const float wa = 1.f / (1.f + da / p.sigma_a2);
            w = ((w * wn) * wz) * wa;
          }
        }
        if (vp) {
          const float lq = (0.2126f * cq.x + 0.7152f * cq.y) + 0.0722f * cq.z;
          const float dl = fabsf(lp - lq) / lden;
          w = w * (1.f / (1.f + dl * dl));
        }
      }
      sx = sx + w * cq.x;
      sy = sy + w * cq.y;
      sz = sz + w * cq.z;
      sv = sv + (w * w) * cq.w;
      sw = sw + w;
    }
  }
  float4 o = cp;
  if (sw > 0.f) o = make_float4(sx / sw, sy / sw, sz / sw, sv / (sw * sw));
  reinterpret_cast<float4*>(p.out)[ip] = o;
}

}  // namespace rtp

// ------------------------------------------------------------ host half ---
#include "rtp_host_util.hpp"

using namespace rtp_host;

namespace {

rtp_status bad(const char* msg) { return rtp_internal_fail(RTP_ERR_INVALID_ARGUMENT, msg); }

// [a, a + bytes) and [b, b + bytes) share a byte (NULL overlaps nothing)
bool overlap(const void* a, const void* b, size_t bytes) {
  if (!a || !b) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

rtp_status check_denoise(rtp_context* c, const float* cv, const float* g0, const float* g1, int32_t nx, int32_t ny,
                         const rtp_denoise_params* q, const float* out, const float* scratch, bool need_scratch) {
  if (!c || !cv || !q || !out || (need_scratch && !scratch)) return bad("rtp_denoise: NULL argument");
  if (nx <= 0 || ny <= 0 || (int64_t)nx * ny > INT32_MAX) return bad("rtp_denoise: bad canvas size");
  if (q->levels < 1 || q->levels > 8) return bad("rtp_denoise: levels must be 1..8");
  if (!(q->sigma_l > 0.f) || !(q->sigma_z > 0.f) || !(q->sigma_a > 0.f))
    return bad("rtp_denoise: sigma_l, sigma_z and sigma_a must be greater than zero");
  if (q->normal_log2 < 0 || q->normal_log2 > 8) return bad("rtp_denoise: normal_log2 must be 0..8");
  if ((g0 == nullptr) != (g1 == nullptr)) return bad("rtp_denoise: the guides g0 and g1 are given together or not at all");
  const size_t bytes = (size_t)nx * (size_t)ny * 16;
  const float* ins[3] = {cv, g0, g1};
  for (const float* in : ins)
    if (overlap(in, out, bytes) || overlap(in, scratch, bytes))
      return bad("rtp_denoise: out and scratch must not alias an input");
  if (overlap(out, scratch, bytes)) return bad("rtp_denoise: out and scratch must not alias each other");
  return RTP_OK;
}

// the L levels, ping-ponging between scratch and out so that the last lands in out
rtp_status launch_denoise(rtp_context* c, const float* cv, const float* g0, const float* g1, int32_t nx, int32_t ny,
                          const rtp_denoise_params* q, float* out, float* scratch, hipStream_t stream,
                          double* kernel_ms) {
  HIP_TRY(hipSetDevice(c->device));
  const dim3 grid((unsigned)((nx + rtp::kAtrousBX - 1) / rtp::kAtrousBX),
                  (unsigned)((ny + rtp::kAtrousBY - 1) / rtp::kAtrousBY)),
      block(rtp::kAtrousBX * rtp::kAtrousBY);
  // (these kernels read no per-context state: rtp_context::done is not recorded)
  return timed_launch(c, stream, kernel_ms, false, [&]() -> rtp_status {
    const float* src = cv;
    for (int s = 0; s < q->levels; s++) {
      rtp::AtrousParams p{};
      p.in = src, p.g0 = g0, p.g1 = g1;
      p.out = ((q->levels - 1 - s) % 2 == 0) ? out : scratch;
      p.nx = nx, p.ny = ny, p.step = 1 << s, p.normal_log2 = q->normal_log2;
      p.sigma_l = q->sigma_l;
      p.sigma_z_step = q->sigma_z * (float)p.step;
      p.sigma_a2 = q->sigma_a * q->sigma_a;
      if (g0) hipLaunchKernelGGL(rtp::rtp_atrous_kernel<true>, grid, block, 0, stream, p);
      else hipLaunchKernelGGL(rtp::rtp_atrous_kernel<false>, grid, block, 0, stream, p);
      HIP_TRY(hipGetLastError());
      src = p.out;
    }
    return RTP_OK;
  });
}

rtp_status launch_resolve(rtp_context* c, const float* sums, const float* m2, const int32_t* count, int32_t spp,
                          int64_t n, float* cv, hipStream_t stream, double* kernel_ms) {
  HIP_TRY(hipSetDevice(c->device));
  return timed_launch(c, stream, kernel_ms, false, [&]() -> rtp_status {
    hipLaunchKernelGGL(rtp::rtp_resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const float4*>(sums), m2, count, spp, n, reinterpret_cast<float4*>(cv));
    HIP_TRY(hipGetLastError());
    return RTP_OK;
  });
}

rtp_status check_resolve(rtp_context* c, const float* sums, int64_t n, const float* cv) {
  if (!c || !sums || !cv) return bad("rtp_resolve: NULL argument");
  if (n < 1 || n > INT32_MAX) return bad("rtp_resolve: the entry count must be 1..2^31-1");
  return RTP_OK;
}

}  // namespace

extern "C" {

rtp_status rtp_resolve_device(rtp_context* c, const float* d_sums, const float* d_m2, const int32_t* d_count,
                              int32_t spp, int64_t n, float* d_cv, void* hip_stream, rtp_stats* stats) {
  RTP_TRY(check_resolve(c, d_sums, n, d_cv));
  double ms = 0;
  RTP_TRY(launch_resolve(c, d_sums, d_m2, d_count, spp, n, d_cv, (hipStream_t)hip_stream, stats ? &ms : nullptr));
  fill_stats(stats, (uint64_t)n, ms);
  return RTP_OK;
}

rtp_status rtp_resolve(rtp_context* c, const float* sums, const float* m2, const int32_t* count, int32_t spp,
                       int64_t n, float* cv, rtp_stats* stats) {
  RTP_TRY(check_resolve(c, sums, n, cv));
  HIP_TRY(hipSetDevice(c->device));
  DevBufs b;
  float *ds = nullptr, *dm = nullptr, *dv = nullptr;
  int32_t* dc = nullptr;
  HIP_TRY(b.get(&ds, (size_t)n * 16, sums));
  if (m2) HIP_TRY(b.get(&dm, (size_t)n * 4, m2));
  if (count) HIP_TRY(b.get(&dc, (size_t)n * 4, count));
  HIP_TRY(b.get(&dv, (size_t)n * 16));
  double ms = 0;
  RTP_TRY(launch_resolve(c, ds, dm, dc, spp, n, dv, nullptr, &ms));
  HIP_TRY(DevBufs::back(cv, dv, (size_t)n * 16));
  fill_stats(stats, (uint64_t)n, ms);
  return RTP_OK;
}

rtp_status rtp_denoise_device(rtp_context* c, const float* d_cv, const float* d_g0, const float* d_g1, int32_t nx,
                              int32_t ny, const rtp_denoise_params* params, float* d_out, float* d_scratch,
                              void* hip_stream, rtp_stats* stats) {
  RTP_TRY(check_denoise(c, d_cv, d_g0, d_g1, nx, ny, params, d_out, d_scratch, true));
  double ms = 0;
  RTP_TRY(launch_denoise(c, d_cv, d_g0, d_g1, nx, ny, params, d_out, d_scratch, (hipStream_t)hip_stream,
                         stats ? &ms : nullptr));
  fill_stats(stats, (uint64_t)nx * (uint64_t)ny, ms);
  return RTP_OK;
}

rtp_status rtp_denoise(rtp_context* c, const float* cv, const float* g0, const float* g1, int32_t nx, int32_t ny,
                       const rtp_denoise_params* params, float* out, rtp_stats* stats) {
  RTP_TRY(check_denoise(c, cv, g0, g1, nx, ny, params, out, nullptr, false));
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = (size_t)nx * (size_t)ny * 16;
  DevBufs b;
  float *dv = nullptr, *d0 = nullptr, *d1 = nullptr, *dout = nullptr, *dscr = nullptr;
  HIP_TRY(b.get(&dv, bytes, cv));
  if (g0) {
    HIP_TRY(b.get(&d0, bytes, g0));
    HIP_TRY(b.get(&d1, bytes, g1));
  }
  HIP_TRY(b.get(&dout, bytes));
  HIP_TRY(b.get(&dscr, bytes));
  double ms = 0;
  RTP_TRY(launch_denoise(c, dv, d0, d1, nx, ny, params, dout, dscr, nullptr, &ms));
  HIP_TRY(DevBufs::back(out, dout, bytes));
  fill_stats(stats, (uint64_t)nx * (uint64_t)ny, ms);
  return RTP_OK;
}

}  // extern "C"
