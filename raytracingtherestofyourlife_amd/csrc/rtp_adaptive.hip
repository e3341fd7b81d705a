// rtp_adaptive.hip -- the device side of adaptive sampling
// (include/rtp_adaptive.h): the noise estimate of a render state, the ordered
// stream compaction that selects the entries worth more samples, and the
// gather / scatter of their state around the existing resume launch.  Kernels
// and their launchers; the C ABI over them is rtp_adaptive_host.cpp.
//
// The arithmetic is the contract (rtp_adaptive.h states it operation by
// operation; tests/_adaptive_ref.py restates it in numpy float32 and the
// tests compare bits): float only, no contraction (-ffp-contract=off),
// correctly rounded division and sqrt.
//
// No kernel here waits for another block: the compaction is three launches
// (count, scan, scatter) ordered by the stream, with no look-back, ticket or
// grid barrier, and no atomics -- the ids come out ascending whatever the
// block scheduling.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rtp_adaptive.hpp"

namespace rtp {

__device__ __forceinline__ bool state_finite(const float4 s, const float m) {
  return __builtin_isfinite(s.x) && __builtin_isfinite(s.y) && __builtin_isfinite(s.z) && __builtin_isfinite(m);
}

// rtp_adaptive.h, "Noise", for a finite entry
__device__ __forceinline__ float noise_of(const float4 s, const float m, const int32_t c) {
  if (c < 2) return __builtin_inff();
  const float nf = (float)c;
  const float Y = (0.2126f * s.x + 0.7152f * s.y) + 0.0722f * s.z;
  const float spread = m - (Y * Y) / nf;
  const float s2 = (spread <= 1e-6f * m) ? 0.f : spread / (nf - 1.f);
  const float sem = __builtin_sqrtf(s2 / nf);
  const float mean = Y / nf;
  return sem == 0.f ? 0.f : (mean > 0.f ? sem / mean : __builtin_inff());
}

// One lane per entry.
__global__ void __launch_bounds__(256) rtp_noise_kernel(const float4* __restrict__ sums, const float* __restrict__ m2,
                                                        const int32_t* __restrict__ count, int64_t n,
                                                        float* __restrict__ noise) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 s = sums[i];
  const float m = m2[i];
  noise[i] = state_finite(s, m) ? noise_of(s, m, count[i]) : __builtin_inff();
}

// rtp_adaptive.h, "Selection" (28 bytes read per entry; false past the end)
__device__ __forceinline__ bool entry_active(const float4* __restrict__ sums, const float* __restrict__ m2,
                                             const int32_t* __restrict__ count, int64_t i, int64_t n,
                                             const SelectParams& p) {
  if (i >= n || !p.any) return false;
  const float4 s = sums[i];
  const float m = m2[i];
  const int32_t c = count[i];
  if (!state_finite(s, m) || c > p.count_limit) return false;
  return noise_of(s, m, c) > p.threshold;
}

// A block owns kSelBlock consecutive entries: in round k its thread t looks at
// entry base + k * kSelThreads + t, so a wave reads 64 consecutive entries and
// the entries' order is (round, wave, lane).

// (a) the block's number of active entries
__global__ void __launch_bounds__(kSelThreads) rtp_select_count_kernel(const float4* __restrict__ sums,
                                                                       const float* __restrict__ m2,
                                                                       const int32_t* __restrict__ count, int64_t n,
                                                                       SelectParams p,
                                                                       int32_t* __restrict__ block_count) {
  __shared__ int32_t wave_sum[kSelWaves];
  const int64_t base = (int64_t)blockIdx.x * kSelBlock;
  int32_t mine = 0;  // (wave-uniform)
#pragma unroll
  for (int k = 0; k < kSelRounds; k++) {
    const bool a = entry_active(sums, m2, count, base + k * kSelThreads + (int)threadIdx.x, n, p);
    mine += __popcll(__ballot(a));
  }
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t t = 0;
    for (int w = 0; w < kSelWaves; w++) t += wave_sum[w];
    block_count[blockIdx.x] = t;
  }
}

// (b) one block: block_count becomes its exclusive prefix sum, in place, a
// chunk of kScanThreads counts at a time (Hillis-Steele in LDS, the chunks
// chained by a running carry every thread keeps), and *total the sum.
__global__ void __launch_bounds__(kScanThreads) rtp_select_scan_kernel(int32_t* __restrict__ block_count, int32_t nb,
                                                                       int64_t* __restrict__ total) {
  __shared__ int32_t buf[2][kScanThreads];
  const int t = (int)threadIdx.x;
  int32_t carry = 0;
  for (int32_t c0 = 0; c0 < nb; c0 += kScanThreads) {
    const int32_t i = c0 + t;
    const int32_t v = i < nb ? block_count[i] : 0;
    int cur = 0;
    buf[0][t] = v;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
      int32_t x = buf[cur][t];
      if (t >= d) x += buf[cur][t - d];
      buf[cur ^ 1][t] = x;
      cur ^= 1;
      __syncthreads();
    }
    if (i < nb) block_count[i] = carry + (buf[cur][t] - v);
    carry += buf[cur][kScanThreads - 1];
    __syncthreads();  // (the next chunk rewrites buf)
  }
  if (t == 0) *total = (int64_t)carry;
}

// (c) the predicate again; an active entry's place is the block's offset, plus
// the active entries of the (round, wave) pairs before its own, plus the
// active lanes below it in its wave's ballot.
__global__ void __launch_bounds__(kSelThreads) rtp_select_scatter_kernel(const float4* __restrict__ sums,
                                                                         const float* __restrict__ m2,
                                                                         const int32_t* __restrict__ count, int64_t n,
                                                                         SelectParams p,
                                                                         const int32_t* __restrict__ block_offset,
                                                                         int64_t* __restrict__ ids) {
  __shared__ int32_t part[kSelRounds * kSelWaves];
  const int64_t base = (int64_t)blockIdx.x * kSelBlock;
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  unsigned long long bal[kSelRounds];
#pragma unroll
  for (int k = 0; k < kSelRounds; k++)
    bal[k] = __ballot(entry_active(sums, m2, count, base + k * kSelThreads + (int)threadIdx.x, n, p));
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kSelRounds; k++) part[k * kSelWaves + wave] = __popcll(bal[k]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t run = 0;
    for (int j = 0; j < kSelRounds * kSelWaves; j++) {
      const int32_t c = part[j];
      part[j] = run;
      run += c;
    }
  }
  __syncthreads();
  const int64_t first = block_offset[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kSelRounds; k++) {
    if (!((bal[k] >> lane) & 1ull)) continue;
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[k] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal[k], 0u));
    const int64_t dst = first + part[k * kSelWaves + wave] + (int64_t)below;
    // (dst < n always when the state did not change between (a) and (c); the
    // guard keeps a caller's mistake inside the id buffer)
    if (dst < n) ids[dst] = base + k * kSelThreads + (int)threadIdx.x;
  }
}

// One lane per selected entry: its state into the compact buffers.
__global__ void __launch_bounds__(256) rtp_state_gather_kernel(const int64_t* __restrict__ ids, int64_t total, int64_t n,
                                                               StatePtrs full, StatePtrs compact) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= total) return;
  const int64_t id = ids[k];
  if (id < 0 || id >= n) return;
  reinterpret_cast<float4*>(compact.rgba)[k] = reinterpret_cast<const float4*>(full.rgba)[id];
  compact.seed[k] = full.seed[id];
  if (full.live) compact.live[k] = full.live[id];
  compact.m2[k] = full.m2[id];
}

// ... and back, with the pass's samples added to the entry's count.
__global__ void __launch_bounds__(256) rtp_state_scatter_kernel(const int64_t* __restrict__ ids, int64_t total, int64_t n,
                                                                StatePtrs compact, StatePtrs full,
                                                                int32_t* __restrict__ count, int32_t spp) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= total) return;
  const int64_t id = ids[k];
  if (id < 0 || id >= n) return;
  reinterpret_cast<float4*>(full.rgba)[id] = reinterpret_cast<const float4*>(compact.rgba)[k];
  full.seed[id] = compact.seed[k];
  if (full.live) full.live[id] = compact.live[k];
  full.m2[id] = compact.m2[k];
  count[id] = count[id] + spp;
}

}  // namespace rtp

// ------------------------------------------------------------ launchers ---
extern "C" {

hipError_t rtp_launch_noise(const float* sums, const float* m2, const int32_t* count, int64_t n, float* noise,
                            hipStream_t stream) {
  hipLaunchKernelGGL(rtp::rtp_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     reinterpret_cast<const float4*>(sums), m2, count, n, noise);
  return hipGetLastError();
}

// block_count: int32[rtp::select_blocks(n)] scratch
hipError_t rtp_launch_select(const float* sums, const float* m2, const int32_t* count, int64_t n,
                             const rtp::SelectParams* p, int32_t* block_count, int64_t* ids, int64_t* total,
                             hipStream_t stream) {
  const int32_t nb = (int32_t)rtp::select_blocks(n);
  const float4* s4 = reinterpret_cast<const float4*>(sums);
  hipLaunchKernelGGL(rtp::rtp_select_count_kernel, dim3((unsigned)nb), dim3(rtp::kSelThreads), 0, stream, s4, m2, count,
                     n, *p, block_count);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rtp::rtp_select_scan_kernel, dim3(1), dim3(rtp::kScanThreads), 0, stream, block_count, nb, total);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rtp::rtp_select_scatter_kernel, dim3((unsigned)nb), dim3(rtp::kSelThreads), 0, stream, s4, m2,
                     count, n, *p, block_count, ids);
  return hipGetLastError();
}

hipError_t rtp_launch_state_gather(const int64_t* ids, int64_t total, int64_t n, const rtp::StatePtrs* full,
                                   const rtp::StatePtrs* compact, hipStream_t stream) {
  hipLaunchKernelGGL(rtp::rtp_state_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, ids,
                     total, n, *full, *compact);
  return hipGetLastError();
}

hipError_t rtp_launch_state_scatter(const int64_t* ids, int64_t total, int64_t n, const rtp::StatePtrs* compact,
                                    const rtp::StatePtrs* full, int32_t* count, int32_t spp, hipStream_t stream) {
  hipLaunchKernelGGL(rtp::rtp_state_scatter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, ids,
                     total, n, *compact, *full, count, spp);
  return hipGetLastError();
}

}  // extern "C"
