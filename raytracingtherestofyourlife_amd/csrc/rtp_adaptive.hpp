// rtp_adaptive.hpp -- what rtp_adaptive.hip (kernels, launchers) and
// rtp_adaptive_host.cpp (the C ABI of include/rtp_adaptive.h) share: the
// compaction's geometry, the kernels' argument structs, the launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rtp {

// the selection: a block of kSelThreads threads owns kSelBlock consecutive
// entries, kSelRounds per thread; one block of kScanThreads scans the counts
constexpr int kSelThreads = 256, kSelRounds = 8, kSelBlock = kSelThreads * kSelRounds, kSelWaves = kSelThreads / 64;
constexpr int kScanThreads = 256;
inline int64_t select_blocks(int64_t n) { return (n + kSelBlock - 1) / kSelBlock; }

// rtp_refine_params as the predicate reads it
struct SelectParams {
  float threshold;
  int32_t count_limit;  // max_spp - spp: an entry with more samples is full
  int32_t any;          // 0: max_spp < spp, nothing is selected
};

// a render state's arrays (rtp_render_state; live nullable)
struct StatePtrs {
  float* rgba;
  uint32_t* seed;
  uint32_t* live;
  float* m2;
};

}  // namespace rtp

extern "C" {
hipError_t rtp_launch_noise(const float* sums, const float* m2, const int32_t* count, int64_t n, float* noise,
                            hipStream_t stream);
hipError_t rtp_launch_select(const float* sums, const float* m2, const int32_t* count, int64_t n,
                             const rtp::SelectParams* p, int32_t* block_count, int64_t* ids, int64_t* total,
                             hipStream_t stream);
hipError_t rtp_launch_state_gather(const int64_t* ids, int64_t total, int64_t n, const rtp::StatePtrs* full,
                                   const rtp::StatePtrs* compact, hipStream_t stream);
hipError_t rtp_launch_state_scatter(const int64_t* ids, int64_t total, int64_t n, const rtp::StatePtrs* compact,
                                    const rtp::StatePtrs* full, int32_t* count, int32_t spp, hipStream_t stream);
}
