/*
 * rtp_adaptive.h -- adaptive sampling on the device (librtp.so): the second
 * header of the C ABI.  It includes rtp.h and adds the entry points that
 * refine a render state (rtp.h rtp_render_state) where it is noisy:
 *   noise    the relative standard error of each entry's mean luminance,
 *   select   the entries worth more samples, as an ascending id list built on
 *            the device (an ordered stream compaction),
 *   refine   one adaptive pass: select, gather the selected entries' state,
 *            the existing resume launch over the id list, scatter back.
 * rtp.h keeps its prototypes and RTP_ABI_VERSION; these symbols live in the
 * same library.
 *
 * All arithmetic below is float, in the order written, without contraction;
 * / and sqrtf are correctly rounded.  The results are these bits.
 *
 * Noise.  For an entry with rgb sums (sx, sy, sz), second moment m2 and
 * count (int32) samples:
 *   finite = isfinite(sx) && isfinite(sy) && isfinite(sz) && isfinite(m2)
 *   if (!finite || count < 2)            noise = +inf
 *   else nf = (float)count
 *        Y      = (0.2126f*sx + 0.7152f*sy) + 0.0722f*sz
 *        spread = m2 - (Y*Y)/nf
 *        s2     = (spread <= 1e-6f*m2) ? 0.f : spread/(nf - 1.f)
 *        sem    = sqrtf(s2/nf);  mean = Y/nf
 *        noise  = sem == 0.f ? 0.f : (mean > 0.f ? sem/mean : +inf)
 * (a spread within 1e-6 of m2 is the rounding of the float accumulations, not
 * variance: a pixel whose samples all have one luminance, a black one too,
 * gives 0).
 *
 * Selection.  An entry is active iff it is finite, noise > threshold, and
 * count <= max_spp - spp (max_spp < spp selects nothing).  An entry with fewer
 * than two samples and a finite state is active (its noise is +inf); a
 * non-finite entry never is: more samples cannot repair a NaN sum.
 */
#ifndef RTP_ADAPTIVE_H
#define RTP_ADAPTIVE_H

#include "rtp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  float threshold; /* select noise > threshold; >= 0, not NaN */
  int32_t spp;     /* samples a pass adds to a selected entry, 1..8388607 */
  int32_t max_spp; /* no entry grows past this count; >= 1 */
} rtp_refine_params;

/* d_sums: device float4[n]; d_m2: float[n]; d_count: int32[n] (all required);
 * d_noise: device float[n].  One lane per entry.  Asynchronous on hip_stream;
 * stats != NULL synchronises (kernel_ms).  RTP_ERR_INVALID_ARGUMENT, nothing
 * launched: a NULL pointer, n outside 1..2^31-1. */
rtp_status rtp_noise_device(rtp_context* ctx, const float* d_sums, const float* d_m2, const int32_t* d_count,
                            int64_t n, float* d_noise, void* hip_stream, rtp_stats* stats);
/* Host buffers, synchronous. */
rtp_status rtp_noise(rtp_context* ctx, const float* sums, const float* m2, const int32_t* count, int64_t n,
                     float* noise, rtp_stats* stats);

/* The active entries' indices in ascending order into d_ids (device
 * int64[n]; entries past the total are left untouched) and their number into
 * *d_n_selected (device int64).  Three launches -- count per block of 2048
 * entries, an exclusive scan of the block counts by one block, scatter by
 * rank -- none of which waits for another block; no atomics: the order is
 * part of the contract.  The state must not change between them.  The block
 * counts are the context's scratch (one host thread per context, rtp.h).
 * Asynchronous; stats != NULL synchronises (kernel_ms: the three launches).
 * RTP_ERR_INVALID_ARGUMENT, nothing launched: a NULL pointer, n outside
 * 1..2^31-1, params as for rtp_refine_device. */
rtp_status rtp_select_active_device(rtp_context* ctx, const float* d_sums, const float* d_m2, const int32_t* d_count,
                                    int64_t n, const rtp_refine_params* params, int64_t* d_ids,
                                    int64_t* d_n_selected, void* hip_stream, rtp_stats* stats);

/* One adaptive pass over the whole nx x ny canvas in buffer order.  d_state:
 * host struct of device arrays of nx*ny entries; rgba, seed and m2 are
 * required, live_bounces is nullable.  d_count: device int32[nx*ny], the
 * samples each entry has so far.  The pass selects, copies the 8-byte total
 * back on hip_stream and waits for it -- the resume launch is planned on the
 * host from the number of entries; this is the pass's ONE synchronisation --
 * writes the total to *n_selected (host), and when it is not 0 gathers the
 * selected entries' state into compact scratch, runs the resume launch of
 * rtp_render_resume_device over the id list with params->spp samples,
 * scatters the state back and adds spp to d_count of each selected entry;
 * those three are queued behind the wait and not waited for.  A selected
 * entry's state equals the state it would have after
 * rtp_render_resume_device(spp) over that pixel alone; an unselected entry's
 * state and count keep their bits: a pixel with count samples equals
 * rtp_render_pixels(spp = count).  The scratch (ids, compact state, block
 * counts, total) is the context's: it grows on demand, stays valid across
 * rtp_set_scene and is freed by rtp_destroy.  stats != NULL synchronises:
 * samples = total * spp, kernel_ms = the device time of the pass's launches
 * (rtp_refine_last_timing has its parts).
 * RTP_ERR_INVALID_ARGUMENT, nothing launched, state and count untouched: a
 * NULL d_state, rgba, seed, m2, d_count, params or n_selected; spp outside
 * 1..8388607; max_spp < 1; threshold NaN or negative; a bad camera or size;
 * depth < 1; RTP_KERNEL=1 or RTP_DEBUG_STATS=1 in the environment, as for
 * rtp_render_resume_device.  RTP_ERR_NO_SCENE without a scene. */
rtp_status rtp_refine_device(rtp_context* ctx, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t depth,
                             const rtp_render_state* d_state, int32_t* d_count, const rtp_refine_params* params,
                             int64_t* n_selected, void* hip_stream, rtp_stats* stats);
/* Host arrays (state and count of nx*ny entries), synchronous: uploaded,
 * refined by rtp_refine_device and copied back. */
rtp_status rtp_refine(rtp_context* ctx, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t depth,
                      const rtp_render_state* host_state, int32_t* count, const rtp_refine_params* params,
                      int64_t* n_selected, rtp_stats* stats);

/* rtp_refine_device repeated until a pass selects nothing or max_passes
 * (>= 1) passes have run.  selected_per_pass: host int64[max_passes], entry i
 * = what pass i selected (a final 0 included); *passes_run: how many entries
 * were written.  stats (nullable): the totals over the passes. */
rtp_status rtp_render_adaptive_device(rtp_context* ctx, const rtp_camera* cam, int32_t nx, int32_t ny, int32_t depth,
                                      const rtp_render_state* d_state, int32_t* d_count,
                                      const rtp_refine_params* params, int32_t max_passes,
                                      int64_t* selected_per_pass, int32_t* passes_run, void* hip_stream,
                                      rtp_stats* stats);

/* Diagnostics, NOT a stable interface (it serves tools/adaptive_bench.py and
 * may change or go without an ABI version bump; do not build on it): the
 * device time in ms of the parts of the context's last
 * rtp_refine_device call that was given stats: ms4[0] select (three
 * launches), [1] gather, [2] the resume launch, [3] scatter (0 for the parts
 * a pass that selected nothing did not run). */
rtp_status rtp_refine_last_timing(rtp_context* ctx, double* ms4);

/* Host helper: rtp_normalize with each pixel's own count -- rgb NaN -> 0, then
 * sqrt(c / (float)count[i]) on all four channels. */
rtp_status rtp_normalize_counts(float* rgba, const int32_t* count, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* RTP_ADAPTIVE_H */
