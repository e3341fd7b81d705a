// rtp_launch.hpp -- the host side of rtp_kernels.hip: the table of
// render-kernel instances, the occupancy planning over it, and the launchers
// (extern "C", declared in rtp_launch_decl.hpp; none is part of rtp.h).
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "rtp_diag.hpp"
#include "rtp_launch_decl.hpp"
#include "rtp_pool.hpp"

namespace {
// Which render kernel a launch runs: its modes as flags, and its sphere walk.
enum : unsigned { kStats = 1, kTiles = 2, kPlan = 4, kSteal = 8, kViews = 16, kResume = 32, kLockstep = 64 };
struct Instance {
  unsigned modes;
  int walk;  // the sphere BVH: 0 none, 1 the global threaded walk, 2 the LDS walk; 3: a mesh scene's quad BVH
  const void* fn;
  int threads;   // per block
  bool dyn_lds;  // takes the LDS walk's tree as dynamic LDS
  const char* name;
};
#define RTP_ROW(modes, walk, threads, dyn, ...) \
  {modes, walk, reinterpret_cast<const void*>(&rtp::__VA_ARGS__), threads, dyn, #__VA_ARGS__}
#define POOL(modes, walk, ...) RTP_ROW(modes, walk, 64 * rtp::kWavesPerBlock, false, __VA_ARGS__)
#define LDS(modes, ...) RTP_ROW(modes, 2, 64 * rtp::kLdsBvhWavesPerBlock, true, __VA_ARGS__)
// Every render-kernel instance there is; a mode without a row is refused.
// rtp_render_pool<kStats, kBvh, kTiles, kPlan, kSteal, kViews, kResume, kMesh>, rtp_render_pool_lds<kTiles, kSteal>.
const Instance kInstances[] = {
    // lockstep: a pixel list or range only
    RTP_ROW(kLockstep, 0, 256, false, rtp_render_lockstep<false>),
    RTP_ROW(kLockstep, 1, 256, false, rtp_render_lockstep<true>),
    // plain, with its stats builds
    POOL(0, 0, rtp_render_pool<false, false>),
    POOL(0, 1, rtp_render_pool<false, true>),
    POOL(kStats, 0, rtp_render_pool<true, false>),
    POOL(kStats, 1, rtp_render_pool<true, true>),
    // the tile deal
    POOL(kTiles, 0, rtp_render_pool<false, false, true>),
    POOL(kTiles, 1, rtp_render_pool<false, true, true>),
    // work stealing
    POOL(kSteal, 0, rtp_render_pool<false, false, false, false, true>),
    POOL(kSteal, 1, rtp_render_pool<false, true, false, false, true>),
    POOL(kSteal | kTiles, 0, rtp_render_pool<false, false, true, false, true>),
    POOL(kSteal | kTiles, 1, rtp_render_pool<false, true, true, false, true>),
    // a planned launch (no sphere BVH)
    POOL(kPlan, 0, rtp_render_pool<false, false, false, true>),
    POOL(kPlan | kStats, 0, rtp_render_pool<true, false, false, true>),
    // batched views (no sphere BVH)
    POOL(kViews, 0, rtp_render_pool<false, false, false, false, false, true>),
    POOL(kViews | kSteal, 0, rtp_render_pool<false, false, false, false, true, true>),
    // a pass over a render state
    POOL(kResume, 0, rtp_render_pool<false, false, false, false, false, false, true>),
    POOL(kResume, 1, rtp_render_pool<false, true, false, false, false, false, true>),
    POOL(kResume | kSteal, 0, rtp_render_pool<false, false, false, false, true, false, true>),
    POOL(kResume | kSteal, 1, rtp_render_pool<false, true, false, false, true, false, true>),
    // the sphere BVH walked out of LDS
    LDS(0, rtp_render_pool_lds<false, false>),
    LDS(kTiles, rtp_render_pool_lds<true, false>),
    LDS(kSteal, rtp_render_pool_lds<false, true>),
    LDS(kSteal | kTiles, rtp_render_pool_lds<true, true>),
    // a mesh scene (walk 3): {plain, stealing} x {render, resume}
    POOL(0, 3, rtp_render_pool<false, false, false, false, false, false, false, true>),
    POOL(kSteal, 3, rtp_render_pool<false, false, false, false, true, false, false, true>),
    POOL(kResume, 3, rtp_render_pool<false, false, false, false, false, false, true, true>),
    POOL(kResume | kSteal, 3, rtp_render_pool<false, false, false, false, true, false, true, true>),
};
#undef LDS
#undef POOL
#undef RTP_ROW

// the row of a mode, or null: no such instance
const Instance* find_instance(unsigned modes, int walk) {
  // The tile deal has no stats build: with RTP_DEBUG_STATS=1 it runs its
  // production instance (p.dbg still receives the waves' lifetime counters).
  if (modes == (kStats | kTiles) && walk != 2) modes = kTiles;
  for (const Instance& r : kInstances)
    if (r.modes == modes && r.walk == walk) return &r;
  return nullptr;
}
unsigned flag(bool on, unsigned f) { return on ? f : 0u; }

int blocks_per_cu(const Instance* r, size_t dyn) {
  int nb = 0;
  if (!r || hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, r->fn, r->threads, dyn) != hipSuccess || nb <= 0) nb = 1;
  return nb;
}
// (the occupancy of the LDS walk's instances at the largest tree: one block
// per CU; also sets their dynamic-LDS limit)
int lds_walk_blocks_per_cu() {
  static int cached = -1;
  if (cached > 0) return cached;
  const int dyn = rtp::kLdsWalkDynBytes;
  int nb = INT32_MAX;
  for (const Instance& r : kInstances) {
    if (!r.dyn_lds) continue;
    (void)hipFuncSetAttribute(r.fn, hipFuncAttributeMaxDynamicSharedMemorySize, dyn);
    nb = std::min(nb, blocks_per_cu(&r, (size_t)dyn));
  }
  cached = nb;
  return cached;
}
int device_cus(int* dev_out = nullptr) {  // 0: no device
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
  if (dev_out) *dev_out = dev;
  return cus;
}
// the waves of the plain instance <stats, walk> that fit the chip at once
int pool_resident_waves(bool stats, int walk) {
  static int cached[2][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}};
  int& c = cached[stats][walk];
  if (c > 0) return c;
  int dev = 0;
  const int cus = device_cus(&dev);
  if (cus == 0) return 1024;
  if (walk == 2) {
    c = cus * lds_walk_blocks_per_cu() * rtp::kLdsBvhWavesPerBlock;
    return c;
  }
  const int nb = blocks_per_cu(find_instance(flag(stats, kStats), walk), 0);
  c = cus * nb * rtp::kWavesPerBlock;
  if (const char* v = getenv("RTP_VERBOSE")) {
    if (v[0] == '1') {
      int lds_cu = 0;
      (void)hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev);
      hipFuncAttributes fa{};
      (void)hipFuncGetAttributes(&fa, find_instance(0, 0)->fn);
      fprintf(stderr, "rtp: pool kernel %d CUs x %d blocks of %d waves; LDS %zu B per block, %d B per CU; %d VGPRs\n",
              cus, nb, rtp::kWavesPerBlock, (size_t)fa.sharedSizeBytes, lds_cu, fa.numRegs);
    }
  }
  return c;
}
// Waves of the stealing instances that fit the chip at once: their own
// occupancy (the s_entry table adds 2 KiB of LDS per block), the smaller of
// the contiguous / pixel-list and tile-deal instances.  A stealing launch
// larger than this would leave blocks waiting for a free CU, and their
// statically assigned first entries would run as a tail after the stolen work.
int steal_resident_waves(int walk) {
  static int cached[3] = {-1, -1, -1};
  const int wk = walk == 3 ? 3 : walk ? 1 : 0;  // (a mesh scene has no tile-deal instance)
  int& c = cached[wk == 3 ? 2 : wk];
  if (c > 0) return c;
  const int cus = device_cus();
  if (cus == 0) return 1024;
  const int nb = wk == 3 ? blocks_per_cu(find_instance(kSteal, 3), 0)
                         : std::min(blocks_per_cu(find_instance(kSteal, wk), 0),
                                    blocks_per_cu(find_instance(kSteal | kTiles, wk), 0));
  c = cus * nb * rtp::kWavesPerBlock;
  return c;
}
int kernel_variant() {
  const char* e = getenv("RTP_KERNEL");
  if (e && e[0] == '1') return 1;
  return 2;
}
}  // namespace

// The printable name of a mode's instance, or null when there is none (the
// host's question "is there an LDS-walk instance for this launch?", and the
// table's test).  variant: 1 lockstep, 2 the pool kernel.
extern "C" const char* rtp_instance_name(int variant, int stats, int walk, int tiles, int plan, int steal, int views,
                                         int resume) {
  if (variant != 1 && variant != 2) return nullptr;
  const Instance* r = find_instance(flag(variant == 1, kLockstep) | flag(stats, kStats) | flag(tiles, kTiles) |
                                        flag(plan, kPlan) | flag(steal, kSteal) | flag(views, kViews) |
                                        flag(resume, kResume),
                                    walk);
  return r ? r->name : nullptr;
}

// Work plan: how many lanes' worth of attenuation history the launch needs.
extern "C" int64_t rtp_plan_history_lanes(int64_t npix, int spp, int bvh, int stats, int* variant_out,
                                          int* waves_out) {
  const int v = kernel_variant();
  if (variant_out) *variant_out = v;
  if (v == 1) {
    if (waves_out) *waves_out = (int)((npix + 63) / 64);
    return npix;
  }
  // pixels per wave when the launch cannot fill every resident wave: 80, so
  // that a lane often serves two pixels (the cheap pixels fill the lanes the
  // expensive ones' sample chains leave idle) while the waves per SIMD stay
  // few (each step of a chain is faster).  Rank 0's share of the C2 frame
  // under the N-rank tile deal, kernel ms (r03k/l, profiles/r03k_*):
  //   px/wave:  64    80    96    112   128
  //   N = 2:    95.5  83.6  86.5  79.0  88.7
  //   N = 4:    74.0  64.4  65.1  69.0  73.8
  //   N = 8:    58.7  58.6  59.2   --   65.0
  // (non-monotone: which pixels share a wave decides its longest chain).
  // Below a third of the resident waves at 64 pixels (C1, the 1/8 share)
  // the steps already run at one wave's latency: fewer waves gain nothing,
  // and a second pixel on a lane only lengthens its chain (C1: 0.70 -> 0.80
  // ms at 80), so such launches keep 64.  RTP_WAVE_PIXELS overrides
  // (experiments).
  // Long chains (spp >= 2048) on a share that fills 1.5-2.5 waves per SIMD
  // at 128 pixels per wave take 128: every pixel's chain is then ~2x the
  // average sample chain of a lane's two pixels, so the lanes stay full, and
  // fewer waves per SIMD make each step of the longest chains faster (the
  // per-step cost rises ~2.5 k cycles per extra wave on a SIMD, 13 k alone:
  // tools/lat_bench.hip).  C4's 1/8 share (259 200 pixels, 4096 spp), kernel
  // ms (r04c): 80 px/wave 388, 96 323, 112 354, 128 310.  C2's shares keep
  // 64/80 (1000 spp: 128 px/wave was 9-10% slower at N = 2, 4, 8).
  const int64_t resident = pool_resident_waves(stats != 0, bvh);
  const int64_t simds = std::max<int64_t>(1, resident / RTP_POOL_MIN_WAVES_PER_EU);
  int wave_px = (npix + 63) / 64 * 3 < resident ? 64 : 80;
  if (spp >= 2048 && npix * 2 >= simds * 128 * 3 && npix * 2 <= simds * 128 * 5) wave_px = 128;
  if (const char* e = getenv("RTP_WAVE_PIXELS")) wave_px = std::max(1, std::min(rtp::kPool, atoi(e)));
  const int64_t by_lanes = (npix + wave_px - 1) / wave_px;
  const int64_t by_pool = (npix + rtp::kPool - 1) / rtp::kPool;
  int64_t W = std::min<int64_t>(by_lanes, resident);
  W = std::max<int64_t>(W, by_pool);
  W = std::max<int64_t>(W, 1);
  if (waves_out) *waves_out = (int)W;
  return W * rtp::kPool;
}

// Work stealing (pool_body kSteal) when a launch's entries exceed what the
// resident waves' pools hold: the resident waves, each refilling its slots
// from the unclaimed entries.  Returns the waves (0: no stealing).
extern "C" int rtp_plan_steal(int64_t npix, int bvh) {
  const int64_t resident = pool_resident_waves(false, bvh);
  if (npix <= resident * rtp::kPool) return 0;
  if (bvh == 2) return (int)resident;  // (its instances' occupancy: lds_walk_blocks_per_cu)
  return std::min<int>((int)resident, steal_resident_waves(bvh));
}

// Bytes of LDS the LDS walk's tree may take (nodes of 8 octant copies plus
// the leaf spheres, 16 B each): what the 16-wave block leaves of the CU's 160 KiB.
extern "C" int rtp_lds_walk_capacity(void) { return std::max(0, rtp::kLdsWalkDynBytes); }

// The render launch.  The planner's choices arrive as arguments -- variant,
// waves, bvh (the sphere walk), stats, steal (rtp_plan_steal gave the waves) --
// and the rest of the mode is read off the launch's KParams.
extern "C" hipError_t rtp_launch_render(const rtp::DevScene* scene, const rtp::KParams* p, int variant, int waves,
                                        int bvh, int stats, int steal, hipStream_t stream, int lds_bytes) {
  if (p->npix <= 0) return hipSuccess;
  unsigned modes = flag(p->tile_world > 0, kTiles) | flag(p->views, kViews) | flag(p->resume, kResume);
  // (v1 has the global walk only and no stats build, and takes no wave plan)
  if (variant == 1) modes |= kLockstep;
  else modes |= flag(stats && p->dbg, kStats) | flag(p->wave_begin, kPlan) | flag(steal, kSteal);
  const Instance* r = find_instance(modes, variant == 1 && bvh ? 1 : bvh);
  if (!r) return hipErrorNotSupported;
  // what the mode does not say: a resume pass reads its seeds, batched views take no pixel list
  if ((p->resume && !p->seed_out) || (p->views && p->pixel_ids)) return hipErrorNotSupported;
  size_t dyn = 0;
  if (r->dyn_lds) {
    if (lds_bytes <= 0 || lds_bytes > rtp::kLdsWalkDynBytes) return hipErrorNotSupported;
    (void)lds_walk_blocks_per_cu();  // (sets the kernels' dynamic-LDS limit once)
    dyn = (size_t)lds_bytes;
  }
  const int per_block = variant == 1 ? r->threads : r->threads / 64;  // v1: a lane per entry; v2: waves
  const int64_t blocks = ((variant == 1 ? p->npix : (int64_t)waves) + per_block - 1) / per_block;
  void* args[] = {(void*)&scene, (void*)p, (void*)&waves};  // (v1 takes no waves)
  (void)hipLaunchKernel(r->fn, dim3((unsigned)blocks), dim3((unsigned)r->threads), args, dyn, stream);
  return hipGetLastError();
}

extern "C" hipError_t rtp_launch_eval_closest(const rtp::DevScene* scene, const float* rays, uint32_t* out,
                                              int64_t n, int bvh, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const dim3 g((unsigned)((n + 255) / 256)), b(256);
  if (bvh == 3) hipLaunchKernelGGL(rtp::rtp_eval_closest_mesh_kernel, g, b, 0, stream, scene, rays, out, n);
  else if (bvh) hipLaunchKernelGGL(rtp::rtp_eval_closest_kernel<true>, g, b, 0, stream, scene, rays, out, n);
  else hipLaunchKernelGGL(rtp::rtp_eval_closest_kernel<false>, g, b, 0, stream, scene, rays, out, n);
  return hipGetLastError();
}
extern "C" hipError_t rtp_launch_eval_bounce(const rtp::DevScene* scene, const float* rays, const uint32_t* seeds,
                                             uint32_t* out, int64_t n, int bvh, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const dim3 g((unsigned)((n + 255) / 256)), b(256);
  if (bvh == 3) hipLaunchKernelGGL(rtp::rtp_eval_bounce_mesh_kernel, g, b, 0, stream, scene, rays, seeds, out, n);
  else if (bvh) hipLaunchKernelGGL(rtp::rtp_eval_bounce_kernel<true>, g, b, 0, stream, scene, rays, seeds, out, n);
  else hipLaunchKernelGGL(rtp::rtp_eval_bounce_kernel<false>, g, b, 0, stream, scene, rays, seeds, out, n);
  return hipGetLastError();
}
extern "C" hipError_t rtp_launch_eval_raygen(const rtp::DevCamera* cam, int nx, int ny, const int64_t* pixels,
                                             const uint32_t* seeds, uint32_t* out, int64_t n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const dim3 g((unsigned)((n + 255) / 256)), b(256);
  hipLaunchKernelGGL(rtp::rtp_eval_raygen_kernel, g, b, 0, stream, *cam, nx, ny, pixels, seeds, out, n);
  return hipGetLastError();
}
extern "C" hipError_t rtp_launch_guides(const rtp::DevScene* scene, const rtp::GuideParams* p, int bvh,
                                        hipStream_t stream) {
  if (p->npix <= 0) return hipSuccess;
  const dim3 g((unsigned)((p->npix + 255) / 256)), b(256);
  if (bvh) hipLaunchKernelGGL(rtp::rtp_guides_kernel<true>, g, b, 0, stream, scene, *p);
  else hipLaunchKernelGGL(rtp::rtp_guides_kernel<false>, g, b, 0, stream, scene, *p);
  return hipGetLastError();
}

extern "C" hipError_t rtp_launch_build_ff_tables(const rtp::FfBuildOut* out, int max_r, uint32_t t1, uint32_t t2,
                                                 hipStream_t stream) {
  if (max_r < 1 || max_r >= rtp::kFfMaxSteps) return hipErrorInvalidValue;
  const uint64_t total = 1ull << 32, chunk = 1ull << 30;
  for (uint64_t base = 0; base < total; base += chunk) {
    hipLaunchKernelGGL(rtp::rtp_build_ff_tables_kernel, dim3((unsigned)(chunk / 256)), dim3(256), 0, stream, *out,
                       max_r, t1, t2, base, chunk);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

extern "C" hipError_t rtp_launch_eval_primitive(int kind, const void* in, void* out, int64_t n, const uint32_t* tab,
                                                uint32_t t1, uint32_t t2, hipStream_t stream) {
  const int block = 256;
  const int64_t grid = (n + block - 1) / block;
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(rtp::rtp_eval_primitive_kernel, dim3((unsigned)grid), dim3(block), 0, stream, kind, in, out, n,
                     tab, t1, t2);
  return hipGetLastError();
}
extern "C" hipError_t rtp_launch_verify_fast_math(int kind, uint32_t lo, uint64_t count, unsigned long long* bad,
                                                  uint32_t* first_bad, hipStream_t stream) {
  const int block = 256;
  const uint64_t grid = (count + block - 1) / block;
  if (grid == 0) return hipSuccess;
  hipLaunchKernelGGL(rtp::rtp_verify_fast_math_kernel, dim3((unsigned)grid), dim3(block), 0, stream, kind, lo, count,
                     bad, first_bad);
  return hipGetLastError();
}
