// rtp_pool.hpp -- the two CDNA4 (gfx950) render kernels of the path-tracing
// hot path, over the per-ray code of rtp_trace.hpp.
//
// Both kernels run the fused per-depth stage sequence of SURVEY.md 3.2 (one
// call of bounce() == one depth of MapperPathTracer.cxx:286-305 for one ray)
// and differ only in how work is mapped to lanes:
//
//  v1  rtp_render_lockstep: one lane per pixel; the lane walks its pixel's
//      samples and depths in order (MapperPathTracer.cxx:278-354).  Lanes of
//      a wave stay on the same depth, so a wave executes a live bounce as long
//      as ANY of its 64 paths is alive -- kept as the simple reference mapping.
//
//  v2  rtp_render_pool (default): persistent waves.  Each wave owns a pool of
//      pixels in LDS (RNG state, colour sum, sample count).  A lane always
//      carries a LIVE path: when its path ends, the lane banks the sample's
//      contribution into the pixel's slot, queues the pixel for the RNG
//      fast-forward of its remaining dead depths, and immediately starts the
//      next sample of a READY pixel.  The fast-forwards (pure integer Wang
//      hashing) run in full-wave batches when the READY queue
//      runs dry.  Per-pixel sample order, draw order and summation order are
//      exactly the reference's; only the interleaving across pixels changes.
//
// Scene and light data are wave-uniform and arrive through a const __restrict__
// kernel argument, so the compiler reads them with scalar loads into SGPRs.
// The only per-lane global memory traffic is the attenuation history needed
// by the reference's back-to-front radiance product (MapperPathTracer.cxx:
// 328-348), stored depth-major [d][lane] like the reference's ChannelBuffers.
#pragma once
#include "rtp_trace.hpp"

// One compiled path.  The alternatives measured and rejected in rounds 1-2
// (and the RTP_DUP cost-attribution probes behind DESIGN.md 4.1's tables) are
// in git history: `git show c9f7859:raytracingtherestofyourlife_amd/csrc/
// rtp_kernels.hip`.  The numeric scheduling constants below stay tunable.
#ifndef RTP_FF_MARGIN
#define RTP_FF_MARGIN 12  // pool kernel: fast-forward when READY holds fewer than idle lanes + this
#endif
// history rows of a finished sample loaded together in the fast-forward batch
#ifndef RTP_HIST_PREFETCH
#define RTP_HIST_PREFETCH 6
#endif
constexpr int kHistPrefetch = RTP_HIST_PREFETCH;
// and the rest kHistChunk at a time (r03r: 4 rows per wait, -0.4% at N = 1,
// -1.1% at the 1/8 share, against two per wait)
#ifndef RTP_HIST_CHUNK
#define RTP_HIST_CHUNK 4
#endif
constexpr int kHistChunk = RTP_HIST_CHUNK;
#ifndef RTP_WALK_DONE
// pool kernel, sphere-BVH scenes: a loop iteration walks the BVH until this
// many of the wave's paths have finished their walks (or all have)
#define RTP_WALK_DONE 48
#endif
#ifndef RTP_CRIT_FF
#define RTP_CRIT_FF 100  // pool kernel: lag (per mille of the wave's average samples) that makes a pixel critical
#endif
#ifndef RTP_BVH_NT
#define RTP_BVH_NT 0  // (experiment: the walk's node gathers as non-temporal loads)
#endif
#ifndef RTP_POOL
#define RTP_POOL 128  // pixel slots per wave (kPool)
#endif
// Issue-priority balancing: the SIMD arbiter favours older waves, so with a
// static split of pixels the youngest wave of each SIMD finished ~1/3 later
// than the oldest, and the SIMD ran its last milliseconds with one or two
// waves (little latency hiding).  Every kPrioPeriod finished samples a wave publishes
// its finished samples to a global counter and sets s_setprio from how far
// its own completed fraction lags the global one.
#ifndef RTP_PRIO_BALANCE
#define RTP_PRIO_BALANCE 1
#endif
#ifndef RTP_PRIO_THR
#define RTP_PRIO_THR 0.0002f
#endif
#ifndef RTP_PRIO_PERIOD
#define RTP_PRIO_PERIOD 128
#endif
constexpr int kPrioPeriod = RTP_PRIO_PERIOD;
#ifndef RTP_POOL_MIN_WAVES_PER_EU
#define RTP_POOL_MIN_WAVES_PER_EU 5
#endif
// gfx950 allocates VGPRs in granules of 8: 5 waves per SIMD need <= 96.  The
// waves-per-EU hint alone settles at 102 (4 waves); the hard cap costs one
// spilled 64-bit value (16 B of scratch).
#ifndef RTP_POOL_MAX_VGPR
#define RTP_POOL_MAX_VGPR 96
#endif

namespace rtp {

// ------------------------------------------------------------------ v1 ---
template <bool kBvh>
__global__ void __launch_bounds__(256) rtp_render_lockstep(const DevScene* __restrict__ sc, KParams p) {
  __shared__ __align__(16) float s_qshade[kQTableFloats];
  fill_qshade(sc, s_qshade);
  __syncthreads();
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.npix) return;
  const int64_t pix = pixel_of(p, k);
  const uint32_t t1 = sc->which_t1, t2 = sc->which_t2;
  uint32_t seed = p.seed_base + (uint32_t)pix;  // seeds[i] = i (MapperPathTracer.cxx:265-267)
  float cr = 0.f, cg = 0.f, cb = 0.f;
  uint32_t live = 0;
  const int pi = (int32_t)pix % p.nx, pj = (int32_t)pix / p.nx;
  float4* __restrict__ hist = reinterpret_cast<float4*>(p.hist) + k;
  const int64_t stride = p.npix;
  const int D = p.depth;
  for (int s = 0; s < p.spp; s++) {
    Path ps;
    ps.dir = camera_ray(p.cam, pi, pj, p.nx, p.ny, seed);
    ps.org = ld3(p.cam.eye);
    ps.nonfinite = false;
    int result = kAlive, k_end = D;
    f3 emit = mk(0.f, 0.f, 0.f);
    for (int d = 0; d < D; d++) {
      if (result != kAlive) {
        seed = dead_step(seed, t1, t2);
        continue;
      }
      live++;
      ps.d = d;
      result = bounce<kBvh>(sc, ps, seed, emit, hist + (int64_t)d * stride, D, nullptr, s_qshade);
      if (result != kAlive) k_end = d;
    }
    f3 c = path_radiance(result, k_end, emit, ps.nonfinite, hist, stride);
    cr = cr + c.x;
    cg = cg + c.y;
    cb = cb + c.z;
  }
  reinterpret_cast<float4*>(p.out)[k] = make_float4(cr, cg, cb, 0.f);
  if (p.seed_out) p.seed_out[k] = seed;
  if (p.live_out) p.live_out[k] = live;
}

// ------------------------------------------------------------------ v2 ---
constexpr int kWavesPerBlock = 4;
constexpr int kPool = RTP_POOL;  // pixel slots per wave (power of two: queue index = cursor & (kPool-1))
static_assert(kPool == kPoolSlots || RTP_POOL != 128, "rtp_layout.hpp kPoolSlots is the production pool size");
static_assert((kPool & (kPool - 1)) == 0 && kPool >= 64, "pool size must be a power of two >= 64");
// A wave's pool in LDS: one array of kPool per field, in this order (the
// 32-bit fields first, so every array is aligned).  The pixel's RNG state,
// colour sums, finished samples and live-bounce count; the remaining dead
// depths of its finished sample; the READY and fast-forward rings (of slots).
#define RTP_POOL_SLOT_FIELDS(F)                                                                       \
  F(uint32_t, seed) F(float, r) F(float, g) F(float, b) F(uint32_t, samples) F(uint32_t, live) \
  F(uint16_t, rem) F(uint16_t, q_ready) F(uint16_t, q_ff)
struct PoolSlots {
#define F(T, name) T* name;
  RTP_POOL_SLOT_FIELDS(F)
#undef F
  uint32_t* entry;  // kSteal: the slot's entry    } the wave's part of a table of the block,
  float* m2;        // kResume: its second moment  } null in the other instances
};
// LDS per wave: 30 B x 128 slots x 4 waves + the 2 KB quad shading table =
// 17 KiB per block.  Occupancy is set by VGPRs (5 waves per SIMD at <= 96, below).
// Measured on C2 / C3 / C4: 128 slots at 5 waves beat 256 slots at 4 waves
// by 6 / 10 / 5%; 256 slots at 5 waves (LDS booked to the last byte) and
// 128 slots at 6 waves (80 VGPRs, spills) were slower.
#define F(T, name) +(int)sizeof(T)
constexpr int kSlotBytes = 0 RTP_POOL_SLOT_FIELDS(F);
#undef F
static_assert(kSlotBytes == 30, "the measured pool: 30 B per slot");
constexpr int pool_lds_bytes(int waves) { return waves * kPool * kSlotBytes; }  // a block's pools
constexpr int entry_lds_bytes(int waves) { return waves * kPool * (int)sizeof(*PoolSlots().entry); }  // its entry table
// s_entry_all (kSteal) and s_m2_all (kResume): the block's tables
template <class Cfg>
RTP_DEV PoolSlots pool_slots(unsigned char* smem, int wib, uint32_t* s_entry_all, float* s_m2_all) {
  PoolSlots s;
  unsigned char* at = smem + (size_t)wib * kPool * kSlotBytes;
#define F(T, name) s.name = reinterpret_cast<T*>(at), at += kPool * sizeof(T);
  RTP_POOL_SLOT_FIELDS(F)
#undef F
  s.entry = Cfg::kSteal ? s_entry_all + wib * kPool : nullptr;
  s.m2 = Cfg::kResume ? s_m2_all + wib * kPool : nullptr;
  return s;
}
// PoolSlots::rem packs the remaining dead depths with how the sample's path ended
constexpr int kRemMask = 0x3fff, kEndLight = 0x4000, kEndNonfinite = 0x8000;
static_assert(kMaxDepth <= kRemMask, "the remaining dead depths fit rem's count field");

RTP_DEV uint32_t lane_rank(uint64_t mask) {  // number of set mask bits below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
RTP_DEV void wave_sync() {  // order LDS traffic between lanes of this wave (no cross-wave barrier)
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

RTP_DEV void set_priority(float lag) {  // (RTP_PRIO_BALANCE above) s_setprio needs an immediate
  if (lag > RTP_PRIO_THR) __builtin_amdgcn_s_setprio(3);
  else if (lag > 0.0f) __builtin_amdgcn_s_setprio(2);
  else if (lag > -RTP_PRIO_THR) __builtin_amdgcn_s_setprio(1);
  else __builtin_amdgcn_s_setprio(0);
}

// byte offset of the KParams argument in rtp_render_pool's kernarg segment:
// the first argument (the scene pointer) rounded up to KParams' alignment
// (also checked against the code object's argument metadata by
// tests/test_abi.py)
constexpr int kKParamsOffset =
    (int)((sizeof(const DevScene*) + alignof(KParams) - 1) / alignof(KParams) * alignof(KParams));
static_assert(alignof(KParams) <= 16 && kKParamsOffset == 8, "KParams follows the 8-byte scene pointer");
typedef const __attribute__((address_space(4))) KParams CKP;
// The kernel arguments re-read where they are used (scalar loads from the
// kernarg segment): values loaded once and kept live through the scheduling
// loop were SGPRs spilled to VGPR lanes (v_readlane in the hot path).
RTP_DEV CKP& kparams() {
  CKP* pp = (CKP*)((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() +
                   kKParamsOffset);
  asm volatile("" : "+s"(pp));
  return *pp;
}
typedef const __attribute__((address_space(1))) uint32_t GU32;
// kPlan: a planned launch (KParams::wave_begin): wave w owns the entries
// [wave_begin[w], wave_begin[w+1]) -- up to kPool of them, grouped by their
// expected cost -- instead of the interleaved entries j * n_waves + w.
// The pool kernel's body; kWPB waves per block, kLdsBvh: the sphere BVH is
// walked out of the block's LDS copy (s_bvh: the LDS walk's compact nodes,
// then its leaf spheres; rtp_render_pool_lds).
// kSteal: a launch with more entries than its waves' pools hold (C3, C4,
// C5 on one GPU).  The waves are the resident ones; a slot whose pixel has
// all its samples writes the pixel out and claims the next unclaimed entry
// (one atomic per batch), so no wave idles while entries remain, instead of
// waves of 128 pixels each running in generations with a tail per wave.
// kViews: a batched launch over several cameras (KParams::views, view_split
// above): the entries of different views share a wave under the interleaved
// deal and under stealing, so the camera is per lane -- each refill gathers
// its view's DevCamera from the global table (three 16-byte loads; the table
// of a hemisphere sweep is ~14 KB and stays in the vector L1 / L2).
// kResume: one more pass over a render state (rtp_render_resume_device).  An
// entry's seed, sums, live count and second moment are gathered from the
// state arrays (KParams::out, seed_out, live_out, m2) where the other
// instances compute or zero them, and written back by the unchanged write-out:
// each entry is owned by one slot, read once before its first sample of the
// pass and written once after its last.  PoolSlots::samples counts the pass's
// samples.  The second moment of the samples' luminance runs in a fifth float
// per slot (PoolSlots::m2), added where the sample is added to the sums.
// One instance's modes, by name (the seven of rtp_render_pool's template
// signature, in its order); LdsBvh: rtp_render_pool_lds's 16-wave block.
// Mesh: a mesh scene (rtp_set_scene_mesh): the quads behind the mesh BVH,
// walked resumably like the sphere BVH (rtp_trace.hpp mesh_visit).
template <bool Stats, bool Bvh, bool Tiles, bool Plan, bool Steal, bool Views, bool Resume, bool LdsBvh = false,
          bool Mesh = false>
struct PoolCfg {
  static constexpr bool kStats = Stats, kBvh = Bvh, kTiles = Tiles, kPlan = Plan, kSteal = Steal, kViews = Views,
                        kResume = Resume, kLdsBvh = LdsBvh, kMesh = Mesh;
  static constexpr int kWPB = LdsBvh ? kLdsBvhWavesPerBlock : kWavesPerBlock;  // waves per block
};

// A wave's place in the launch (wave-uniform): its global id, the launch's
// waves, (kPlan) its first entry, and the slots that hold an entry at the deal.
struct PoolWave {
  int w, n_waves, wbase, n_slots;
};
// slot j of wave w <-> list entry k = j * n_waves + w (pixels interleaved over waves)
// or, planned, k = wave_begin[w] + j.  Idx: the deal and the write-outs index
// with 64 bits, the refill with 32 (a 64-bit index spilled there).
template <class Cfg, class Idx>
RTP_DEV Idx dealt_entry(const PoolWave& wv, int slot) {
  return Cfg::kPlan ? (Idx)(wv.wbase + slot) : (Idx)slot * wv.n_waves + wv.w;
}
template <class Cfg, class Idx>
RTP_DEV Idx entry_of(const PoolSlots& s, const PoolWave& wv, int slot) {  // (kSteal: the entry the slot claimed last)
  if constexpr (Cfg::kSteal) return (Idx)s.entry[slot];
  else return dealt_entry<Cfg, Idx>(wv, slot);
}

// Slot j writes its entry k out, after the entry's last sample of the launch.
// (Its counterpart, a slot taking an entry, stays written out at the deal and
// at the steal claim: as one function it moved the code of 12 instances.)
template <class Cfg>
RTP_DEV void slot_write(const KParams& p, const PoolSlots& s, int j, int64_t k) {
  reinterpret_cast<float4*>(p.out)[k] = make_float4(s.r[j], s.g[j], s.b[j], 0.f);
  if (p.seed_out) p.seed_out[k] = s.seed[j];
  if (p.live_out) p.live_out[k] = s.live[j];
  if constexpr (Cfg::kResume)
    if (p.m2) p.m2[k] = s.m2[j];
}

// Back-to-front radiance of a sample that ended on the light at depth k_end
// (path_radiance), from the slot's history rows (row k_end holds E).
// Rows k_end and k_end-1 .. k_end-5 issued together (clamped to row 0; rows
// below 0 are not applied), the rest kHistChunk per trip, each chunk's loads
// issued together (one wait per chunk); products in the reference's order
// (depth k_end-1 down to 0).  One wait instead of up to three dependent round
// trips: C2 -1% (r03f, profiles/r03f_ab_history_prefetch.txt).
// (The masked multiply stays written out twice: as a helper of its own it
// moved the code of every pool instance.)
RTP_DEV f3 light_radiance(const float4* hist_base, int slot, int k_end, int64_t stride) {
  const float4* __restrict__ hp = hist_base + slot;
  f3 rw[kHistPrefetch];
#pragma unroll
  for (int i = 0; i < kHistPrefetch; i++) {
    const float4 v = hp[(int64_t)max(k_end - i, 0) * stride];
    rw[i] = mk(v.x, v.y, v.z);
  }
  float sx = rw[0].x + 0.0f, sy = rw[0].y + 0.0f, sz = rw[0].z + 0.0f;
#pragma unroll
  for (int i = 1; i < kHistPrefetch; i++) {
    const bool on = k_end - i >= 0;
    sx = on ? 0.0f + rw[i].x * sx : sx;
    sy = on ? 0.0f + rw[i].y * sy : sy;
    sz = on ? 0.0f + rw[i].z * sz : sz;
  }
  int dd = k_end - kHistPrefetch;
  for (; dd >= 0; dd -= kHistChunk) {
    f3 rc[kHistChunk];
#pragma unroll
    for (int i = 0; i < kHistChunk; i++) {
      const float4 v = hp[(int64_t)max(dd - i, 0) * stride];
      rc[i] = mk(v.x, v.y, v.z);
    }
#pragma unroll
    for (int i = 0; i < kHistChunk; i++) {
      const bool on = dd - i >= 0;
      sx = on ? 0.0f + rc[i].x * sx : sx;
      sy = on ? 0.0f + rc[i].y * sy : sy;
      sz = on ? 0.0f + rc[i].z * sz : sz;
    }
  }
  return mk(sx, sy, sz);
}

// The fast-forward's first jump-table read, issued before the radiance loads
// so that its latency overlaps theirs: the direct table of the sample's
// remaining count frc when there is one (then it is the only read), else the
// 32-depth table.
struct FfEarly {
  bool direct, chain;  // which table was read, if any
  uint32_t seed;
};
RTP_DEV FfEarly ff_early_read(bool mine, uint32_t fseed, int frc) {
  FfEarly e;
  e.seed = 0;
  CKP& FP = kparams();
  e.direct = mine && FP.ffd != nullptr && (unsigned)(frc - FP.ffd_first) < (unsigned)FP.ffd_count;
  e.chain = mine && !e.direct && FP.ff[0] != nullptr && frc >= 32;
  if (e.direct || e.chain) {
    GU32* src = (GU32*)(e.direct ? FP.ffd + ((uint64_t)(frc - FP.ffd_first) << 32) : FP.ff[0]);
    e.seed = src[fseed];
  }
  return e;
}

// The pool kernel's body: the deal, then the scheduling loop -- fast-forward
// batch if due, refill, walk, shade, end, publish -- then the write-out.
// The loop's stages stay inline and its state in plain locals.  As functions
// of their own (a slot taking an entry, the table jumps and hash loop, the
// primary ray, the walk, the priority block) or gathered into structs (the
// scheduler's and the lane's state, a stats object) they changed the
// instructions of the production instances, in every form tried; the helpers
// above are the ones that left them byte for byte.
// s_entry_all (kSteal) and s_m2_all (kResume): the block's tables, null in the other instances
template <class Cfg>
__device__ __forceinline__ void pool_body(const DevScene* __restrict__ sc, const KParams& p, int n_waves,
                                          unsigned char* smem, float* s_qshade, uint32_t* s_bvh,
                                          uint32_t* s_entry_all, float* s_m2_all) {
  constexpr bool kStats = Cfg::kStats, kBvh = Cfg::kBvh, kTiles = Cfg::kTiles, kPlan = Cfg::kPlan,
                 kLdsBvh = Cfg::kLdsBvh, kSteal = Cfg::kSteal, kViews = Cfg::kViews, kResume = Cfg::kResume,
                 kMesh = Cfg::kMesh;
  constexpr int kWPB = Cfg::kWPB;
  const int lane = threadIdx.x & 63;
  const int wib = threadIdx.x >> 6;
  const int w = blockIdx.x * kWPB + wib;  // global wave id
  // the quads' shading data into LDS (the block's only barrier, before any wave leaves)
  fill_qshade(sc, s_qshade);  // (n_quads <= kMaxQuads = kLdsQuads)
  if constexpr (kLdsBvh) {  // and the LDS walk's tree (its size checked on the host: rtp_lds_walk_capacity)
    const int nn = 8 * sc->n_lw_nodes, ns = sc->n_lw_sph;
    u4v* dst = reinterpret_cast<u4v*>(s_bvh);
    GU4* const gn = (GU4*)sc->lw_nodes;
    GU4* const gs = (GU4*)sc->lw_sph;
    for (int i = threadIdx.x; i < nn; i += blockDim.x) dst[i] = gn[i];
    for (int i = threadIdx.x; i < ns; i += blockDim.x) dst[nn + i] = gs[i];
  }
  __syncthreads();
  if (w >= n_waves) return;  // whole wave leaves; no block-level barriers follow
  const PoolSlots s = pool_slots<Cfg>(smem, wib, s_entry_all, s_m2_all);

  const uint32_t t1 = sc->which_t1, t2 = sc->which_t2;
  const int D = p.depth, S = p.spp;
  int n_slots, wbase = 0;
  if constexpr (kPlan) {  // (the host checked the plan; the clamps keep a bad one inside the buffers)
    wbase = p.wave_begin[w];
    n_slots = max(0, min(min(kPool, p.wave_begin[w + 1] - wbase), (int)(p.npix - wbase)));
  } else {
    const int64_t left = p.npix - w;
    n_slots = left <= 0 ? 0 : (int)min<int64_t>(kPool, (left + n_waves - 1) / n_waves);
  }
  const PoolWave wv{w, n_waves, wbase, n_slots};
  for (int j = lane; j < n_slots; j += 64) {  // the deal: slot j takes its entry
    const int64_t k = dealt_entry<Cfg, int64_t>(wv, j);
    if constexpr (kSteal) s.entry[j] = (uint32_t)k;
    if constexpr (kResume) {  // the entry's state so far
      const float4 v = reinterpret_cast<const float4*>(p.out)[k];
      s.seed[j] = p.seed_out[k];
      s.r[j] = v.x;
      s.g[j] = v.y;
      s.b[j] = v.z;
      s.samples[j] = 0u;
      s.live[j] = p.live_out ? p.live_out[k] : 0u;
      s.m2[j] = p.m2 ? p.m2[k] : 0.f;
    } else {
      if constexpr (kViews) s.seed[j] = view_seed(p, (int)k);
      else s.seed[j] = p.seed_base + (uint32_t)pixel_of<kTiles>(p, k);  // seeds[i] = i (MapperPathTracer.cxx:265-267)
      s.r[j] = 0.f;
      s.g[j] = 0.f;
      s.b[j] = 0.f;
      s.samples[j] = 0u;
      s.live[j] = 0u;
    }
    s.rem[j] = 0;
    s.q_ready[j] = (uint16_t)j;
  }
  wave_sync();
  // wave-uniform, monotone queue cursors
  // (uint32: under kSteal a wave's finished-sample count ff_tail runs over
  // every pixel it claims -- C5 on one GPU: ~2.6e10 -- so it wraps; only the
  // differences of cursors (each < 2^31: <= kPool * spp) and their low bits
  // (the ring index) are used, and unsigned arithmetic wraps exactly)
  uint32_t ready_head = 0, ready_tail = (S > 0) ? n_slots : 0, ff_head = 0, ff_tail = 0;
  int unfinished = n_slots;                // stats only: pixels with samples still to run
  unsigned long long t_tail = 0;

  // attenuation history per pixel SLOT, D rows: a pixel has one sample in
  // flight, so its history survives until the fast-forward batch that
  // computes the sample's radiance (row k of a light hit holds E_k)
  // depth-major [d][wave*kPool + slot]: the hot depths 0..4 of all slots
  // stay dense.  (A slot-major layout, one pixel's rows in one 128-byte line,
  // measured no faster: r03c, profiles/r03c_ab_history_prex.txt.)
  float4* __restrict__ const hist_base = reinterpret_cast<float4*>(p.hist) + (int64_t)w * kPool;
  const int64_t stride = (int64_t)n_waves * kPool;
  float4* __restrict__ hist = hist_base;  // per lane: hist_base + slot of its path
  const f3 eye = ld3(p.cam.eye);

  // diagnostics (uniform branch on a kernel argument; off in production)
  // (compiled in only for the kStats instantiation: the counters cost ~30 VGPRs)
  unsigned long long dbg[kStats ? kDbgCounters : 1] = {};
  constexpr bool want_dbg = kStats;
  unsigned long long* const gdbg = want_dbg ? p.dbg + (int64_t)w * kDbgCounters : nullptr;
  const unsigned long long t_start = want_dbg ? __builtin_amdgcn_s_memtime() : 0ull;
  if (p.dbg && lane == 0) {  // placement + start time (RTP_DEBUG_STATS=1|2)
    p.dbg[(int64_t)w * kDbgCounters + kDbgRealStart] = __builtin_amdgcn_s_memrealtime();
    p.dbg[(int64_t)w * kDbgCounters + kDbgHwId] =
        (unsigned)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));  // HW_REG_HW_ID
  }

  uint32_t published = 0;  // wave-uniform: ff_tail when the finished samples were last added to p.progress
  // kSteal (wave-uniform): slots still holding a pixel, and the samples of the
  // pixels already written out (the fair-share average is over the others)
  int live_slots = n_slots;
  uint32_t retired = 0;  // (the samples of the written-out pixels, mod 2^32 like ff_tail)
  bool critical_ff = false;  // wave-uniform: a critical (far-lagging) pixel waits in the FF queue

  bool has_path = false;
  int slot = 0;
  uint32_t seed = 0;
  // Sphere-BVH scenes (global walk): the closest-hit search is resumable.
  // A path's walk spans as many loop iterations as it needs; an iteration
  // walks until RTP_WALK_DONE of the wave's paths have finished theirs, and
  // only those are shaded.  The walks' lengths differ several-fold between
  // lanes (C3: 17 of 64 lanes per VALU instruction when every lane's walk ran
  // to its end inside one iteration); now a long walk no longer holds the
  // other 63 lanes.  The walk is the same walk (same nodes, same order, same
  // running minimum), so the hit is bit-identical.
  int wni = -1;                             // the path's next BVH node; -1: its quads are not scanned yet
  Hit wh{3.40282347e+38f, -1, 0};           // its closest hit so far
  Path ps;
  ps.org = eye;
  ps.dir = mk(0.f, 0.f, 1.f);
  ps.d = 0;
  ps.nonfinite = false;

  for (;;) {
    const uint64_t idle = __ballot(!has_path);
    const int n_idle = __popcll(idle);
    const int n_ready = (int)(ready_tail - ready_head);
    const int n_ff = (int)(ff_tail - ff_head);
    if ((n_ready < n_idle + RTP_FF_MARGIN || critical_ff) && n_ff > 0) {
      critical_ff = false;
      // ---- batch RNG fast-forward over the remaining dead depths of finished
      //      samples (1 + {2,3,2} draws per depth) ----
      const unsigned long long t0 = want_dbg ? __builtin_amdgcn_s_memtime() : 0ull;
      const int n = min(64, n_ff);
      const bool mine = lane < n;
      int fslot = 0, frem = 0;
      uint32_t fseed = 0;
      if (mine) {
        fslot = s.q_ff[(ff_head + lane) & (kPool - 1)];
        fseed = s.seed[fslot];
        frem = s.rem[fslot];
      }
      const FfEarly early = ff_early_read(mine, fseed, frem & kRemMask);
      if (mine) {
        // back-to-front radiance of the pixel's finished sample (path_radiance),
        // banked in sample order before the pixel's next sample can start
        const int flags = frem;
        frem &= kRemMask;
        f3 c;
        if (flags & kEndLight) {
          const int k_end = D - frem;  // a light hit ends the path: rem = D - 1 - k_end + 1
          if (want_dbg) {
            dbg_region(gdbg, kDbgFfRadVisits);
            dbg_add(gdbg, kDbgFfRadRows, (unsigned long long)(k_end + 1));
          }
          c = light_radiance(hist_base, fslot, k_end, stride);
        } else {
          const float v = (flags & kEndNonfinite) ? __builtin_nanf("") : 0.0f;
          c = mk(v, v, v);
        }
        s.r[fslot] = s.r[fslot] + c.x;  // cols += sumtotl (MapperPathTracer.cxx:350), in sample order
        s.g[fslot] = s.g[fslot] + c.y;
        s.b[fslot] = s.b[fslot] + c.z;
        if constexpr (kResume) {  // m2 += y * y, y the sample's luminance (include/rtp.h rtp_render_state)
          const float y = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
          s.m2[fslot] = s.m2[fslot] + y * y;
        }
      }
      // jump over 32 / 16 / 8 / 4 dead depths with one table read each
      // (HBM-resident tables of the dead-step map, built once per device),
      // then hash the few remaining depths
      if (early.direct) {
        fseed = early.seed;
        frem = 0;
      } else if (early.chain) {
        fseed = early.seed;
        frem -= 32;
      }
#pragma unroll
      for (int j = 1; j < kFfTables; j++) {
        GU32* __restrict__ tab = (GU32*)kparams().ff[j];
        if (tab != nullptr && mine && frem >= (32 >> j)) {
          fseed = tab[fseed];
          frem -= 32 >> j;
        }
      }
      int iters = 0;
      for (int i = 0;; i++) {
        const bool act = mine && i < frem;
        if (!__any(act)) break;
        if (act) fseed = dead_step(fseed, t1, t2);
        if (want_dbg) {
          const uint64_t am = __ballot(act);
          if (lane == 0) dbg_add(gdbg, kDbgDeadLanes, (unsigned long long)__popcll(am));
        }
        iters++;
      }
      bool again = false;
      if (mine) s.seed[fslot] = fseed;
      if (mine) again = s.samples[fslot] < (uint32_t)S;
      if (want_dbg) unfinished -= __popcll(__ballot(mine && !again));
      if constexpr (kSteal) {
        // pixels with all their samples: written out, their slots take the
        // next unclaimed entries (claimed in launch order after the initial
        // n_waves * kPool)
        const uint64_t done = __ballot(mine && !again);
        if (done) {
          const int nd = __popcll(done);
          unsigned long long base = 0;
          if (lane == 0) base = atomicAdd(kparams().progress + 1, (unsigned long long)nd);
          base = __shfl(base, 0) + (unsigned long long)n_waves * kPool;
          retired += (uint32_t)(nd * S);
          if (mine && !again) {
            slot_write<Cfg>(p, s, fslot, entry_of<Cfg, int64_t>(s, wv, fslot));
            const unsigned long long kn = base + lane_rank(done);
            if (kn < (unsigned long long)p.npix) {  // a fresh pixel in this slot, at the front of READY below
              s.entry[fslot] = (uint32_t)kn;
              if constexpr (kResume) {  // the claimed entry's state so far
                const float4 v = reinterpret_cast<const float4*>(p.out)[kn];
                s.seed[fslot] = p.seed_out[kn];
                s.r[fslot] = v.x;
                s.g[fslot] = v.y;
                s.b[fslot] = v.z;
                s.samples[fslot] = 0u;
                s.live[fslot] = p.live_out ? p.live_out[kn] : 0u;
                s.m2[fslot] = p.m2 ? p.m2[kn] : 0.f;
              } else {
                if constexpr (kViews) s.seed[fslot] = view_seed(p, (int)kn);
                else s.seed[fslot] = p.seed_base + (uint32_t)pixel_of<kTiles>(p, (int)kn);
                s.r[fslot] = 0.f;
                s.g[fslot] = 0.f;
                s.b[fslot] = 0.f;
                s.samples[fslot] = 0u;
                s.live[fslot] = 0u;
              }
              s.rem[fslot] = 0;
              again = true;
            }
          }
          live_slots -= __popcll(__ballot(mine && !again));
        }
      }
      // Fair share: a pixel whose completed samples are at or below the
      // wave's average (ff_tail / n_slots) goes to the FRONT of the READY
      // ring, the others to the back.  FIFO alone let cheap pixels (short
      // paths, back sooner) take more than their share of lanes, so the
      // expensive pixels' sequential sample chains ran on alone at the end
      // (17% of bounce steps with ~12 of 64 lanes live).
      // (samples * slots <= 2^23 * 2^7; ff_tail (no stealing) and ff_tail - retired (the
      // held pixels' finished samples) are <= 2^7 * spp: 32 bits suffice)
      const bool urgent = again && (kSteal ? s.samples[fslot] * (uint32_t)live_slots <= (uint32_t)(ff_tail - retired)
                                           : s.samples[fslot] * (uint32_t)n_slots <= (uint32_t)ff_tail);
      const uint64_t pu = __ballot(urgent), pn = __ballot(again && !urgent);
      ready_head -= (uint32_t)__popcll(pu);
      if (urgent) s.q_ready[(ready_head + lane_rank(pu)) & (kPool - 1)] = (uint16_t)fslot;
      if (again && !urgent) s.q_ready[(ready_tail + lane_rank(pn)) & (kPool - 1)] = (uint16_t)fslot;
      ready_tail += __popcll(pn);
      ff_head += n;
      wave_sync();
      if (want_dbg) {
        dbg[kDbgFfPhases] += 1;
        dbg[kDbgFfLanes] += (unsigned long long)n;
        dbg[kDbgFfIters] += (unsigned long long)iters;
        dbg[kDbgCyclesFf] += __builtin_amdgcn_s_memtime() - t0;
      }
      // on into the refill, which takes the pixels this batch made READY,
      // and the bounce: a sample's chain spends no iteration of its own on
      // the fast-forward
    }
    // ---- refill idle lanes with the next sample of READY pixels ----
    const unsigned long long tb = stamp(want_dbg);
    const int take = min(n_idle, (int)(ready_tail - ready_head));
    if (!has_path) {
      const int r = (int)lane_rank(idle);
      if (r < take) {
        if (want_dbg) dbg_region(gdbg, kDbgRefillVisits);
        slot = s.q_ready[(ready_head + r) & (kPool - 1)];
        seed = s.seed[slot];
        hist = hist_base + slot;
        // the camera and tile constants re-read from the kernel arguments
        // here (kparams): kept live through the loop they were SGPRs spilled
        // to VGPR lanes, ~30 v_readlane per refill (through the kernarg
        // segment pointer: &p would copy p to scratch)
        CKP& P = kparams();
        int pi, pj;
        if constexpr (kViews) {  // the entry's view: its camera gathered per lane
          int v, u;
          view_split(P, entry_of<Cfg, int>(s, wv, slot), v, u);
          view_pixel_xy(P, u, pi, pj);
          const DevCamera vc = P.views[v].cam;
          ps.dir = camera_ray(vc, pi, pj, P.nx, P.ny, seed);
          ps.org = ld3(vc.eye);
        } else {
          pixel_xy<kTiles>(P, entry_of<Cfg, int>(s, wv, slot), pi, pj);
          ps.dir = camera_ray(P.cam, pi, pj, P.nx, P.ny, seed);
          ps.org = ld3(P.cam.eye);
        }
        ps.d = 0;
        ps.nonfinite = false;
        has_path = true;
      }
    }
    ready_head += take;
    if (!__any(has_path) && ff_tail == ff_head) break;  // nothing live, nothing READY, nothing to fast-forward
    if (want_dbg) dbg[kDbgCyclesRefill] += __builtin_amdgcn_s_memtime() - tb;
    // ---- one depth of every live path: walk (sphere-BVH scenes), shade, end ----
    bool ended = false;
    const unsigned long long ta = stamp(want_dbg);
    unsigned long long tbnc = ta;
    bool shade = has_path;
    if constexpr (kMesh) {
      // The resumable search of a mesh scene, with the sphere walk's rule
      // (RTP_WALK_DONE): a new ray scans the inline spheres, then walks the
      // mesh BVH from node 0 -- or, under RTP_MESH_SCAN=1 (wave-uniform),
      // tests every quad in storage order, wni counting quads instead of nodes.
      const bool scan = sc->mesh_scan != 0;
      const int nn = scan ? sc->n_mesh_quads : sc->n_mesh_nodes;
      if (has_path && wni < 0) {
        wh = mesh_spheres(sc, ps.org, ps.dir);
        wni = 0;
      }
      const uint64_t pm = __ballot(has_path);
      const int need = min(RTP_WALK_DONE, __popcll(pm));
      bool walking = has_path && wni < nn;
      if (__ballot(walking)) {
        const f3 o = ps.org, d = ps.dir;
        const MeshRay R = mesh_ray(sc, o, d);
        GF4* __restrict__ quads = (GF4*)sc->mesh_quads;
        u4v v = u4v{0u, 0u, 0u, 0u};
        if (walking && !scan) v = R.nodes[wni];
        for (;;) {
          const uint64_t wm = __ballot(walking);
          if (wm == 0 || __popcll(pm & ~wm) >= need) break;
          if (walking) {
            int next;
            if (scan) {
              mesh_quad_test(quads, wni, o, d, wh);
              next = wni + 1;
            } else {
              next = mesh_visit(quads, R, o, d, v, wni, wh);
            }
            walking = next < nn;
            if (walking && !scan) v = R.nodes[next];
            wni = next;
          }
        }
      }
      shade = has_path && !walking;
    } else if constexpr (kBvh) {
      // the resumable sphere-BVH walk; the lanes whose walk is done shade
      const int nn = kLdsBvh ? sc->n_lw_nodes : sc->n_nodes;
      if (has_path && wni < 0) {  // a new ray: the quads first (their hit bounds the walk)
        wh = closest_hit<false, false>(sc, ps.org, ps.dir, true, nullptr, s_qshade + kPrexLdsOffset);
        wni = 0;
      }
      const uint64_t pm = __ballot(has_path);
      const int need = min(RTP_WALK_DONE, __popcll(pm));
      bool walking = has_path && wni < nn;
      if (__ballot(walking)) {
        const f3 o = ps.org, d = ps.dir;
        const BvhRay R = bvh_ray<kLdsBvh>(sc, o, d);
        GF4* __restrict__ geom_g = (GF4*)sc->sph_geom;
        // the LDS walk: this octant's copy of the nodes, then the leaf spheres
        LU4* const lnodes = (LU4*)s_bvh + (kLdsBvh ? ray_octant(d) * nn : 0);
        LF4* const lsph = (LF4*)s_bvh + (kLdsBvh ? 8 * nn : 0);
        auto node = [&](int i) {
          if constexpr (kLdsBvh) return lnodes[i];
          else if constexpr (RTP_BVH_NT) return __builtin_nontemporal_load(R.nodes + i);
          else return R.nodes[i];
        };
        u4v v = u4v{0u, 0u, 0u, 0u};
        if (walking) v = node(wni);
        for (;;) {
          const uint64_t wm = __ballot(walking);
          if (wm == 0 || __popcll(pm & ~wm) >= need) break;
          if (walking) {
            const int next = bvh_visit<kLdsBvh>(geom_g, lsph, R, o, d, v, wni, wh);
            walking = next < nn;
            if (walking) v = node(next);
            wni = next;
          }
        }
        if (has_path && !walking) bvh_resolve(wh, R);
      }
      shade = has_path && !walking;
      if (want_dbg) dbg[kDbgCyclesIntersect] += stamp(want_dbg) - ta;
    }
    if (shade) {
      f3 emit = mk(0.f, 0.f, 0.f);
      int res;
      if constexpr (kMesh) {
        res = shade_hit<false, true, true>(sc, ps, seed, emit, hist + (int64_t)ps.d * stride, D, s_qshade, wh, gdbg);
        wni = -1;
      } else if constexpr (kBvh) {
        res = shade_hit<kBvh, true>(sc, ps, seed, emit, hist + (int64_t)ps.d * stride, D, s_qshade, wh,
                                    gdbg);  // (stats build: the region counters; nullptr otherwise)
        wni = -1;
      } else {
        res = bounce<kBvh, true>(sc, ps, seed, emit, hist + (int64_t)ps.d * stride, D, want_dbg ? dbg : nullptr,
                                 s_qshade, gdbg);
      }
      tbnc = stamp(want_dbg);
      if (res == kAlive && ps.d < D - 1) {
        ps.d++;
      } else {
        const int k_end = ps.d;
        if (want_dbg) dbg_region(gdbg, kDbgEndVisits);
        // the radiance product runs in the fast-forward batch (above)
        if (res == kLight) hist[(int64_t)k_end * stride] = make_float4(emit.x, emit.y, emit.z, 0.f);
        // dead depths left: D-1-k_end, plus depth k_end's own draws when the
        // path died there (bounce<.., true> left them to the fast-forward)
        const int rem = D - 1 - k_end + (res != kAlive ? 1 : 0);
        s.rem[slot] = (uint16_t)(rem | (res == kLight ? kEndLight : 0) | (ps.nonfinite ? kEndNonfinite : 0));
        s.samples[slot] = s.samples[slot] + 1u;
        s.live[slot] = s.live[slot] + (uint32_t)(k_end + 1);
        s.seed[slot] = seed;
        ended = true;
        has_path = false;
      }
    }
    if (want_dbg) {
      const unsigned long long te = __builtin_amdgcn_s_memtime();
      dbg[kDbgCyclesShade] += tbnc - ta;  // minus the intersect share, subtracted on the host
      dbg[kDbgCyclesEnd] += te - tbnc;
    }
    // ---- the ended samples queue for the fast-forward; publish ----
    const uint64_t fin = __ballot(ended);
    if (ended) s.q_ff[(ff_tail + lane_rank(fin)) & (kPool - 1)] = (uint16_t)slot;
#if RTP_CRIT_FF > 0
    // A pixel whose finished samples lag the wave's average by more than
    // RTP_CRIT_FF/1000 runs its sample chain on the critical path (its path
    // length keeps it behind): its fast-forward is not left waiting for the
    // READY queue to run dry -- the batch runs in the next iteration.
    // (a scheduling heuristic: single precision is plenty; kSteal: fresh
    // pixels always lag, so no critical batches)
    if (!kSteal && __ballot(ended && (float)(s.samples[slot] * (uint32_t)n_slots) * 1000.0f <
                              (float)ff_tail * (float)(1000 - RTP_CRIT_FF)))
      critical_ff = true;
#endif
    ff_tail += __popcll(fin);
    wave_sync();
    if (RTP_PRIO_BALANCE && ff_tail - published >= (uint32_t)kPrioPeriod) {
      unsigned long long g = 0;
      if (lane == 0) g = atomicAdd(kparams().progress, (unsigned long long)(ff_tail - published));
      g = __shfl(g, 0) + (unsigned long long)(ff_tail - published);
      published = ff_tail;
      float lag;
      if constexpr (kSteal) {
        // remaining samples: this wave's (its held pixels') against the
        // average wave's, npix * S - g over the waves.  While unclaimed
        // entries remain, the average includes them and every wave sits
        // below it (priority 0: the stealing balances); once they are gone
        // the waves with the most work left get the issue slots.  In units
        // of a full pool's samples, like the fractions below.
        const float mine_left = (float)live_slots * (float)S - (float)(ff_tail - retired);
        const float avg_left = ((float)kparams().npix * (float)S - (float)g) / (float)n_waves;
        lag = (mine_left - avg_left) / ((float)kPool * (float)S);
      } else {
        // completed fractions: global g / (npix*S) vs own ff_tail / (n_slots*S)
        lag = ((float)g / (float)kparams().npix - (float)ff_tail / (float)n_slots) / (float)S;
      }
      set_priority(lag);
    }
    if (want_dbg && unfinished < 64) {
      if (t_tail == 0) t_tail = __builtin_amdgcn_s_memtime();
      dbg[kDbgTailSteps] += 1;
      dbg[kDbgTailLanes] += (unsigned long long)__popcll(__ballot(has_path || ended));
    }
    if (want_dbg) {
      dbg[kDbgBounceSteps] += 1;
      dbg[kDbgBounceLanes] += (unsigned long long)__popcll(__ballot(has_path || ended));
      dbg[kDbgCyclesBounce] += __builtin_amdgcn_s_memtime() - tb;
    }
  }
  if (!kStats && p.dbg && lane == 0)  // RTP_DEBUG_STATS=2: lifetime only
    p.dbg[(int64_t)w * kDbgCounters + kDbgRealEnd] = __builtin_amdgcn_s_memrealtime();
  if (want_dbg && lane == 0) {
    dbg[kDbgCyclesTotal] = __builtin_amdgcn_s_memtime() - t_start;
    dbg[kDbgRealEnd] = __builtin_amdgcn_s_memrealtime();
    dbg[kDbgTailCycles] = t_tail ? __builtin_amdgcn_s_memtime() - t_tail : 0;
    for (int c = 0; c < (kStats ? kDbgRefillVisits : 0); c++)  // (the later counters are accumulated in place)
      if (c != kDbgRealStart && c != kDbgHwId) p.dbg[(int64_t)w * kDbgCounters + c] = dbg[c];
  }
  wave_sync();
  for (int j = lane; j < (kSteal ? 0 : n_slots); j += 64)  // (kSteal: written as they finished)
    slot_write<Cfg>(p, s, j, entry_of<Cfg, int64_t>(s, wv, j));
}

#if RTP_POOL_MAX_VGPR > 0
#define RTP_POOL_VGPR_ATTR __attribute__((amdgpu_num_vgpr(RTP_POOL_MAX_VGPR)))
#else
#define RTP_POOL_VGPR_ATTR
#endif
template <bool kStats, bool kBvh, bool kTiles = false, bool kPlan = false, bool kSteal = false, bool kViews = false,
          bool kResume = false, bool kMesh = false>
__global__ void __launch_bounds__(256, RTP_POOL_MIN_WAVES_PER_EU) RTP_POOL_VGPR_ATTR
    rtp_render_pool(const DevScene* __restrict__ sc, KParams p, int n_waves) {
  static_assert(!kViews || (!kStats && !kBvh && !kTiles && !kPlan), "batched views: the plain and stealing instances");
  static_assert(!kMesh || (!kStats && !kBvh && !kTiles && !kPlan && !kViews),
                "mesh scenes: {plain, stealing} x {render, resume}");
  static_assert(!kResume || (!kStats && !kTiles && !kPlan && !kViews),
                "resume: {no BVH, global sphere walk} x {plain, stealing}; no stats, wave plan, tile deal or views");
  __shared__ __align__(16) unsigned char smem[pool_lds_bytes(kWavesPerBlock)];
  __shared__ __align__(16) float s_qshade[kQTableFloats];
  float* s_m2 = nullptr;
  uint32_t* s_entry = nullptr;
  if constexpr (kResume) {  // (+2 KiB a block: 5 blocks per CU still fit)
    __shared__ float m2[kWavesPerBlock * kPool];
    s_m2 = m2;
  }
  if constexpr (kSteal) {
    __shared__ uint32_t entry[kWavesPerBlock * kPool];
    s_entry = entry;
  }
  pool_body<PoolCfg<kStats, kBvh, kTiles, kPlan, kSteal, kViews, kResume, /*LdsBvh*/ false, kMesh>>(
      sc, p, n_waves, smem, s_qshade, nullptr, s_entry, s_m2);
}

// Scenes whose LDS walk tree fits (DevScene::lw_nodes, rtp_lds_walk_capacity):
// one 16-wave block per CU (4 waves per SIMD, <= 128 VGPRs) shares one LDS
// copy of the tree -- dynamic LDS after the waves' pools, the quad tables and
// (kSteal) the slots' entries.
template <bool kTiles, bool kSteal>
__global__ void __launch_bounds__(64 * kLdsBvhWavesPerBlock, 1) __attribute__((amdgpu_num_vgpr(128)))
    rtp_render_pool_lds(const DevScene* __restrict__ sc, KParams p, int n_waves) {
  __shared__ __align__(16) unsigned char smem[pool_lds_bytes(kLdsBvhWavesPerBlock)];
  __shared__ __align__(16) float s_qshade[kQTableFloats];
  extern __shared__ __align__(16) uint32_t s_dyn[];
  uint32_t* s_entry = nullptr;
  if constexpr (kSteal) {
    __shared__ uint32_t entry[kLdsBvhWavesPerBlock * kPool];
    s_entry = entry;
  }
  using Cfg = PoolCfg</*Stats*/ false, /*Bvh*/ true, kTiles, /*Plan*/ false, kSteal, /*Views*/ false,
                      /*Resume*/ false, /*LdsBvh*/ true>;
  pool_body<Cfg>(sc, p, n_waves, smem, s_qshade, s_dyn, s_entry, nullptr);
}
constexpr int kLdsWalkStaticBytes = pool_lds_bytes(kLdsBvhWavesPerBlock) + kQTableFloats * (int)sizeof(float) +
                                    entry_lds_bytes(kLdsBvhWavesPerBlock);
constexpr int kLdsWalkDynBytes = 160 * 1024 - kLdsWalkStaticBytes;  // the tree's share of the CU's 160 KiB
static_assert(kPool != 128 || kLdsWalkDynBytes >= 64 * 1024, "the LDS walk keeps room for a C3-size tree");

}  // namespace rtp
