// rtp_diag.hpp -- the diagnostic and utility kernels over the per-ray code:
// single primitives, closest_hit and bounce on host rays, the first-hit
// guides, the RNG jump tables, the exhaustive fast-math check.
#pragma once
#include "rtp_trace.hpp"

namespace rtp {

__global__ void rtp_eval_primitive_kernel(int kind, const void* in, void* out, int64_t n, const uint32_t* tab,
                                          uint32_t t1, uint32_t t2) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* fi = static_cast<const float*>(in);
  const uint32_t* ui = static_cast<const uint32_t*>(in);
  float* fo = static_cast<float*>(out);
  uint32_t* uo = static_cast<uint32_t*>(out);
  switch (kind) {
    case 0: fo[i] = rtp_sinf(fi[i]); break;
    case 1: fo[i] = rtp_cosf(fi[i]); break;
    case 2: fo[i] = 1.0f / __builtin_sqrtf(fi[i]); break;
    case 3: uo[i] = wang(ui[i]); break;
    case 4: uo[i] = tab[ui[i]]; break;          // jump-table gather (ff16 / ff32)
    case 5: uo[i] = dead_step(ui[i], t1, t2); break;
    default: break;
  }
}

// closest_hit with and without the prefilter on a list of rays (o, d: 6
// floats each): out[7 i ..] = prefiltered (t bits, kind, idx), exact scan
// (t bits, kind, idx), 1 if the lane fell back to the exact scan.
template <bool kBvh>
__global__ void __launch_bounds__(256) rtp_eval_closest_kernel(const DevScene* __restrict__ sc,
                                                               const float* __restrict__ rays, uint32_t* out,
                                                               int64_t n) {
  __shared__ __align__(16) float s_qshade[kQTableFloats];
  fill_qshade(sc, s_qshade);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = rays + 6 * i;
  const f3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
  uint32_t full = 0;
  const Hit a = closest_hit<kBvh>(sc, o, d, true, &full, s_qshade + kPrexLdsOffset);
  const Hit b = closest_hit<kBvh>(sc, o, d, false, nullptr, nullptr);
  uint32_t* w = out + 7 * i;
  w[0] = __float_as_uint(a.t), w[1] = (uint32_t)a.kind, w[2] = (uint32_t)a.idx;
  w[3] = __float_as_uint(b.t), w[4] = (uint32_t)b.kind, w[5] = (uint32_t)b.idx;
  w[6] = full;
}

// One bounce() per host ray (o, d: 6 floats; its seed), one lane per ray:
// depth 0 of a two-deep path, so that A[0] is stored.  out[15 i ..] = the
// result code, emit, A[0], ps.org, ps.dir, the seed after the depth's draws,
// ps.nonfinite.  emit starts as 0 and A[0] as 1: what the reference's
// arrays hold after a depth that ends the path (SurfaceWorklets.h:104-109,
// ScatterWorklet.h:80, 114).
template <bool kBvh>
__global__ void __launch_bounds__(256) rtp_eval_bounce_kernel(const DevScene* __restrict__ sc,
                                                              const float* __restrict__ rays,
                                                              const uint32_t* __restrict__ seeds, uint32_t* out,
                                                              int64_t n) {
  __shared__ __align__(16) float s_qshade[kQTableFloats];
  fill_qshade(sc, s_qshade);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = rays + 6 * i;
  Path ps;
  ps.org = mk(r[0], r[1], r[2]);
  ps.dir = mk(r[3], r[4], r[5]);
  ps.d = 0;
  ps.nonfinite = false;
  uint32_t seed = seeds[i];
  f3 emit = mk(0.f, 0.f, 0.f);
  float4 a0 = make_float4(1.f, 1.f, 1.f, 0.f);
  const int res = bounce<kBvh, false>(sc, ps, seed, emit, &a0, 2, nullptr, s_qshade);
  uint32_t* w = out + 15 * i;
  w[0] = (uint32_t)res;
  w[1] = __float_as_uint(emit.x), w[2] = __float_as_uint(emit.y), w[3] = __float_as_uint(emit.z);
  w[4] = __float_as_uint(a0.x), w[5] = __float_as_uint(a0.y), w[6] = __float_as_uint(a0.z);
  w[7] = __float_as_uint(ps.org.x), w[8] = __float_as_uint(ps.org.y), w[9] = __float_as_uint(ps.org.z);
  w[10] = __float_as_uint(ps.dir.x), w[11] = __float_as_uint(ps.dir.y), w[12] = __float_as_uint(ps.dir.z);
  w[13] = seed;
  w[14] = ps.nonfinite ? 1u : 0u;
}

// The same two on a mesh scene (rtp_set_scene_mesh).  Closest hit: the walk
// of the mesh BVH (t bits, kind, the caller's quad index or the sphere index),
// then the brute-force scan of every mesh quad with the same per-lane test,
// then 3.
__global__ void __launch_bounds__(256) rtp_eval_closest_mesh_kernel(const DevScene* __restrict__ sc,
                                                                    const float* __restrict__ rays, uint32_t* out,
                                                                    int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = rays + 6 * i;
  const f3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
  const Hit a = closest_hit_mesh<false>(sc, o, d);
  const Hit b = closest_hit_mesh<true>(sc, o, d);
  uint32_t* w = out + 7 * i;
  w[0] = __float_as_uint(a.t), w[1] = (uint32_t)a.kind, w[2] = (uint32_t)a.idx;
  w[3] = __float_as_uint(b.t), w[4] = (uint32_t)b.kind, w[5] = (uint32_t)b.idx;
  w[6] = 3u;
}
// One depth on a mesh scene: the closest hit by the walk (the scan under
// RTP_MESH_SCAN=1, as the renders), then shade_hit's mesh variant.
__global__ void __launch_bounds__(256) rtp_eval_bounce_mesh_kernel(const DevScene* __restrict__ sc,
                                                                   const float* __restrict__ rays,
                                                                   const uint32_t* __restrict__ seeds, uint32_t* out,
                                                                   int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = rays + 6 * i;
  Path ps;
  ps.org = mk(r[0], r[1], r[2]);
  ps.dir = mk(r[3], r[4], r[5]);
  ps.d = 0;
  ps.nonfinite = false;
  uint32_t seed = seeds[i];
  f3 emit = mk(0.f, 0.f, 0.f);
  float4 a0 = make_float4(1.f, 1.f, 1.f, 0.f);
  const Hit h = sc->mesh_scan ? closest_hit_mesh<true>(sc, ps.org, ps.dir) : closest_hit_mesh<false>(sc, ps.org, ps.dir);
  const int res = shade_hit<false, false, true>(sc, ps, seed, emit, &a0, 2, nullptr, h);
  uint32_t* w = out + 15 * i;
  w[0] = (uint32_t)res;
  w[1] = __float_as_uint(emit.x), w[2] = __float_as_uint(emit.y), w[3] = __float_as_uint(emit.z);
  w[4] = __float_as_uint(a0.x), w[5] = __float_as_uint(a0.y), w[6] = __float_as_uint(a0.z);
  w[7] = __float_as_uint(ps.org.x), w[8] = __float_as_uint(ps.org.y), w[9] = __float_as_uint(ps.org.z);
  w[10] = __float_as_uint(ps.dir.x), w[11] = __float_as_uint(ps.dir.y), w[12] = __float_as_uint(ps.dir.z);
  w[13] = seed;
  w[14] = ps.nonfinite ? 1u : 0u;
}

// First-hit guides of a path camera (rtp_render_guides_device), one lane per
// pixel: the ray through the pixel centre (camera_ray_at with 0.5f for both
// jitter draws), the path kernel's closest_hit, and of that hit the normal
// shade_hit takes (flipped to face the ray origin), t, the texture colour
// and the primitive.  No RNG, no render state.
template <bool kBvh>
__global__ void __launch_bounds__(256) rtp_guides_kernel(const DevScene* __restrict__ sc, GuideParams p) {
  __shared__ __align__(16) float s_qshade[kQTableFloats];
  fill_qshade(sc, s_qshade);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.npix) return;
  const int pi = (int32_t)i % p.nx, pj = (int32_t)i / p.nx;
  const f3 o = ld3(p.cam.eye);
  const f3 d = camera_ray_at(p.cam, pi, pj, p.nx, p.ny, 0.5f, 0.5f);
  const Hit h = closest_hit<kBvh>(sc, o, d, true, nullptr, s_qshade + kPrexLdsOffset);
  float4 a = make_float4(0.f, 0.f, 0.f, __builtin_inff()), b = make_float4(0.f, 0.f, 0.f, 0.f);
  int32_t id = -1;
  if (h.kind >= 0) {
    f3 hn, alb;
    if (h.kind == 0) {
      const float4* r = reinterpret_cast<const float4*>(s_qshade + h.idx * kQShadeFloats);
      const float4 r0 = r[0], r1 = r[1];
      hn = mk(r0.x, r0.y, r0.z);
      alb = mk(r0.w, r1.x, r1.y);
    } else {
      const f3 hp = add(o, scl(d, h.t));
      const DevSphere& S = kBvh ? sc->sph_all[h.idx] : sc->spheres[h.idx];
      hn = mk((hp.x - S.c[0]) / S.r, (hp.y - S.c[1]) / S.r, (hp.z - S.c[2]) / S.r);
      alb = ld3(S.alb);
    }
    if (dot(hn, d) > 0.f) hn = neg(hn);
    a = make_float4(hn.x, hn.y, hn.z, h.t);
    b = make_float4(alb.x, alb.y, alb.z, 1.f);
    id = (h.kind << 24) + h.idx;
  }
  if (p.g0) reinterpret_cast<float4*>(p.g0)[i] = a;
  if (p.g1) reinterpret_cast<float4*>(p.g1)[i] = b;
  if (p.prim) p.prim[i] = id;
}

// RNG jump tables, all in one pass: thread s iterates the dead-step map from
// state s (= base + i) up to max_r steps and, after step r, stores the state
// into every table that tabulates r dead depths (out.t[r] != null: the chain
// tables for 32 / 16 / 8 / 4 ... depths and the direct tables of the counts
// a finished sample most often has).  The stores of a wave go to consecutive
// states, so each is one coalesced 256-byte write; the build costs max_r dead
// steps per state instead of the sum of every table's depth count.
__global__ void __launch_bounds__(256) rtp_build_ff_tables_kernel(FfBuildOut out, int max_r, uint32_t t1, uint32_t t2,
                                                                   uint64_t base, uint64_t count) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint32_t s = (uint32_t)(base + i);
  for (int r = 1; r <= max_r; r++) {
    s = dead_step(s, t1, t2);
    uint32_t* __restrict__ T = out.t[r];  // wave-uniform
    if (T != nullptr) T[base + i] = s;
  }
}

// Exhaustive equivalence check of a fast sequence against the IEEE operation
// for every float bit pattern in [lo, hi] (one lane per pattern).
__global__ void rtp_verify_fast_math_kernel(int kind, uint32_t lo, uint64_t count, unsigned long long* bad,
                                            uint32_t* first_bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t bits = lo + (uint32_t)i;
  const float x = __uint_as_float(bits);
  float want = 0.f, got = 0.f;
  switch (kind) {
    case 0: want = 1.0f / x; got = rcp_nr1(x); break;
    case 1: want = 1.0f / x; got = rcp_nr2(x); break;
    case 2: want = __builtin_sqrtf(x); got = sqrt_fast(x); break;
    case 3: want = 1.0f / __builtin_sqrtf(x); got = rcp_nr1(sqrt_fast(x)); break;
    case 4: want = 1.0f / __builtin_sqrtf(x); got = rcp_nr2(sqrt_fast(x)); break;
    case 5: want = (float)((double)x / kPi); got = cos_over_pi(x); break;
    case 6: { float s, c; rtp_sincosf(x, &s, &c); want = rtp_sinf(x); got = s; break; }
    case 7: { float s, c; rtp_sincosf(x, &s, &c); want = rtp_cosf(x); got = c; break; }
    case 8: {  // x as the divisor of div_markstein, 32 numerators spread over [-x, x] and beyond
      const float r = rcp_nr1(x);
      uint32_t h = bits;
      for (int k = 0; k < 32; k++) {
        h = wang(h + (uint32_t)k);
        const float a = x * ((float)(int32_t)h * 0x1p-31f) * (k < 24 ? 1.0f : 1024.0f);
        const float w = a / x, g = div_markstein(a, x, r);
        if (__float_as_uint(w) != __float_as_uint(g) && fabsf(w) >= 0x1p-120f) {  // (normal quotients)
          want = w;
          got = g;
          break;
        }
      }
      break;
    }
    default: break;
  }
  if (__float_as_uint(want) != __float_as_uint(got)) {
    atomicAdd(bad, 1ull);
    atomicMin(first_bad, bits);
  }
}

// One camera_ray() -- the render kernels' own, two draws -- per host row of
// (pixel index, seed), one lane per row, the pixel split into (i, j) as the
// render kernels split it.  out[5 r ..] = the direction, the seed after the
// draws, j * nx + i.
__global__ void __launch_bounds__(256) rtp_eval_raygen_kernel(DevCamera cam, int nx, int ny,
                                                              const int64_t* __restrict__ pixels,
                                                              const uint32_t* __restrict__ seeds, uint32_t* out,
                                                              int64_t n) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int64_t pix = pixels[r];
  const int pi = (int32_t)pix % nx, pj = (int32_t)pix / nx;
  uint32_t seed = seeds[r];
  const f3 d = camera_ray(cam, pi, pj, nx, ny, seed);
  uint32_t* w = out + 5 * r;
  w[0] = __float_as_uint(d.x), w[1] = __float_as_uint(d.y), w[2] = __float_as_uint(d.z);
  w[3] = seed;
  w[4] = (uint32_t)(pj * nx + pi);
}

}  // namespace rtp
