// rtp_lbvh.hpp -- what the two device LBVH builders share (the sphere BVH,
// rtp_bvh_gpu.hip; the mesh BVH, rtp_mesh_gpu.hip): Morton bit spreading,
// Karras' binary radix tree over sorted keys (Karras 2012; equal keys split by
// position), and a node's depth-first position in the octant orders.  Device
// only.  Each builder keeps its own kernels and outputs around these.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace rtp {

// spread the low 10 bits of v to every third bit
__device__ __forceinline__ uint32_t expand_bits(uint32_t v) {
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}

// common-prefix length of sorted keys i and j (-1 outside); equal keys compare
// their positions, so every key is distinct
__device__ __forceinline__ int delta(const uint32_t* __restrict__ code, int n, int i, int j) {
  if (j < 0 || j >= n) return -1;
  const uint32_t a = code[i], b = code[j];
  if (a != b) return __clz(a ^ b);
  return 32 + __clz((uint32_t)i ^ (uint32_t)j);
}

// Internal node i (0..n-2, root 0) of the radix tree over n >= 2 sorted keys.
// Node ids: the tree's leaf j (sorted position) is n-1+j.
struct KarrasNode {
  int left, right;   // children
  int first, last;   // the node's range of sorted positions
  int dnode;         // the common-prefix length of its range
  int axis;          // split axis: the Morton bit the range splits on (x at bits 3k+2, y 3k+1, z 3k); bit 30
                     // (above the code: the mesh builder's class bit) and equal keys, split by position: x
};
__device__ __forceinline__ KarrasNode karras_node(const uint32_t* __restrict__ code, int n, int i) {
  const int d = (delta(code, n, i, i + 1) - delta(code, n, i, i - 1)) >= 0 ? 1 : -1;
  const int dmin = delta(code, n, i, i - d);
  int lmax = 2;
  while (delta(code, n, i, i + lmax * d) > dmin) lmax <<= 1;
  int l = 0;
  for (int t = lmax >> 1; t >= 1; t >>= 1)
    if (delta(code, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  KarrasNode k;
  k.dnode = delta(code, n, i, j);
  int s = 0;
  for (int div = 2;; div <<= 1) {
    const int t = (l + div - 1) / div;
    if (delta(code, n, i, i + (s + t) * d) > k.dnode) s += t;
    if (t == 1) break;
  }
  const int gamma = i + s * d + min(d, 0);
  k.first = min(i, j), k.last = max(i, j);
  k.left = (k.first == gamma) ? (n - 1 + gamma) : gamma;
  k.right = (k.last == gamma + 1) ? (n - 1 + gamma + 1) : gamma + 1;
  const int bit = 31 - k.dnode;
  k.axis = (k.dnode >= 32 || bit == 30) ? 0 : (bit % 3 == 2 ? 0 : (bit % 3 == 1 ? 1 : 2));
  return k;
}

// The depth-first position of node x in the octant orders oct0 .. oct0+kN-1
// (near child first on the parent's split axis), by one climb to the root.
// size: the number of nodes each subtree contributes to the order.
template <int kN>
__device__ __forceinline__ void octant_positions(int x, int oct0, const int2* __restrict__ child,
                                                 const int* __restrict__ parent, const int8_t* __restrict__ axis,
                                                 const int* __restrict__ size, int (&pos)[kN]) {
#pragma unroll
  for (int k = 0; k < kN; k++) pos[k] = 0;
  for (int c = x, p = parent[x]; p >= 0; c = p, p = parent[p]) {
    const int2 ch = child[p];
    const int ax = axis[p];
    const int before = 1 + size[c == ch.x ? ch.y : ch.x];  // ahead of a far child: p and the sibling's subtree
#pragma unroll
    for (int k = 0; k < kN; k++) {
      const bool neg = ((oct0 + k) >> ax) & 1;  // moving toward lower coordinates: right (upper) child first
      const int near = neg ? ch.y : ch.x;
      pos[k] += (c == near) ? 1 : before;
    }
  }
}

template <typename T>
hipError_t dalloc(T** p, size_t count) {
  return hipMalloc(reinterpret_cast<void**>(p), (count ? count : 1) * sizeof(T));
}

}  // namespace rtp
