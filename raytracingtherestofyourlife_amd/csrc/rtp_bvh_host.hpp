// rtp_bvh_host.hpp -- the host BVH builder shared by the sphere BVH
// (rtp_scene_host.cpp) and the mesh BVH (rtp_mesh_host.cpp): binned SAH over
// primitives given as boxes with a centroid.  Host only, no HIP call.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "rtp_layout.hpp"

namespace rtp_host {

// Binned SAH (16 bins per axis) with deterministic partitions, leaves of
// <= leaf_size primitives; `order` receives the primitives' indices in leaf
// order.
struct BvhPrim {
  float lo[3], hi[3], cen[3];
  int32_t idx;
};
struct TNode {
  float lo[3], hi[3];
  int axis = 0, left = -1, right = -1, first = 0, count = 0;
};

inline float half_area(const float lo[3], const float hi[3]) {
  const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
  return dx * dy + dy * dz + dz * dx;
}

inline int bvh_build(std::vector<BvhPrim>& P, int b, int e, std::vector<TNode>& T, std::vector<int32_t>& order,
                     int leaf_size = rtp::kBvhLeafSize) {
  const int me = (int)T.size();
  T.emplace_back();
  TNode nd;
  float clo[3], chi[3];
  for (int k = 0; k < 3; k++) {
    nd.lo[k] = clo[k] = INFINITY;
    nd.hi[k] = chi[k] = -INFINITY;
  }
  for (int i = b; i < e; i++)
    for (int k = 0; k < 3; k++) {
      nd.lo[k] = std::min(nd.lo[k], P[i].lo[k]);
      nd.hi[k] = std::max(nd.hi[k], P[i].hi[k]);
      clo[k] = std::min(clo[k], P[i].cen[k]);
      chi[k] = std::max(chi[k], P[i].cen[k]);
    }
  const int n = e - b;
  if (n <= leaf_size) {
    nd.first = (int)order.size();
    nd.count = n;
    for (int i = b; i < e; i++) order.push_back(P[i].idx);
    T[me] = nd;
    return me;
  }
  // binned SAH
  constexpr int kBins = 16;
  int best_ax = -1, best_split = 0;
  float best_cost = INFINITY;
  for (int ax = 0; ax < 3; ax++) {
    const float ext = chi[ax] - clo[ax];
    if (!(ext > 0)) continue;
    int cnt[kBins] = {};
    float blo[kBins][3], bhi[kBins][3];
    for (int j = 0; j < kBins; j++)
      for (int k = 0; k < 3; k++) blo[j][k] = INFINITY, bhi[j][k] = -INFINITY;
    for (int i = b; i < e; i++) {
      int j = (int)((P[i].cen[ax] - clo[ax]) / ext * kBins);
      j = std::min(kBins - 1, std::max(0, j));
      cnt[j]++;
      for (int k = 0; k < 3; k++) blo[j][k] = std::min(blo[j][k], P[i].lo[k]), bhi[j][k] = std::max(bhi[j][k], P[i].hi[k]);
    }
    for (int s = 1; s < kBins; s++) {  // split between bins s-1 and s
      float llo[3] = {INFINITY, INFINITY, INFINITY}, lhi[3] = {-INFINITY, -INFINITY, -INFINITY};
      float rlo[3] = {INFINITY, INFINITY, INFINITY}, rhi[3] = {-INFINITY, -INFINITY, -INFINITY};
      int nl = 0, nr = 0;
      for (int j = 0; j < kBins; j++) {
        if (!cnt[j]) continue;
        float* lo = j < s ? llo : rlo;
        float* hi = j < s ? lhi : rhi;
        (j < s ? nl : nr) += cnt[j];
        for (int k = 0; k < 3; k++) lo[k] = std::min(lo[k], blo[j][k]), hi[k] = std::max(hi[k], bhi[j][k]);
      }
      if (!nl || !nr) continue;
      const float cost = nl * half_area(llo, lhi) + nr * half_area(rlo, rhi);
      if (cost < best_cost) best_cost = cost, best_ax = ax, best_split = s;
    }
  }
  int mid;
  if (best_ax >= 0) {
    const int ax = best_ax;
    const float ext = chi[ax] - clo[ax];
    auto bin = [&](const BvhPrim& x) {
      return std::min(kBins - 1, std::max(0, (int)((x.cen[ax] - clo[ax]) / ext * kBins)));
    };
    mid = (int)(std::stable_partition(P.begin() + b, P.begin() + e, [&](const BvhPrim& x) { return bin(x) < best_split; }) -
                P.begin());
    nd.axis = ax;
  } else {  // coincident centroids: median split by index
    std::sort(P.begin() + b, P.begin() + e, [](const BvhPrim& x, const BvhPrim& y) { return x.idx < y.idx; });
    mid = b + n / 2;
    nd.axis = 0;
  }
  nd.left = bvh_build(P, b, mid, T, order, leaf_size);
  nd.right = bvh_build(P, mid, e, T, order, leaf_size);
  T[me] = nd;
  return me;
}

// Threaded flattening of one octant's near-to-far order (bit k of oct set:
// direction component k < 0): depth first, the child on the near side of the
// split axis first; `skip` is the first node after the subtree.  `leaf`
// fills a leaf node from its TNode (the primitive decides what it holds);
// `emit` says whether an inner node is kept (a dropped one's children take
// its place: its box counts as hit).
template <class Leaf, class Emit>
void bvh_thread(const std::vector<TNode>& T, int t, int oct, std::vector<rtp::BvhNode>& out, Leaf&& leaf, Emit&& emit,
                int depth = 0, float parent_area = 0.f) {
  const TNode& n = T[t];
  const float area = half_area(n.lo, n.hi);
  if (n.left >= 0 && !emit(n, depth, area, parent_area)) {
    const bool neg = (oct >> n.axis) & 1;
    const float pa = parent_area > 0.f ? parent_area : area;  // the nearest emitted ancestor's (or the root's)
    bvh_thread(T, neg ? n.right : n.left, oct, out, leaf, emit, depth + 1, pa);
    bvh_thread(T, neg ? n.left : n.right, oct, out, leaf, emit, depth + 1, pa);
    return;
  }
  const int me = (int)out.size();
  out.emplace_back();
  rtp::BvhNode nd{};
  const TNode& s = T[t];
  for (int k = 0; k < 3; k++) nd.lo[k] = s.lo[k], nd.hi[k] = s.hi[k];
  if (s.left < 0) {
    leaf(s, nd);
  } else {
    const bool neg = (oct >> s.axis) & 1;  // moving toward lower coordinates: right (upper) child first
    bvh_thread(T, neg ? s.right : s.left, oct, out, leaf, emit, depth + 1, area);
    bvh_thread(T, neg ? s.left : s.right, oct, out, leaf, emit, depth + 1, area);
    nd.leaf = 0;
  }
  nd.skip = (int32_t)out.size();
  out[me] = nd;
}

}  // namespace rtp_host
