// rtp_scene_host.cpp -- the host build of an inline scene (rtp_scene.hpp):
// the scene/material tables of vtkm::rendering::MapperPathTracer
// (MapperPathTracer.cxx:94-538) as the device reads them -- the quads with
// their prefilter tables, the sphere records and their BVH, the light
// constants.  All ray-independent quantities are precomputed here with the
// reference's own float operations (compiled with -ffp-contract=off; x86-64
// SSE2 arithmetic is IEEE single/double, the same as the reference's g++
// build).  No HIP call: rtp_host.cpp uploads the result, and stand-alone
// programs run the steps without a device (tests/cpp/scene_build_check.cpp).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtp.h"
#include "rtp_bvh_host.hpp"
#include "rtp_host_base.hpp"
#include "rtp_layout.hpp"
#include "rtp_mesh.hpp"
#include "rtp_scene.hpp"

namespace rtp_host {

namespace {

// which = min(3, int(r*3+1)), r = float(t)/4294967295.f  (PdfWorklet.h:20)
int which_of_hash(uint32_t t) {
  float r = (float)t / 4294967295.f;
  int w = (int)(r * 3 + 1);
  return w < 3 ? w : 3;
}

}  // namespace

// smallest hash value with which >= w (which is monotone in t)
uint32_t which_threshold(int w) {
  uint64_t lo = 0, hi = 0x100000000ull;  // answer in [lo, hi]
  while (lo < hi) {
    uint64_t mid = (lo + hi) / 2;
    if (which_of_hash((uint32_t)mid) >= w)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo > 0xffffffffull ? 0xffffffffu : (uint32_t)lo;
}

namespace {

bool bit_equal(const float* a, const float* b, int n) { return std::memcmp(a, b, sizeof(float) * n) == 0; }

// Closest-hit prefilter tables (rtp_kernels.hip closest_hit):
// the quads of groups 0..5 (kinds 1..6, edges along two axes) lie in a plane
// x[axis] = const, bit for bit.  Each gets that plane and a box around its
// vertices in the other two coordinates, widened outward by a few ulps so
// that the float box contains the real one.  Enabled only when every such
// quad qualifies, they fit kMaxPre, and the scene is within the coordinate
// range the kernel's error margins assume (|x| <= kPreLim).
constexpr float kPreLim = 16.0f;
void setup_prefilter(rtp::DevScene* h, const rtp_scene_desc* s, const std::vector<int>& kept) {
  h->n_pre = 0;
  for (int a = 0; a <= 3; a++) h->pre_begin[a] = 0;
  h->pre_scale = 0.0f;
  const int n = h->kind_begin[6];
  if (n <= 0 || n > rtp::kMaxPre) return;
  if (env_is("RTP_PREFILTER", '0')) return;
  std::vector<int> axis_of(n);
  std::vector<rtp::PreQuad> pq(n);
  float scale = 0.0f;
  for (int q = 0; q < n; q++) {
    const rtp::DevQuad& Q = h->quads[q];
    const rtp::QuadKindMasks& K = rtp::kQuadKind[Q.kind];
    const int flat = 7 & ~(K.m01 | K.m03);
    if (Q.kind < 1 || Q.kind > 6 || (flat != 1 && flat != 2 && flat != 4)) return;
    const int a = flat == 1 ? 0 : flat == 2 ? 1 : 2, b = (a + 1) % 3, c = (a + 2) % 3;
    if (!Q.para) return;  // (unreachable: kinds 1..6 are exact parallelograms, see mesh_cell_record)
    {
      const int ei = K.m01 == 1 ? 0 : K.m01 == 2 ? 1 : 2, ej = K.m03 == 1 ? 0 : K.m03 == 2 ? 1 : 2;
      const int ea = 3 - ei - ej;
      rtp::PreExact& E = h->prex[q];
      std::memset(&E, 0, sizeof(E));
      E.i = ei;
      E.s = (ej == (ei + 1) % 3) ? 1 : -1;
      E.b = Q.e01[ei], E.c = Q.e03[ej];
      E.bs = E.s > 0 ? E.b : -E.b, E.cs = E.s > 0 ? E.c : -E.c;
      E.vi = Q.vv[ei][0], E.va = Q.vv[ea][0], E.vj = Q.vv[ej][0];
      E.wi = Q.vv[ei][1], E.wa = Q.vv[ea][1], E.wj = Q.vv[ej][1];
      E.key_lo = Q.key_lo;
    }
    const int32_t* id = s->quad_points + 4 * kept[Q.orig];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const float x = s->points[3 * id[0] + a];
    for (int k = 0; k < 4; k++) {
      const float* v = s->points + 3 * id[k];
      if (!(v[a] == x)) return;  // not in one axis plane
      for (int j = 0; j < 3; j++) {
        if (!std::isfinite(v[j])) return;
        lo[j] = std::min(lo[j], (double)v[j]);
        hi[j] = std::max(hi[j], (double)v[j]);
        scale = std::max(scale, std::fabs(v[j]));
      }
    }
    auto centre_half = [&](int j, float& cen, float& half) {
      cen = (float)(0.5 * (lo[j] + hi[j]));
      const double need = std::max(hi[j] - (double)cen, (double)cen - lo[j]);
      half = (float)need;
      for (int u = 0; u < 2; u++) half = std::nextafter(half, INFINITY);  // >= need after rounding
    };
    rtp::PreQuad& P = pq[q];
    std::memset(&P, 0, sizeof(P));
    P.x = x;
    centre_half(b, P.cb, P.rb);
    centre_half(c, P.cc, P.rc);
    P.qpos = q;
    axis_of[q] = a;
  }
  if (!(scale <= kPreLim)) return;
  int pos = 0;
  for (int a = 0; a < 3; a++) {
    h->pre_begin[a] = pos;
    for (int q = 0; q < n; q++)
      if (axis_of[q] == a) h->pre[pos++] = pq[q];
  }
  h->pre_begin[3] = pos;
  h->pre_scale = scale;
  h->n_pre = n;
}

// Sphere BVH (replaces the VTK-m LinearBVH of buildBVH, MapperPathTracer.cxx:
// 437-449, for scenes with many spheres).  Binned SAH (16 bins per axis) with
// deterministic partitions, leaves of <= kBvhLeafSize spheres.  The tree is
// flattened eight times, once per ray-direction octant: each copy is a
// depth-first "threaded" array (hit: next node; miss or leaf done: skip) that
// visits the child on the near side of the split axis first, so a lane walks
// near-to-far without a stack and the closest-hit bound culls early.  Boxes
// only cull: each sphere box is padded (rtp_layout.hpp bvh_sphere_pad, from
// the roundings of the device's float sphere test) so that every ray that
// test accepts, and the point it returns, lie inside it, and the kernel
// compares against a slack-widened [0, t_best] interval.  The
// closest hit is the lexicographic min of (t, kind, index) whatever the order.
// (BvhPrim, TNode, bvh_build and the threaded flattening: rtp_bvh_host.hpp, shared with the mesh BVH)

// inner nodes of the sphere BVH above this depth are dropped from the walks'
// arrays (bvh_flatten below)
constexpr int kBvhDropDepth = 2;
constexpr float kBvhDropArea = 0.6f;  // (0: off)

// threaded flattening for one octant (bit k set: direction component k < 0)
// A one-sphere leaf carries the sphere itself (rtp::kBvhLeafSphere): lo =
// centre, hi[0] = r*r, hi[1] = the sphere's index (as int bits), so the walk
// runs the exact root test without a box test or a second dependent load.
// Inner nodes above depth `drop` are not emitted: their children take their
// place in the order (the skip of the node before them then lands on their
// first emitted descendant), so the walk treats their boxes as hit.  A box
// only culls, so this changes which nodes a ray visits, never its hit.  The
// top boxes (the whole sphere cloud, its halves) are hit by nearly every ray
// from inside the room: each one dropped is one dependent gather and box test
// fewer per walk.
// Below that, with drop_sa > 0, an inner node with two inner children is
// dropped too when its surface area exceeds drop_sa of its parent's (a ray
// that reaches it would hit its box with about that probability: dropping it
// saves one visit when it would be hit and costs one when it would not).
void bvh_flatten(const std::vector<TNode>& T, int t, int oct, const std::vector<int32_t>& order,
                 const std::vector<rtp::DevSphere>& sph, std::vector<rtp::BvhNode>& out, int drop = 0,
                 float drop_sa = 0.f) {
  bvh_thread(
      T, t, oct, out,
      [&](const TNode& s, rtp::BvhNode& nd) {
        if (RTP_BVH_EMBED && s.count == 1) {
          const rtp::DevSphere& S = sph[order[s.first]];
          std::memcpy(nd.lo, S.c, sizeof(nd.lo));
          nd.hi[0] = S.rr;
          int32_t orig = order[s.first];
          std::memcpy(&nd.hi[1], &orig, sizeof(orig));
          nd.hi[2] = 0.f;
          nd.leaf = rtp::kBvhLeafSphere;
        } else {
          nd.leaf = (s.first << 3) | s.count;
        }
      },
      [&](const TNode& n, int depth, float area, float parent_area) {
        const bool inner2 = T[n.left].left >= 0 && T[n.right].left >= 0;
        return !(depth < drop || (drop_sa > 0.f && inner2 && parent_area > 0.f && area > drop_sa * parent_area));
      });
}

}  // namespace

// rtp_set_scene in steps: extract + buildBVH (MapperPathTracer.cxx:178-197,
// 437-449) and the light coupling of the constructor (:141-148).  Every step
// works on the host only and may refuse the description; the upload
// (rtp_host.cpp scene_upload) then replaces the context's scene.

// (pt_ok, mat_ok, tex_ok: rtp_host_base.hpp, shared with the mesh builder)

// The quads: validated, de-duplicated, grouped by kind, with the prefilter
// tables and the -direct mode's bounds.  Quads that repeat an earlier quad
// bit-for-bit (same vertices in the same order, same material and texture --
// buildBox emits two such pairs per box, CornellBox.cpp:114-137) are dropped:
// under the strict '<' closest test the later copy can never win, so the hit
// record is unchanged.
rtp_status scene_quads(const rtp_scene_desc* s, SceneBuild& B) {
  if (s->n_points <= 0 || !s->points) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: no points");
  if (s->n_quads < 0 || s->n_spheres < 0 || s->n_spheres > rtp::kMaxSpheresBvh)
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: bad primitive counts");
  if (s->n_spheres < 1)
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: the light sphere radius is SphereRadii[0]; need >= 1 sphere");
  rtp::DevScene* h = B.fresh();
  std::vector<int>& kept = B.kept;
  std::vector<rtp::DevQuad> built;
  for (int q = 0; q < s->n_quads; q++) {
    const int32_t* id = s->quad_points + 4 * q;
    for (int k = 0; k < 4; k++)
      if (!pt_ok(s, id[k])) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: quad point id out of range");
    if (!mat_ok(s, s->quad_mat[q]) || !tex_ok(s, s->quad_tex[q]))
      return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: quad material/texture index out of range");
    bool dup = false;
    for (int j : kept) {
      const int32_t* jd = s->quad_points + 4 * j;
      bool same = s->quad_mat[j] == s->quad_mat[q] && s->quad_tex[j] == s->quad_tex[q];
      for (int k = 0; k < 4 && same; k++) same = bit_equal(s->points + 3 * jd[k], s->points + 3 * id[k], 3);
      if (same) {
        dup = true;
        break;
      }
    }
    if (dup) continue;
    if ((int)kept.size() >= rtp::kMaxQuads)
      return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: too many distinct quads");
    rtp::DevQuad Q;
    fill_quad(Q, s->points + 3 * id[0], s->points + 3 * id[1], s->points + 3 * id[2], s->points + 3 * id[3], false);
    Q.mt = s->mat_type[s->quad_mat[q]];
    st(Q.alb, ld(s->tex_rgb + 3 * s->tex_type[s->quad_tex[q]]));
    Q.orig = (int32_t)kept.size();  // rank in the reference's (index) order
    kept.push_back(q);
    built.push_back(Q);
  }
  // group by kind (scan order 1..kQuadKinds-1, then 0); the device scan
  // compares (t, orig) lexicographically, which is exactly the reference's
  // index-order strict '<' scan, so the grouping changes no result.
  {
    int pos = 0;
    for (int g = 0; g < rtp::kQuadKinds; g++) {
      const int kind = (g + 1) % rtp::kQuadKinds;
      h->kind_begin[g] = pos;
      for (const rtp::DevQuad& Q : built)
        if (Q.kind == kind) {
          h->quads[pos] = Q;
          h->quads[pos].key_lo = ((uint32_t)Q.orig << 8) | (uint32_t)pos;  // both < kMaxQuads = 256
          pos++;
        }
    }
    h->kind_begin[rtp::kQuadKinds] = pos;
    if (env_is("RTP_VERBOSE", '1')) {
      fprintf(stderr, "rtp: %d quads by scan group (kind: count / exact parallelograms):", pos);
      for (int g = 0; g < rtp::kQuadKinds; g++) {
        int np = 0;
        for (int i = h->kind_begin[g]; i < h->kind_begin[g + 1]; i++) np += h->quads[i].para ? 1 : 0;
        fprintf(stderr, " %d: %d/%d", (g + 1) % rtp::kQuadKinds, h->kind_begin[g + 1] - h->kind_begin[g], np);
      }
      fprintf(stderr, "\n");
    }
  }
  setup_prefilter(h, s, kept);
  h->n_quads = (int32_t)kept.size();
  // the -direct mode's shape bounds (union of the quads' padded AABBs,
  // AABBSurface.h:36-78)
  float* blo = B.blo;
  float* bhi = B.bhi;
  for (int k = 0; k < 3; k++) blo[k] = INFINITY, bhi[k] = -INFINITY;
  for (int q = 0; q < s->n_quads; q++) {
    const int32_t* id = s->quad_points + 4 * q;
    float mn[3], mx[3];
    for (int k = 0; k < 3; k++) mn[k] = mx[k] = s->points[3 * id[0] + k];
    for (int c2 = 1; c2 < 4; c2++)
      for (int k = 0; k < 3; k++) {
        const float v = s->points[3 * id[c2] + k];
        mn[k] = (v < mn[k]) ? v : mn[k];  // vtkm::Min / Max: (std::min)/(std::max)
        mx[k] = (mx[k] < v) ? v : mx[k];
      }
    for (int k = 0; k < 3; k++) {
      const float ext = 1.0e-4f * (mx[k] - mn[k]);
      const float eps = (1e-6f < ext) ? ext : 1e-6f;
      mn[k] -= eps;
      mx[k] += eps;
      blo[k] = std::min(blo[k], mn[k]);
      bhi[k] = std::max(bhi[k], mx[k]);
    }
  }
  return RTP_OK;
}

// The sphere records, whether they get a BVH, its pad's reach and its builder.
rtp_status scene_spheres(const rtp_scene_desc* s, SceneBuild& B) {
  std::vector<rtp::DevSphere>& sph = B.sph;
  sph.resize(s->n_spheres);
  for (int k = 0; k < s->n_spheres; k++) {
    if (!pt_ok(s, s->sphere_point[k]) || !mat_ok(s, s->sphere_mat[k]) || !tex_ok(s, s->sphere_tex[k]) ||
        !(s->sphere_radius[k] > 0.0f))
      return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: sphere index or radius out of range");
    rtp::DevSphere& S = sph[k];
    std::memset(&S, 0, sizeof(S));
    st(S.c, ld(s->points + 3 * s->sphere_point[k]));
    S.r = s->sphere_radius[k];
    S.rr = S.r * S.r;
    S.mt = s->mat_type[s->sphere_mat[k]];
    st(S.alb, ld(s->tex_rgb + 3 * s->tex_type[s->sphere_tex[k]]));
  }
  const bool use_bvh = B.use_bvh = s->n_spheres >= rtp::kBvhMinSpheres;
  // The reach of the sphere boxes' pad (rtp_layout.hpp bvh_sphere_pad):
  // kBvhReachFactor diagonals of the scene's bounding box -- every quad
  // vertex, every sphere's c -+ r.
  if (use_bvh) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    scene_bounds(s, true, lo, hi);
    B.bvh_reach = rtp::scene_reach(lo, hi);
  }
  // which builder makes the sphere BVH: the host's binned SAH (better trees,
  // O(n log n) on one core) or the device LBVH (rtp_bvh_gpu.hip) for large
  // scenes; RTP_BVH_BUILD=host|gpu overrides
  bool& gpu_build = B.gpu_build;
  gpu_build = use_bvh && s->n_spheres >= rtp::kBvhGpuMinSpheres;
  if (const char* bb = getenv("RTP_BVH_BUILD")) {
    if (!std::strcmp(bb, "gpu")) gpu_build = use_bvh;
    if (!std::strcmp(bb, "host")) gpu_build = false;
  }
  return RTP_OK;
}

// Where the spheres go: into the scene itself (few), or behind a BVH built on
// the device at upload (many) or here -- the global walk's tree and, opt-in,
// the LDS walk's.
void scene_sphere_bvh(const rtp_scene_desc* s, SceneBuild& B, int lds_walk_capacity) {
  rtp::DevScene* h = B.h.get();
  const std::vector<rtp::DevSphere>& sph = B.sph;
  const float bvh_reach = B.bvh_reach;
  std::vector<rtp::BvhNode>& nodes = B.nodes;
  std::vector<rtp::DevSphereG>& geom = B.geom;
  std::vector<rtp::BvhNode>& lw_nodes = B.lw_nodes;
  std::vector<int32_t>& lw_order = B.lw_order;
  int& lw_per_oct = B.lw_per_oct;
  if (!B.use_bvh) {
    for (int k = 0; k < s->n_spheres; k++) h->spheres[k] = sph[k];
  } else if (B.gpu_build) {
    h->n_nodes = 2 * s->n_spheres - 1;  // nodes and sphere records are built on the device (scene_upload)
  } else {
    std::vector<BvhPrim> P(s->n_spheres);
    for (int k = 0; k < s->n_spheres; k++) {
      const rtp::DevSphere& S = sph[k];
      // (the slab test's margin and what float32 sphere_root accepts beyond
      // the sphere: derived in rtp_layout.hpp; the same call in k_boxes)
      const float pad = rtp::bvh_sphere_pad(S.c[0], S.c[1], S.c[2], S.r, bvh_reach);
      for (int a = 0; a < 3; a++) {
        P[k].lo[a] = S.c[a] - S.r - pad;
        P[k].hi[a] = S.c[a] + S.r + pad;
        P[k].cen[a] = S.c[a];
      }
      P[k].idx = k;
    }
    const std::vector<BvhPrim> P0 = P;  // (bvh_build reorders P)
    std::vector<int32_t> order;
    std::vector<TNode> tree;
    bvh_build(P, 0, s->n_spheres, tree, order);
    // inner nodes above this depth are not emitted (bvh_flatten; RTP_BVH_DROP overrides)
    int drop = kBvhDropDepth;
    float drop_sa = kBvhDropArea;
    if (const char* dd = getenv("RTP_BVH_DROP")) drop = std::max(0, std::min(16, atoi(dd)));
    if (const char* da = getenv("RTP_BVH_DROP_SA")) drop_sa = (float)atof(da);
    // the copies the walk reads: octant o walks copy (o & oct_mask)
    // (RTP_BVH_OCT_MASK; the other copies are built the same and never read)
    int oct_mask = 7;
    if (const char* om = getenv("RTP_BVH_OCT_MASK")) oct_mask = atoi(om) & 7;
    h->oct_mask = oct_mask;
    int per_oct = 0;
    for (int oct = 0; oct < 8; oct++) {  // 8 copies of n_nodes entries, indices local to each copy
      std::vector<rtp::BvhNode> one;
      bvh_flatten(tree, 0, oct & oct_mask, order, sph, one, drop, drop_sa);
      per_oct = (int)one.size();  // (the same nodes are dropped in every octant's order)
      nodes.insert(nodes.end(), one.begin(), one.end());
    }
    // The LDS walk's tree (opt-in, RTP_BVH_LDS=1): leaves of up to
    // kLdsWalkLeaf spheres, flattened the same way, used when its 8 copies
    // plus the leaf spheres fit the block's LDS (the stats build and planned
    // launches walk the global tree).  On C3 at 16 spp (r04h/r04i, kernel ms):
    // LDS walk 324, the global walk over the same leaves-of-6 tree 349, the
    // global walk over the leaves-of-1 tree 186 -- the LDS copy saves 7% of the
    // texture-path gathers' cost, the bigger leaves it needs to fit cost 88%
    // (10 exact sphere tests per ray instead of 4: DESIGN.md 4.2).
    if (env_is("RTP_BVH_LDS", '1')) {
      std::vector<BvhPrim> P2 = P0;
      std::vector<TNode> tree2;
      bvh_build(P2, 0, s->n_spheres, tree2, lw_order, rtp::kLdsWalkLeaf);
      for (int oct = 0; oct < 8; oct++) {
        std::vector<rtp::BvhNode> one;
        bvh_flatten(tree2, 0, oct, lw_order, sph, one, drop, drop_sa);
        lw_per_oct = (int)one.size();
        lw_nodes.insert(lw_nodes.end(), one.begin(), one.end());
      }
      const int64_t bytes = (int64_t)16 * (8 * (int64_t)lw_per_oct + (int64_t)lw_order.size());
      if (bytes > lds_walk_capacity) {
        lw_nodes.clear();
        lw_order.clear();
        lw_per_oct = 0;
      }
    }
    geom.resize(order.size());
    for (size_t j = 0; j < order.size(); j++) {
      const rtp::DevSphere& S = sph[order[j]];
      std::memset(&geom[j], 0, sizeof(geom[j]));
      std::memcpy(geom[j].c, S.c, sizeof(S.c));
      geom[j].rr = S.rr;
      geom[j].orig = order[j];
    }
    h->n_nodes = (int32_t)per_oct;
  }
  h->n_spheres = s->n_spheres;
}

// lights (MapperPathTracer.cxx:141-148): light quad = light_box_pointids[1..4];
// the glass constants and the `which` thresholds
rtp_status scene_lights(const rtp_scene_desc* s, SceneBuild& B) {
  rtp::DevScene* h = B.h.get();
  const int32_t* lq = s->light_quad_points;
  for (int k = 0; k < 4; k++)
    if (!pt_ok(s, lq[k])) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: light quad point id out of range");
  if (!pt_ok(s, s->light_sphere_point))
    return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_set_scene: light sphere point id out of range");
  v3 q = ld(s->points + 3 * lq[0]), r = ld(s->points + 3 * lq[1]), ss = ld(s->points + 3 * lq[2]),
     t = ld(s->points + 3 * lq[3]);
  fill_quad(h->light.quad, &q.x, &r.x, &ss.x, &t.x, false);
  {
    float qr = std::sqrt(dot(sub(r, q), sub(r, q)));  // vtkm::Magnitude
    float qt = std::sqrt(dot(sub(t, q), sub(t, q)));
    h->light.area = qr * qt;  // PdfWorklet.h:236-239
  }
  // QuadWorkletGenerateDir uses pts[pointIndex[1]] and pts[pointIndex[3]]
  {
    float x0 = q.x, x1 = ss.x, z0 = q.z, z1 = ss.z, y0 = q.y, y1 = q.y;
    h->light.gx0 = x0, h->light.gdx = x1 - x0;
    h->light.gy0 = y0, h->light.gdy = y1 - y0;
    h->light.gz0 = z0, h->light.gdz = z1 - z0;
  }
  st(h->light.sc, ld(s->points + 3 * s->light_sphere_point));
  h->light.sr = s->sphere_radius[0];  // SphereRadii[0] (PdfWorklet.h:205-210)
  h->light.srr = h->light.sr * h->light.sr;
  h->ior = s->ior;
  {  // schlick's r0^2 and 1/ior with the reference's operations (float, float; double then float)
    float r0 = (1 - h->ior) / (1 + h->ior);
    h->ior_r0sq = r0 * r0;
    h->ior_inv = (float)(1.0 / h->ior);
  }
  h->which_t1 = which_threshold(2);
  h->which_t2 = which_threshold(3);
  return RTP_OK;
}

}  // namespace rtp_host
