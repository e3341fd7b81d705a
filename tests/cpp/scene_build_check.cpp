// scene_build_check.cpp -- the inline scene build (csrc/rtp_scene_host.cpp:
// scene_quads, scene_spheres, scene_sphere_bvh, scene_lights) as plain host
// C++ with a main of its own, linked with the other device-free units only
// (rtp_base_host.cpp, rtp_mesh_host.cpp, scene_cornell.cpp): no HIP header, no
// HIP library, no context.  The four Cornell variants and small hand-made
// descriptors against counts, messages and structure stated here.
// build.build_scene_build_check(), and sanitized by build.build_asan().
// Prints "OK" and exits 0 when every check passes.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rtp.h"
#include "rtp_layout.hpp"
#include "rtp_scene.hpp"

using rtp_host::SceneBuild;

static int failures = 0;
#define EXPECT(cond)                                             \
  do {                                                           \
    if (!(cond) && failures++ < 20) std::fprintf(stderr, "FAIL %d: %s (%s)\n", __LINE__, #cond, rtp_last_error()); \
  } while (0)

// the capacity the LDS walk's tree of the 1000-sphere Cornell variant just fits:
// 16 bytes per node of its 8 copies of 423 nodes and per leaf-order sphere
constexpr int kLwPerOct = 423;
constexpr int kLwFits = 16 * (8 * kLwPerOct + 1000);

// the steps of rtp_set_scene up to the upload; the first refusal ends them
static rtp_status build(const rtp_scene_desc* d, SceneBuild& B, int lds_capacity = kLwFits) {
  rtp_status st = rtp_host::scene_quads(d, B);
  if (st == RTP_OK) st = rtp_host::scene_spheres(d, B);
  if (st != RTP_OK) return st;
  rtp_host::scene_sphere_bvh(d, B, lds_capacity);
  return rtp_host::scene_lights(d, B);
}

static bool refused(const rtp_scene_desc* d, const char* msg) {
  SceneBuild B;
  return build(d, B) == RTP_ERR_INVALID_ARGUMENT && std::strcmp(rtp_last_error(), msg) == 0;
}

// ------------------------------------------------------------ structure ---
// kind_begin rises to n_quads; every key is orig << 8 | position, every orig once
static void check_quads(const SceneBuild& B) {
  const rtp::DevScene& h = *B.h;
  EXPECT(h.kind_begin[0] == 0 && h.kind_begin[rtp::kQuadKinds] == h.n_quads && h.n_quads == (int)B.kept.size());
  for (int g = 0; g < rtp::kQuadKinds; g++) EXPECT(h.kind_begin[g] <= h.kind_begin[g + 1]);
  std::vector<int> seen(B.kept.size(), 0);
  for (int pos = 0; pos < h.n_quads; pos++) {
    const rtp::DevQuad& Q = h.quads[pos];
    EXPECT(Q.orig >= 0 && Q.orig < h.n_quads && Q.key_lo == (((uint32_t)Q.orig << 8) | (uint32_t)pos));
    if (Q.orig >= 0 && Q.orig < h.n_quads) seen[Q.orig]++;
  }
  for (int s : seen) EXPECT(s == 1);
  for (size_t k = 1; k < B.kept.size(); k++) EXPECT(B.kept[k - 1] < B.kept[k]);
  EXPECT(h.n_pre >= 0 && h.n_pre <= rtp::kMaxPre && (h.n_pre == 0 || h.pre_begin[3] == h.n_pre));
}

// The reach as include/rtp.h states it: 2 diagonals of the box around every
// quad vertex and every sphere's c -+ r (in double; the build's is float).
static double reach_of(const rtp_scene_desc* d) {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int q = 0; q < 4 * d->n_quads; q++)
    for (int k = 0; k < 3; k++) {
      const double v = d->points[3 * d->quad_points[q] + k];
      lo[k] = std::fmin(lo[k], v), hi[k] = std::fmax(hi[k], v);
    }
  for (int j = 0; j < d->n_spheres; j++)
    for (int k = 0; k < 3; k++) {
      const double c = d->points[3 * d->sphere_point[j] + k], r = d->sphere_radius[j];
      lo[k] = std::fmin(lo[k], c - r), hi[k] = std::fmax(hi[k], c + r);
    }
  double s = 0;
  for (int k = 0; k < 3; k++) s += (hi[k] - lo[k]) * (hi[k] - lo[k]);
  return 2.0 * std::sqrt(s);
}

// One tree of 8 threaded octant copies of per_oct nodes over the spheres in
// leaf order `order`: skips, leaves, every sphere once per copy, and every
// emitted box around the padded spheres below it.
static void check_tree(const rtp_scene_desc* d, const SceneBuild& B, const std::vector<rtp::BvhNode>& nodes, int per_oct,
                       const std::vector<int32_t>& order) {
  const int n = d->n_spheres;
  EXPECT(per_oct > 0 && nodes.size() == (size_t)8 * per_oct && (int)order.size() == n);
  if (per_oct <= 0 || nodes.size() != (size_t)8 * per_oct || (int)order.size() != n) return;
  {
    std::vector<int> seen(n, 0);
    for (int32_t o : order) {
      EXPECT(o >= 0 && o < n);
      if (o >= 0 && o < n) seen[o]++;
    }
    for (int s : seen) EXPECT(s == 1);
  }
  const double want = reach_of(d);
  EXPECT(std::fabs((double)B.bvh_reach - want) <= 1e-6 * want);
  // each sphere grown by its pad, in the builder's float operations
  std::vector<float> glo(3 * (size_t)n), ghi(3 * (size_t)n);
  for (int k = 0; k < n; k++) {
    const float* c = d->points + 3 * d->sphere_point[k];
    const float r = d->sphere_radius[k];
    const float pad = rtp::bvh_sphere_pad(c[0], c[1], c[2], r, B.bvh_reach);
    EXPECT(pad > 0.f);
    for (int a = 0; a < 3; a++) glo[3 * k + a] = c[a] - r - pad, ghi[3 * k + a] = c[a] + r + pad;
  }
  std::vector<int32_t> members;  // the spheres of one leaf
  auto leaf_members = [&](const rtp::BvhNode& nd) {
    members.clear();
    if (nd.leaf == rtp::kBvhLeafSphere) {
      int32_t orig;
      std::memcpy(&orig, &nd.hi[1], sizeof(orig));
      EXPECT(orig >= 0 && orig < n);
      if (orig >= 0 && orig < n) {
        const float* c = d->points + 3 * d->sphere_point[orig];
        const float r = d->sphere_radius[orig];
        EXPECT(nd.lo[0] == c[0] && nd.lo[1] == c[1] && nd.lo[2] == c[2] && nd.hi[0] == r * r);
        members.push_back(orig);
      }
    } else {
      const int first = nd.leaf >> 3, count = nd.leaf & 7;
      EXPECT(count >= 1 && first >= 0 && first + count <= n);
      if (count >= 1 && first >= 0 && first + count <= n)
        for (int j = first; j < first + count; j++) members.push_back(order[j]);
    }
  };
  for (int oct = 0; oct < 8; oct++) {
    const rtp::BvhNode* N = nodes.data() + (size_t)oct * per_oct;
    std::vector<int> seen(n, 0);
    for (int i = 0; i < per_oct; i++) {
      EXPECT(N[i].skip > i && N[i].skip <= per_oct);
      if (N[i].leaf == 0) continue;
      EXPECT(N[i].skip == i + 1);
      leaf_members(N[i]);
      for (int32_t m : members) seen[m]++;
    }
    for (int s : seen) EXPECT(s == 1);
    // every emitted box (inner nodes and the leaves of several spheres) holds
    // the padded spheres of every leaf in its subtree, the nodes i .. skip - 1
    for (int i = 0; i < per_oct; i++) {
      if (N[i].leaf == rtp::kBvhLeafSphere) continue;
      const int end = N[i].skip > i && N[i].skip <= per_oct ? N[i].skip : i + 1;
      for (int j = i; j < end; j++) {
        if (N[j].leaf == 0) continue;
        leaf_members(N[j]);
        for (int32_t m : members)
          for (int a = 0; a < 3; a++) EXPECT(N[i].lo[a] <= glo[3 * m + a] && ghi[3 * m + a] <= N[i].hi[a]);
      }
    }
  }
}

static std::vector<int32_t> global_order(const SceneBuild& B) {
  std::vector<int32_t> order;
  for (const rtp::DevSphereG& g : B.geom) order.push_back(g.orig);
  return order;
}

// ------------------------------------------------------------- Cornell ---
static void cornell() {
  const int want_pre[4] = {12, 12, 12, 6}, want_quads[4] = {18, 18, 18, 6};
  rtp_scene_desc d{};
  for (int v = 0; v < 4; v++) {
    SceneBuild B;
    EXPECT(rtp_cornell_box(v, &d) == RTP_OK && build(&d, B) == RTP_OK);
    check_quads(B);
    EXPECT(B.h->n_pre == want_pre[v] && B.h->n_quads == want_quads[v] && B.h->n_spheres == d.n_spheres);
    EXPECT(B.lw_nodes.empty() && B.lw_order.empty() && B.lw_per_oct == 0);
    if (v < 3) {
      EXPECT(!B.use_bvh && B.nodes.empty() && B.geom.empty() && B.h->n_nodes == 0);
    } else {
      EXPECT(B.use_bvh && !B.gpu_build && d.n_spheres == 1000);
      EXPECT(B.nodes.size() == 15000 && B.h->n_nodes == 1875 && B.geom.size() == 1000 && B.h->oct_mask == 7);
      check_tree(&d, B, B.nodes, B.h->n_nodes, global_order(B));
      for (size_t j = 0; j < B.geom.size(); j++) {
        const int32_t o = B.geom[j].orig;
        const float* c = d.points + 3 * d.sphere_point[o];
        EXPECT(B.geom[j].c[0] == c[0] && B.geom[j].c[1] == c[1] && B.geom[j].c[2] == c[2] &&
               B.geom[j].rr == d.sphere_radius[o] * d.sphere_radius[o]);
      }
    }
  }
}

// the 1000-sphere variant under the switches of the host build
static void cornell_switches() {
  rtp_scene_desc d{};
  EXPECT(rtp_cornell_box(3, &d) == RTP_OK);
  setenv("RTP_BVH_LDS", "1", 1);
  {  // the LDS walk's tree: kept when its 8 copies and leaf spheres fit the capacity, dropped one byte below
    SceneBuild fits, tight;
    EXPECT(build(&d, fits, kLwFits) == RTP_OK && build(&d, tight, kLwFits - 1) == RTP_OK);
    EXPECT(fits.lw_per_oct == kLwPerOct && fits.lw_nodes.size() == (size_t)8 * kLwPerOct && fits.lw_order.size() == 1000);
    check_tree(&d, fits, fits.lw_nodes, fits.lw_per_oct, fits.lw_order);
    EXPECT(tight.lw_per_oct == 0 && tight.lw_nodes.empty() && tight.lw_order.empty());
    EXPECT(fits.nodes.size() == 15000 && tight.nodes.size() == 15000);  // (the global tree is built either way)
  }
  unsetenv("RTP_BVH_LDS");
  setenv("RTP_BVH_DROP", "0", 1);
  setenv("RTP_BVH_DROP_SA", "0", 1);
  {  // nothing dropped: the whole binary tree over leaves of one sphere, 2 n - 1 nodes per copy
    SceneBuild B;
    EXPECT(build(&d, B) == RTP_OK);
    EXPECT(B.h->n_nodes == 1999 && B.nodes.size() == (size_t)8 * 1999 && B.geom.size() == 1000);
    check_tree(&d, B, B.nodes, B.h->n_nodes, global_order(B));
  }
  unsetenv("RTP_BVH_DROP");
  unsetenv("RTP_BVH_DROP_SA");
  setenv("RTP_BVH_OCT_MASK", "0", 1);
  {  // every octant walks copy 0's order
    SceneBuild B;
    EXPECT(build(&d, B) == RTP_OK);
    EXPECT(B.h->oct_mask == 0 && B.nodes.size() == 15000);
    for (int oct = 1; oct < 8 && B.nodes.size() == 15000; oct++)
      EXPECT(std::memcmp(B.nodes.data(), B.nodes.data() + (size_t)oct * 1875, 1875 * sizeof(rtp::BvhNode)) == 0);
    check_tree(&d, B, B.nodes, B.h->n_nodes, global_order(B));
  }
  unsetenv("RTP_BVH_OCT_MASK");
}

// ---------------------------------------------------- small descriptors ---
// A scene of unit squares z = const (points 4 q .. 4 q + 3 of quad q), spheres
// with a centre point each behind them, three materials and two textures; the
// light is quad 0 and sphere 0.
struct Small {
  std::vector<float> points;
  std::vector<int32_t> quad_points, quad_mat, quad_tex, sphere_point, sphere_mat, sphere_tex;
  std::vector<float> sphere_radius;
  int32_t mat_type[3] = {0, 1, 2}, tex_type[2] = {0, 1};
  float tex_rgb[6] = {0.5f, 0.25f, 0.125f, 15.f, 15.f, 15.f};
  rtp_scene_desc d{};

  void quad(float z) {
    const float p[4][3] = {{0, 0, z}, {1, 0, z}, {1, 1, z}, {0, 1, z}};
    for (int i = 0; i < 4; i++) {
      quad_points.push_back((int32_t)(points.size() / 3));
      points.insert(points.end(), p[i], p[i] + 3);
    }
    quad_mat.push_back(0), quad_tex.push_back(0);
  }
  void sphere(float x, float y, float z, float r) {
    sphere_point.push_back((int32_t)(points.size() / 3));
    points.insert(points.end(), {x, y, z});
    sphere_radius.push_back(r), sphere_mat.push_back(2), sphere_tex.push_back(1);
  }
  const rtp_scene_desc* desc() {
    d.points = points.data(), d.n_points = (int32_t)(points.size() / 3);
    d.quad_points = quad_points.data(), d.quad_mat = quad_mat.data(), d.quad_tex = quad_tex.data();
    d.n_quads = (int32_t)quad_mat.size();
    d.sphere_point = sphere_point.data(), d.sphere_radius = sphere_radius.data();
    d.sphere_mat = sphere_mat.data(), d.sphere_tex = sphere_tex.data(), d.n_spheres = (int32_t)sphere_radius.size();
    d.mat_type = mat_type, d.n_mat = 3, d.tex_type = tex_type, d.n_tex_type = 2, d.tex_rgb = tex_rgb, d.n_tex = 2;
    for (int k = 0; k < 4; k++) d.light_quad_points[k] = quad_points[k];
    d.light_sphere_point = sphere_point[0];
    d.ior = 1.5f;
    return &d;
  }
};

// which = min(3, int(r * 3 + 1)), r = float(t) / 4294967295.f (PdfWorklet.h:20)
static int which_of(uint32_t t) {
  const float r = (float)t / 4294967295.f;
  const int w = (int)(r * 3 + 1);
  return w < 3 ? w : 3;
}

static void small_scenes() {
  {  // one quad and one sphere
    Small s;
    s.quad(0.f), s.sphere(0.5f, 0.5f, 2.f, 0.25f);
    SceneBuild B;
    EXPECT(build(s.desc(), B) == RTP_OK);
    check_quads(B);
    const rtp::DevScene& h = *B.h;
    EXPECT(h.n_quads == 1 && B.kept == std::vector<int>{0} && h.n_pre == 1 && h.pre_scale == 1.f);
    EXPECT(h.quads[0].key_lo == 0u && h.quads[0].mt == 0 && h.quads[0].alb[0] == 0.5f && h.quads[0].alb[2] == 0.125f);
    EXPECT(h.quads[0].e01[0] == 1.f && h.quads[0].e03[1] == 1.f && h.quads[0].para != 0);
    EXPECT(h.n_spheres == 1 && !B.use_bvh && B.nodes.empty() && B.geom.empty());
    EXPECT(h.spheres[0].c[2] == 2.f && h.spheres[0].r == 0.25f && h.spheres[0].rr == 0.0625f && h.spheres[0].mt == 2 &&
           h.spheres[0].alb[1] == 15.f);
    EXPECT(h.light.area == 1.f && h.light.sr == 0.25f && h.light.srr == 0.0625f && h.light.sc[0] == 0.5f);
    EXPECT(h.light.gx0 == 0.f && h.light.gdx == 1.f && h.light.gdy == 0.f && h.light.gdz == 0.f);
    EXPECT(h.ior == 1.5f && h.ior_inv == (float)(1.0 / 1.5) && h.ior_r0sq == (-0.5f / 2.5f) * (-0.5f / 2.5f));
    EXPECT(which_of(h.which_t1) == 2 && which_of(h.which_t1 - 1) == 1);
    EXPECT(which_of(h.which_t2) == 3 && which_of(h.which_t2 - 1) == 2);
    // the -direct mode's bounds: each axis widened by 1e-4 of its extent, at least 1e-6
    for (int k = 0; k < 2; k++) EXPECT(B.blo[k] == -1e-4f && B.bhi[k] == 1.f + 1e-4f);
    EXPECT(B.blo[2] == -1e-6f && B.bhi[2] == 1e-6f);
  }
  {  // two bit-identical quads: the second is dropped
    Small s;
    s.quad(0.f), s.quad(0.f), s.sphere(0.5f, 0.5f, 2.f, 0.25f);
    SceneBuild B;
    EXPECT(build(s.desc(), B) == RTP_OK);
    check_quads(B);
    EXPECT(B.h->n_quads == 1 && B.kept == std::vector<int>{0});
  }
  {  // kMaxQuads distinct quads fit, one more is refused
    Small s;
    for (int q = 0; q < rtp::kMaxQuads; q++) s.quad(0.01f * (float)q);
    s.sphere(0.5f, 0.5f, -2.f, 0.25f);
    SceneBuild B;
    EXPECT(rtp::kMaxQuads == 256 && build(s.desc(), B) == RTP_OK && B.h->n_quads == 256);
    check_quads(B);
    s.quad(0.01f * 256.f);
    EXPECT(s.quad_mat.size() == 257 && refused(s.desc(), "rtp_set_scene: too many distinct quads"));
  }
  for (float z : {17.f, 16.f}) {  // the prefilter's coordinate range ends at 16
    Small s;
    s.quad(z), s.sphere(0.5f, 0.5f, 2.f, 0.25f);
    SceneBuild B;
    EXPECT(build(s.desc(), B) == RTP_OK && B.h->n_quads == 1);
    EXPECT(B.h->n_pre == (z == 16.f ? 1 : 0) && B.h->pre_scale == (z == 16.f ? 16.f : 0.f));
  }
  {  // ids out of range, each with its message
    Small s;
    s.quad(0.f), s.sphere(0.5f, 0.5f, 2.f, 0.25f);
    s.desc();
    s.quad_points[2] = s.d.n_points;
    EXPECT(refused(&s.d, "rtp_set_scene: quad point id out of range"));
    s.quad_points[2] = -1;
    EXPECT(refused(&s.d, "rtp_set_scene: quad point id out of range"));
    s.quad_points[2] = 2;
    s.quad_mat[0] = 3;
    EXPECT(refused(&s.d, "rtp_set_scene: quad material/texture index out of range"));
    s.quad_mat[0] = 0;
    s.quad_tex[0] = 2;
    EXPECT(refused(&s.d, "rtp_set_scene: quad material/texture index out of range"));
    s.quad_tex[0] = 0;
    for (float r : {0.f, -1.f, NAN}) {
      s.sphere_radius[0] = r;
      EXPECT(refused(&s.d, "rtp_set_scene: sphere index or radius out of range"));
    }
    s.sphere_radius[0] = 0.25f;
    s.sphere_point[0] = s.d.n_points;
    EXPECT(refused(&s.d, "rtp_set_scene: sphere index or radius out of range"));
    s.sphere_point[0] = 4;
    s.d.light_quad_points[3] = s.d.n_points;
    EXPECT(refused(&s.d, "rtp_set_scene: light quad point id out of range"));
    s.d.light_quad_points[3] = 3;
    s.d.light_sphere_point = -1;
    EXPECT(refused(&s.d, "rtp_set_scene: light sphere point id out of range"));
    s.d.light_sphere_point = 4;
    SceneBuild B;
    EXPECT(build(&s.d, B) == RTP_OK);  // (put back whole, it builds)
  }
  for (int n : {rtp::kBvhMinSpheres - 1, rtp::kBvhMinSpheres}) {  // inline spheres, or a BVH from kBvhMinSpheres on
    Small s;
    s.quad(0.f);
    for (int k = 0; k < n; k++) s.sphere(0.1f * (float)k, 0.5f + 0.03f * (float)(k * k % 7), 1.f + 0.2f * (float)(k % 3), 0.04f);
    SceneBuild B;
    EXPECT(rtp::kBvhMinSpheres == 9 && build(s.desc(), B) == RTP_OK && B.h->n_spheres == n);
    if (n < rtp::kBvhMinSpheres) {
      EXPECT(!B.use_bvh && B.nodes.empty() && B.geom.empty() && B.h->n_nodes == 0);
      for (int k = 0; k < n; k++) EXPECT(B.h->spheres[k].c[0] == 0.1f * (float)k && B.h->spheres[k].r == 0.04f);
    } else {
      EXPECT(B.use_bvh && !B.gpu_build && (int)B.geom.size() == n && B.h->n_nodes >= 1);
      check_tree(s.desc(), B, B.nodes, B.h->n_nodes, global_order(B));
    }
  }
}

int main() {
  setenv("RTP_BVH_BUILD", "host", 1);
  for (const char* e : {"RTP_BVH_LDS", "RTP_BVH_DROP", "RTP_BVH_DROP_SA", "RTP_BVH_OCT_MASK", "RTP_PREFILTER"}) unsetenv(e);
  cornell();
  cornell_switches();
  small_scenes();
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
