// rtp_mesh_host.cpp -- the host builder of a mesh scene's quad BVH
// (rtp_set_scene_mesh): descriptor checks, each quad's padded box
// (rtp_layout.hpp kMeshCosMin has the derivation), the binned-SAH tree and its
// eight threaded octant copies (rtp_bvh_host.hpp, shared with the sphere BVH),
// and the walk's compact nodes.  No HIP call: tests and stand-alone programs
// run it without a device (rtp_mesh_build_host).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "rtp_bvh_host.hpp"
#include "rtp_context.hpp"
#include "rtp_host_util.hpp"
#include "rtp_mesh.hpp"

namespace rtp_host {

namespace {
rtp_status bad(const char* msg) { return rtp_internal_fail(RTP_ERR_INVALID_ARGUMENT, msg); }

struct d3 {
  double x, y, z;
};
d3 operator-(d3 a, d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
double dotd(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
d3 crossd(d3 a, d3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double len(d3 a) { return std::sqrt(dotd(a, a)); }
d3 ldd(const float* p) { return {p[0], p[1], p[2]}; }

// The pad of one quad (v00 = q, v10 = r, v11 = s, v01 = t), in double:
// (kMeshRound reach / sine + h) / kMeshCosMin + the slab terms, or kMeshHuge
// for a strongly non-planar or degenerate quad (rtp_layout.hpp).
float quad_pad(d3 q, d3 r, d3 s, d3 t, double reach, double amax) {
  const d3 e01 = r - q, e03 = t - q, e21 = r - s, e23 = t - s;
  const d3 n1 = crossd(e01, e03);
  const double A1 = len(n1), A2 = len(crossd(e21, e23));
  const double l1 = len(e01) * len(e03), l2 = len(e21) * len(e23);
  if (!(A1 > 0) || !(A2 > 0) || !std::isfinite(A1) || !std::isfinite(A2)) return rtp::kMeshHuge;
  const double sine = std::min(A1 / l1, A2 / l2);
  if (!(sine >= rtp::kMeshMinSine)) return rtp::kMeshHuge;
  const double h = std::fabs(dotd(s - q, n1)) / A1;  // v11 off the first triangle's plane
  if (h > 0) {
    // the fold: v11's projection lies w beyond the diagonal (v10, v01), away from v00
    const d3 diag = t - r;
    d3 u1 = crossd(n1, diag);
    const double lu = len(u1);
    if (!(lu > 0)) return rtp::kMeshHuge;
    const double side = dotd(q - r, u1) < 0 ? 1.0 : -1.0;  // u1 points away from v00
    const double w = side * dotd(s - r, u1) / lu;
    if (!(w > 0) || !(h / w < 0.5 * rtp::kMeshCosMin)) return rtp::kMeshHuge;
  }
  const double slab = 1e-5 + 0x1p-16 * amax + 0x1p-18 * reach;
  const double pad = ((double)rtp::kMeshRound * reach / sine + h) / (double)rtp::kMeshCosMin + slab;
  if (!(pad < reach)) return rtp::kMeshHuge;
  return std::nextafter((float)pad, INFINITY);
}

// The pad of a triangle cell (v11 == v01: the reference's test accepts only
// its first triangle v00 = q, v10 = r, v01 = t): the roundings and the slab
// terms of quad_pad over the sine of the corner at v00 alone, no h and no fold
// (rtp_layout.hpp kMeshCosMin, "Triangle cells").
float tri_pad(d3 q, d3 r, d3 t, double reach, double amax) {
  const d3 e01 = r - q, e03 = t - q;
  const double A1 = len(crossd(e01, e03));
  const double l1 = len(e01) * len(e03);
  if (!(A1 > 0) || !std::isfinite(A1)) return rtp::kMeshHuge;
  const double sine = A1 / l1;
  if (!(sine >= rtp::kMeshMinSine)) return rtp::kMeshHuge;
  const double slab = 1e-5 + 0x1p-16 * amax + 0x1p-18 * reach;
  const double pad = ((double)rtp::kMeshRound * reach / sine) / (double)rtp::kMeshCosMin + slab;
  if (!(pad < reach)) return rtp::kMeshHuge;
  return std::nextafter((float)pad, INFINITY);
}

// the ordered key of a half: key k >= 0 is the half with bits k, k < 0 its negative
float half_value(int key) {
  const int b = key < 0 ? -key : key;
  const int e = b >> 10, m = b & 0x3ff;
  const float v = e == 0 ? std::ldexp((float)m, -24) : e == 31 ? INFINITY : std::ldexp((float)(m | 0x400), e - 25);
  return key < 0 ? -v : v;
}
// f32 -> f16 bits rounded outward: the smallest half >= x (up) or the largest <= x
uint32_t half_outward(float x, bool up) {
  if (std::isnan(x)) return up ? 0x7c00u : 0xfc00u;
  int lo = -0x7c00, hi = 0x7c00;  // -inf .. +inf
  if (up) {
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (half_value(mid) >= x) hi = mid;
      else lo = mid + 1;
    }
  } else {
    while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;
      if (half_value(mid) <= x) lo = mid;
      else hi = mid - 1;
    }
  }
  return lo < 0 ? 0x8000u | (uint32_t)(-lo) : (uint32_t)lo;
}
}  // namespace

rtp_status mesh_validate_head(const rtp_scene_desc* s) {
  if (!s) return bad("rtp_set_scene_mesh: NULL argument");
  if (s->n_points <= 0 || !s->points) return bad("rtp_set_scene: no points");
  if (s->n_quads < 0 || s->n_spheres < 0) return bad("rtp_set_scene: bad primitive counts");
  if (s->n_spheres < 1) return bad("rtp_set_scene: the light sphere radius is SphereRadii[0]; need >= 1 sphere");
  if (s->n_quads < 1 || s->n_quads > rtp::kMaxQuadsMesh)
    return bad("rtp_set_scene_mesh: a mesh scene takes 1 to 4194304 quads");
  if (s->n_spheres >= rtp::kBvhMinSpheres)
    return bad("rtp_set_scene_mesh: a mesh scene takes at most 8 spheres (no quad BVH together with a sphere BVH)");
  return RTP_OK;
}

rtp_status mesh_quad_fail(int check) {
  return bad(check == 0   ? "rtp_set_scene: quad point id out of range"
             : check == 1 ? "rtp_set_scene: quad material/texture index out of range"
                          : "rtp_set_scene_mesh: a quad vertex is not finite");
}

rtp_status mesh_validate_tail(const rtp_scene_desc* s) {
  for (int k = 0; k < s->n_spheres; k++)
    if (!pt_ok(s, s->sphere_point[k]) || !mat_ok(s, s->sphere_mat[k]) || !tex_ok(s, s->sphere_tex[k]) ||
        !(s->sphere_radius[k] > 0.0f))
      return bad("rtp_set_scene: sphere index or radius out of range");
  for (int k = 0; k < 4; k++)
    if (!pt_ok(s, s->light_quad_points[k])) return bad("rtp_set_scene: light quad point id out of range");
  if (!pt_ok(s, s->light_sphere_point)) return bad("rtp_set_scene: light sphere point id out of range");
  return RTP_OK;
}

rtp_status mesh_bounds_fail() { return bad("rtp_set_scene_mesh: the scene's bounds are not finite"); }

rtp_status mesh_validate(const rtp_scene_desc* s) {
  const rtp_status rs = mesh_validate_head(s);
  if (rs != RTP_OK) return rs;
  for (int q = 0; q < s->n_quads; q++) {
    for (int k = 0; k < 4; k++)
      if (!pt_ok(s, s->quad_points[4 * q + k])) return mesh_quad_fail(0);
    if (!mat_ok(s, s->quad_mat[q]) || !tex_ok(s, s->quad_tex[q])) return mesh_quad_fail(1);
    for (int k = 0; k < 4; k++)
      for (int a = 0; a < 3; a++)
        if (!std::isfinite(s->points[3 * s->quad_points[4 * q + k] + a])) return mesh_quad_fail(2);
  }
  return mesh_validate_tail(s);
}

rtp_status mesh_build(const rtp_scene_desc* s, MeshBuild& B, int leaf_size) {
  const rtp_status rs = mesh_validate(s);
  if (rs != RTP_OK) return rs;
  const int n = s->n_quads;
  // the reach: kBvhReachFactor diagonals of the scene's bounding box (every
  // quad vertex, every sphere's c -+ r), as for the sphere BVH
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int q = 0; q < n; q++)
    for (int c = 0; c < 4; c++)
      for (int k = 0; k < 3; k++) {
        const float v = s->points[3 * s->quad_points[4 * q + c] + k];
        lo[k] = std::min(lo[k], v), hi[k] = std::max(hi[k], v);
      }
  for (int j = 0; j < s->n_spheres; j++)
    for (int k = 0; k < 3; k++) {
      const float c = s->points[3 * s->sphere_point[j] + k], r = s->sphere_radius[j];
      lo[k] = std::min(lo[k], c - r), hi[k] = std::max(hi[k], c + r);
    }
  const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
  B.reach = rtp::kBvhReachFactor * std::sqrt(ex * ex + ey * ey + ez * ez);
  if (!std::isfinite(B.reach)) return mesh_bounds_fail();
  B.boxes.resize((size_t)6 * n);
  B.pads.resize(n);
  B.n_triangles = B.n_unbounded = 0;
  std::vector<BvhPrim> P(n);
  for (int q = 0; q < n; q++) {
    const float* v[4];
    for (int c = 0; c < 4; c++) v[c] = s->points + 3 * s->quad_points[4 * q + c];
    // a triangle cell: v11 and v01 compare equal (include/rtp_mesh.h)
    const bool tri = rtp::mesh_is_triangle(v[2], v[3]);
    float mn[3], mx[3];
    for (int k = 0; k < 3; k++) {
      if (tri) {  // the accepted region is the triangle: its three vertices
        mn[k] = std::min(std::min(v[0][k], v[1][k]), v[3][k]);
        mx[k] = std::max(std::max(v[0][k], v[1][k]), v[3][k]);
        continue;
      }
      // the four vertices and v00 + e01 + e03 with the device's float edges
      const float far = v[0][k] + (v[1][k] - v[0][k]) + (v[3][k] - v[0][k]);
      mn[k] = std::min(std::min(std::min(v[0][k], v[1][k]), std::min(v[2][k], v[3][k])), far);
      mx[k] = std::max(std::max(std::max(v[0][k], v[1][k]), std::max(v[2][k], v[3][k])), far);
    }
    double amax = 0;
    for (int k = 0; k < 3; k++) amax = std::max(amax, (double)std::max(std::fabs(mn[k]), std::fabs(mx[k])));
    const float pad = tri ? tri_pad(ldd(v[0]), ldd(v[1]), ldd(v[3]), B.reach, amax)
                          : quad_pad(ldd(v[0]), ldd(v[1]), ldd(v[2]), ldd(v[3]), B.reach, amax);
    B.pads[q] = pad;
    B.n_triangles += tri ? 1 : 0;
    B.n_unbounded += pad == rtp::kMeshHuge ? 1 : 0;
    for (int k = 0; k < 3; k++) {
      // (one step outward: the float sums may round toward the quad)
      P[q].lo[k] = B.boxes[6 * (size_t)q + k] = std::nextafter(mn[k] - pad, -INFINITY);
      P[q].hi[k] = B.boxes[6 * (size_t)q + 3 + k] = std::nextafter(mx[k] + pad, INFINITY);
      P[q].cen[k] = 0.5f * mn[k] + 0.5f * mx[k];
    }
    P[q].idx = q;
  }
  // The quads with unbounded boxes go under a subtree of their own beside the
  // tree of the others (one root above both): every ray tests them, and they
  // do not turn the SAH splits of the rest into index medians.
  const int n_fin = (int)(std::stable_partition(P.begin(), P.end(), [&](const BvhPrim& x) {
                            return B.pads[x.idx] < rtp::kMeshHuge;
                          }) - P.begin());
  std::vector<TNode> tree;
  B.order.clear();
  B.order.reserve(n);
  if (n_fin == 0 || n_fin == n) {
    bvh_build(P, 0, n, tree, B.order, leaf_size);
  } else {
    tree.emplace_back();  // node 0: the root, filled below
    TNode root;
    root.left = bvh_build(P, 0, n_fin, tree, B.order, leaf_size);
    root.right = bvh_build(P, n_fin, n, tree, B.order, leaf_size);
    for (int k = 0; k < 3; k++) {
      root.lo[k] = std::min(tree[root.left].lo[k], tree[root.right].lo[k]);
      root.hi[k] = std::max(tree[root.left].hi[k], tree[root.right].hi[k]);
    }
    tree[0] = root;
  }
  B.nodes.clear();
  for (int oct = 0; oct < 8; oct++) {
    std::vector<rtp::BvhNode> one;
    bvh_thread(
        tree, 0, oct, one, [](const TNode& t, rtp::BvhNode& nd) { nd.leaf = (t.first << 3) | t.count; },
        [](const TNode&, int, float, float) { return true; });
    B.n_nodes = (int)one.size();
    B.nodes.insert(B.nodes.end(), one.begin(), one.end());
  }
  return RTP_OK;
}

void mesh_compact(const rtp::BvhNode* nodes, int64_t total, uint32_t* out) {
  for (int64_t i = 0; i < total; i++) {
    const rtp::BvhNode& nd = nodes[i];
    uint32_t* w = out + 4 * i;
    w[0] = half_outward(nd.lo[0], false) | half_outward(nd.lo[1], false) << 16;
    w[1] = half_outward(nd.lo[2], false) | half_outward(nd.hi[0], true) << 16;
    w[2] = half_outward(nd.hi[1], true) | half_outward(nd.hi[2], true) << 16;
    w[3] = nd.leaf == 0 ? (uint32_t)nd.skip : rtp::kCBvhLeafBit | (uint32_t)nd.leaf;
  }
}

}  // namespace rtp_host

extern "C" {

rtp_status rtp_mesh_build_host(const rtp_scene_desc* scene, int32_t oct, int32_t node_cap, int32_t* n_nodes,
                               void* nodes, int32_t* order, float* boxes, float* pads, float* guarantee) {
  if (oct < 0 || oct > 7) return rtp_internal_fail(RTP_ERR_INVALID_ARGUMENT, "rtp_mesh_build_host: octant outside 0..7");
  rtp_host::MeshBuild B;
  const rtp_status rs = rtp_host::mesh_build(scene, B);
  if (rs != RTP_OK) return rs;
  if (n_nodes) *n_nodes = B.n_nodes;
  if (nodes) {
    if (node_cap < B.n_nodes) return rtp_internal_fail(RTP_ERR_INVALID_ARGUMENT, "rtp_mesh_build_host: node_cap too small");
    std::memcpy(nodes, B.nodes.data() + (size_t)oct * B.n_nodes, (size_t)B.n_nodes * sizeof(rtp::BvhNode));
  }
  if (order) std::memcpy(order, B.order.data(), B.order.size() * sizeof(int32_t));
  if (boxes) std::memcpy(boxes, B.boxes.data(), B.boxes.size() * sizeof(float));
  if (pads) std::memcpy(pads, B.pads.data(), B.pads.size() * sizeof(float));
  if (guarantee) guarantee[0] = rtp::kMeshCosMin, guarantee[1] = B.reach;
  return RTP_OK;
}

int32_t rtp_mesh_leaf_size(void) { return rtp::kMeshLeaf; }

void rtp_mesh_compact_host(const void* nodes, int64_t n, uint32_t* out) {
  rtp_host::mesh_compact(static_cast<const rtp::BvhNode*>(nodes), n, out);
}

// The brute-force scan of a descriptor's quads on the host, for tests: the
// Lagae-Dutre test in float32 as the reference states it (Surface.h:31-161:
// this file is compiled without contraction, and 1 / det is the IEEE
// quotient), every quad in index order with a strict '<', t > 0.001.  out: 2
// words per ray, the accepted t's bits and the winning quad (-1: none).  The
// spheres are not looked at.
rtp_status rtp_mesh_scan_host(const rtp_scene_desc* s, const float* rays, int64_t n, uint32_t* out) {
  const rtp_status rs = rtp_host::mesh_validate(s);
  if (rs != RTP_OK) return rs;
  if (!rays || !out || n < 0) return rtp_internal_fail(RTP_ERR_INVALID_ARGUMENT, "rtp_mesh_scan_host: bad arguments");
  struct V {
    float x, y, z;
  };
  auto sub = [](V a, V b) { return V{a.x - b.x, a.y - b.y, a.z - b.z}; };
  auto dot = [](V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; };
  auto cross = [](V a, V b) { return V{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; };
  auto ldv = [&](int32_t id) { return V{s->points[3 * id], s->points[3 * id + 1], s->points[3 * id + 2]}; };
  struct Q {
    V v00, v11, e01, e03, e21, e23;
  };
  std::vector<Q> quads(s->n_quads);
  for (int q = 0; q < s->n_quads; q++) {
    const int32_t* id = s->quad_points + 4 * q;
    const V a = ldv(id[0]), b = ldv(id[1]), c = ldv(id[2]), d = ldv(id[3]);
    quads[q] = Q{a, c, sub(b, a), sub(d, a), sub(b, c), sub(d, c)};
  }
  const float eps = 1e-5f;
  for (int64_t i = 0; i < n; i++) {
    const V o{rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]}, d{rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]};
    float best = 3.40282347e+38f;
    int32_t win = -1;
    for (int q = 0; q < s->n_quads; q++) {
      const Q& K = quads[q];
      const V P = cross(d, K.e03);
      const float det = dot(K.e01, P);
      if (std::fabs(det) < eps) continue;
      const float inv = 1.0f / det;
      const V T = sub(o, K.v00);
      const float alpha = dot(T, P) * inv;
      if (alpha < 0.0f) continue;
      const V Qv = cross(T, K.e01);
      const float beta = dot(d, Qv) * inv;
      if (beta < 0.0f) continue;
      const float t = dot(K.e03, Qv) * inv;
      if (t < 0.0f) continue;
      if (alpha + beta > 1.0f) {
        const V Pp = cross(d, K.e21);
        const float detp = dot(K.e23, Pp);
        if (std::fabs(detp) < eps) continue;
        const float invp = 1.0f / detp;
        const V Tp = sub(o, K.v11);
        if (dot(Tp, Pp) * invp < 0.0f) continue;
        const V Qp = cross(Tp, K.e23);
        if (dot(d, Qp) * invp < 0.0f) continue;
      }
      if (t > 0.001f && t < best) best = t, win = q;
    }
    uint32_t bits;
    std::memcpy(&bits, &best, 4);
    out[2 * i] = bits;
    out[2 * i + 1] = (uint32_t)win;
  }
  return RTP_OK;
}

}  // extern "C"
