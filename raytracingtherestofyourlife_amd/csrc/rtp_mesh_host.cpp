// rtp_mesh_host.cpp -- the host builder of a mesh scene's quad BVH
// (rtp_set_scene_mesh): descriptor checks, the scene's bounds, each quad's
// padded box and record (rtp_mesh_cell.hpp: the functions the device builder
// calls too), the binned-SAH tree and its eight threaded octant copies
// (rtp_bvh_host.hpp, shared with the sphere BVH), and the walk's compact
// nodes.  No HIP call: tests and stand-alone programs run it without a device
// (rtp_mesh_build_host).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "rtp_bvh_host.hpp"
#include "rtp_host_base.hpp"
#include "rtp_mesh.hpp"

namespace rtp_host {

namespace {
rtp_status bad(const char* msg) { return rtp_internal_fail(RTP_ERR_INVALID_ARGUMENT, msg); }
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

void scene_bounds(const rtp_scene_desc* s, bool quads, float lo_io[3], float hi_io[3]) {
  float lo[3], hi[3];  // (locals: the caller's arrays could alias the points)
  for (int k = 0; k < 3; k++) lo[k] = lo_io[k], hi[k] = hi_io[k];
  for (int q = 0; q < (quads ? s->n_quads : 0); q++)
    for (int c = 0; c < 4; c++)
      for (int k = 0; k < 3; k++) {
        const float v = s->points[3 * s->quad_points[4 * q + c] + k];
        lo[k] = rtp::min_of(lo[k], v), hi[k] = rtp::max_of(hi[k], v);
      }
  for (int j = 0; j < s->n_spheres; j++)
    for (int k = 0; k < 3; k++) {
      const float c = s->points[3 * s->sphere_point[j] + k], r = s->sphere_radius[j];
      lo[k] = rtp::min_of(lo[k], c - r), hi[k] = rtp::max_of(hi[k], c + r);
    }
  for (int k = 0; k < 3; k++) lo_io[k] = lo[k], hi_io[k] = hi[k];
}

rtp_status mesh_build(const rtp_scene_desc* s, MeshBuild& B, int leaf_size) {
  const rtp_status rs = mesh_validate(s);
  if (rs != RTP_OK) return rs;
  const int n = s->n_quads;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  scene_bounds(s, true, lo, hi);
  B.reach = rtp::scene_reach(lo, hi);
  if (!rtp::finite_f(B.reach)) return mesh_bounds_fail();
  B.boxes.resize((size_t)6 * n);
  B.pads.resize(n);
  B.n_triangles = B.n_unbounded = 0;
  std::vector<BvhPrim> P(n);
  for (int q = 0; q < n; q++) {
    const int32_t* id = s->quad_points + 4 * q;
    const rtp::MeshCellBox c = rtp::mesh_cell_box(rtp::load_f3(s->points + 3 * id[0]), rtp::load_f3(s->points + 3 * id[1]),
                                                  rtp::load_f3(s->points + 3 * id[2]), rtp::load_f3(s->points + 3 * id[3]),
                                                  B.reach);
    B.pads[q] = c.pad;
    B.n_triangles += c.tri ? 1 : 0;
    B.n_unbounded += c.pad == rtp::kMeshHuge ? 1 : 0;
    for (int k = 0; k < 3; k++) {
      P[q].lo[k] = B.boxes[6 * (size_t)q + k] = c.lo[k];
      P[q].hi[k] = B.boxes[6 * (size_t)q + 3 + k] = c.hi[k];
      P[q].cen[k] = c.cen[k];
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
    w[0] = rtp::half_outward(nd.lo[0], false) | rtp::half_outward(nd.lo[1], false) << 16;
    w[1] = rtp::half_outward(nd.lo[2], false) | rtp::half_outward(nd.hi[0], true) << 16;
    w[2] = rtp::half_outward(nd.hi[1], true) | rtp::half_outward(nd.hi[2], true) << 16;
    w[3] = nd.leaf == 0 ? (uint32_t)nd.skip : rtp::kCBvhLeafBit | (uint32_t)nd.leaf;
  }
}

void fill_quad(rtp::DevQuad& Q, const float* q, const float* r, const float* s, const float* t, bool mesh) {
  const rtp::MeshCellRecord c =
      rtp::mesh_cell_record(rtp::load_f3(q), rtp::load_f3(r), rtp::load_f3(s), rtp::load_f3(t), mesh);
  std::memset(&Q, 0, sizeof(Q));
  for (int k = 0; k < 3; k++) {
    Q.vv[k][0] = q[k], Q.vv[k][1] = s[k];
    Q.e01[k] = (&c.e01.x)[k], Q.e03[k] = (&c.e03.x)[k];
    Q.e21[k] = (&c.e21.x)[k], Q.e23[k] = (&c.e23.x)[k];
    Q.n[k] = (&c.n.x)[k];
  }
  Q.para = c.para;
  Q.kind = c.kind;
}

void mesh_records(const rtp_scene_desc* s, const MeshBuild& build, std::vector<rtp::DevQuad>& quads,
                  std::vector<float>& shade) {
  const int n = s->n_quads;
  quads.resize(n);
  shade.assign((size_t)8 * n, 0.f);
  for (int j = 0; j < n; j++) {
    const int q = build.order[j];
    const int32_t* id = s->quad_points + 4 * q;
    rtp::DevQuad& Q = quads[j];
    fill_quad(Q, s->points + 3 * id[0], s->points + 3 * id[1], s->points + 3 * id[2], s->points + 3 * id[3], true);
    Q.mt = s->mat_type[s->quad_mat[q]];
    std::memcpy(Q.alb, s->tex_rgb + 3 * s->tex_type[s->quad_tex[q]], 12);
    Q.orig = q;
    Q.key_lo = (uint32_t)q;  // the caller's index: the hit's index and the tie-break of equal t
    float* sh = shade.data() + (size_t)8 * q;
    std::memcpy(sh, Q.n, 12);
    std::memcpy(sh + 3, Q.alb, 12);
    std::memcpy(sh + 6, &Q.mt, 4);
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
