// asan_mesh_tri.cpp -- triangle cells (include/rtp_mesh.h: a cell (a, b, c, c))
// through the device-free builder of a mesh scene's BVH (csrc/rtp_mesh_host.cpp,
// rtp_mesh_build_host) under the host AddressSanitizer + UBSan, built by
// build.build_asan() like asan_mesh.cpp.
//
// It creates no context and touches no device: a curved terrain given as
// triangle cells and a mixed scene (planar quads, bent quads, triangle cells,
// slivers, degenerate cells), both generated here, go through the builder;
// the outputs are checked for shape and for what a triangle cell is promised
// (a bounded box around its three vertices), and the host scan runs over both.
// Prints "OK" and exits 0 when every check passes.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rtp.h"
#include "rtp_mesh.hpp"

static int failures = 0;
#define EXPECT(cond)                                               \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::fprintf(stderr, "FAIL %d: %s (%s)\n", __LINE__, #cond,  \
                   rtp_last_error() ? rtp_last_error() : "");      \
      failures++;                                                  \
    }                                                              \
  } while (0)

struct Node {  // rtp::BvhNode
  float lo[3];
  int32_t skip;
  float hi[3];
  int32_t leaf;
};

static const float kHuge = 0x1p100f;  // the pad of an unbounded box

// a room's light (points 8..11 of three leading quads), then cells added by the caller
struct Scene {
  std::vector<float> pts;
  std::vector<int32_t> cells, mat, tex;
  int32_t sphere_point = 0, sphere_mat = 4, sphere_tex = 0;
  float radius = 0.1f;
  int32_t mat_type[5] = {0, 0, 0, 1, 2}, tex_type[5] = {0, 1, 2, 3, 0};
  float tex_rgb[12] = {0.65f, 0.05f, 0.05f, 0.73f, 0.73f, 0.73f, 0.12f, 0.45f, 0.15f, 15.f, 15.f, 15.f};
  rtp_scene_desc d{};

  int32_t point(float x, float y, float z) {
    pts.push_back(x), pts.push_back(y), pts.push_back(z);
    return (int32_t)(pts.size() / 3 - 1);
  }
  void cell(int32_t a, int32_t b, int32_t c, int32_t e, int32_t m) {
    cells.insert(cells.end(), {a, b, c, e});
    mat.push_back(m), tex.push_back(m);
  }
  Scene() {
    for (int k = 0; k < 3; k++) {  // two walls and the light: points 0..11
      const float y = k == 2 ? 0.998f : 0.f, x0 = k == 2 ? 0.375f : (float)k, x1 = k == 2 ? 0.625f : (float)k;
      const int32_t a = k == 2 ? point(x0, y, 0.375f) : point(x0, 0, 0);
      const int32_t b = k == 2 ? point(x1, y, 0.375f) : point(x0, 1, 0);
      const int32_t c = k == 2 ? point(x1, y, 0.625f) : point(x0, 1, 1);
      const int32_t e = k == 2 ? point(x0, y, 0.625f) : point(x0, 0, 1);
      cell(a, b, c, e, k == 2 ? 3 : k);
    }
    sphere_point = point(0.5f, 0.5f, 0.5f);
  }
  // an nx x nz curved terrain on shared vertices: two triangle cells per cell, or one bent quad
  void hills(int nx, int nz, bool split) {
    const int32_t base = (int32_t)(pts.size() / 3);
    for (int i = 0; i <= nx; i++)
      for (int j = 0; j <= nz; j++) {
        const float x = (float)i / nx, z = (float)j / nz;
        point(x, 0.08f * (0.5f + 0.5f * std::sin(7.f * x + 1.f) * std::cos(5.f * z)) + 0.02f, z);
      }
    for (int i = 0; i < nx; i++)
      for (int j = 0; j < nz; j++) {
        const int32_t v00 = base + i * (nz + 1) + j, v10 = v00 + nz + 1, v11 = v10 + 1, v01 = v00 + 1;
        if (split) cell(v00, v10, v01, v01, 1), cell(v11, v01, v10, v10, 1);
        else cell(v00, v10, v11, v01, 1);
      }
  }
  const rtp_scene_desc* desc() {
    d.points = pts.data(), d.n_points = (int32_t)(pts.size() / 3);
    d.quad_points = cells.data(), d.quad_mat = mat.data(), d.quad_tex = tex.data(), d.n_quads = (int32_t)mat.size();
    d.sphere_point = &sphere_point, d.sphere_radius = &radius, d.sphere_mat = &sphere_mat, d.sphere_tex = &sphere_tex;
    d.n_spheres = 1;
    d.mat_type = mat_type, d.n_mat = 5, d.tex_type = tex_type, d.n_tex_type = 5, d.tex_rgb = tex_rgb, d.n_tex = 4;
    for (int k = 0; k < 4; k++) d.light_quad_points[k] = 8 + k;
    d.light_sphere_point = sphere_point;
    d.ior = 1.5f;
    return &d;
  }
};

struct Built {
  std::vector<float> boxes, pads;
  int unbounded = 0;
};

static Built build_and_check(Scene& S) {
  const rtp_scene_desc* d = S.desc();
  const int nq = d->n_quads;
  std::vector<Node> nodes((size_t)2 * nq);
  std::vector<int32_t> order(nq);
  Built B;
  B.boxes.resize((size_t)6 * nq), B.pads.resize(nq);
  float g[2] = {0, 0};
  for (int oct = 0; oct < 8; oct += 7) {
    int32_t nn = 0;
    EXPECT(rtp_mesh_build_host(d, oct, (int32_t)nodes.size(), &nn, nodes.data(), order.data(), B.boxes.data(),
                               B.pads.data(), g) == RTP_OK);
    EXPECT(nn >= 1 && nn <= 2 * nq);
    std::vector<int> seen(nq, 0);
    int64_t covered = 0;
    for (int i = 0; i < nn; i++) {
      EXPECT(nodes[i].skip > i && nodes[i].skip <= nn);
      if (nodes[i].leaf) {
        const int first = nodes[i].leaf >> 3, cnt = nodes[i].leaf & 7;
        EXPECT(cnt >= 1 && cnt <= rtp_mesh_leaf_size() && first + cnt <= nq);
        covered += cnt;
      }
    }
    EXPECT(covered == nq);
    for (int j = 0; j < nq; j++) {
      EXPECT(order[j] >= 0 && order[j] < nq);
      if (order[j] >= 0 && order[j] < nq) seen[order[j]]++;
    }
    for (int j = 0; j < nq; j++) EXPECT(seen[j] == 1);
  }
  EXPECT(g[0] > 0.f && g[0] < 0.1f && g[1] > 1.f);
  for (int q = 0; q < nq; q++) B.unbounded += B.pads[q] == kHuge;
  return B;
}

// a triangle cell's bounded box holds its three vertices and nothing a pad away from them
static void check_triangle_box(const Scene& S, const Built& B, int q) {
  const int32_t* id = S.cells.data() + 4 * q;
  EXPECT(B.pads[q] > 0.f && B.pads[q] < kHuge);
  for (int k = 0; k < 3; k++) {
    float mn = INFINITY, mx = -INFINITY;
    for (int c : {0, 1, 3}) mn = std::fmin(mn, S.pts[3 * id[c] + k]), mx = std::fmax(mx, S.pts[3 * id[c] + k]);
    EXPECT(B.boxes[6 * q + k] < mn - B.pads[q] * 0.999f && B.boxes[6 * q + k] > mn - B.pads[q] * 1.001f - 1e-6f);
    EXPECT(B.boxes[6 * q + 3 + k] > mx + B.pads[q] * 0.999f && B.boxes[6 * q + 3 + k] < mx + B.pads[q] * 1.001f + 1e-6f);
  }
}

static void scan(Scene& S) {
  // rays from above: each hits a cell; one along a terrain edge
  const float rays[18] = {0.31f, 0.9f, 0.47f, 0.01f, -1.f, 0.02f, 0.7f, 0.5f, 0.2f, -1.f, -0.1f, 0.3f,
                          0.25f, 0.6f, 0.25f, 0.f,   -1.f, 0.f};
  uint32_t hit[6] = {0, 0, 0, 0, 0, 0};
  EXPECT(rtp_mesh_scan_host(S.desc(), rays, 3, hit) == RTP_OK);
  for (int r = 0; r < 3; r++) EXPECT((int32_t)hit[2 * r + 1] >= 0 && (int32_t)hit[2 * r + 1] < S.d.n_quads);
}

static void triangle_terrain(int nx, int nz) {
  Scene S;
  S.hills(nx, nz, true);
  const Built B = build_and_check(S);
  EXPECT(B.unbounded == 0);  // no triangle of the curved terrain is unbounded
  for (int q = 3; q < S.d.n_quads; q += 7) check_triangle_box(S, B, q);
  scan(S);
}

static void mixed() {
  Scene S;
  S.hills(12, 12, true);   // 288 triangle cells
  S.hills(12, 12, false);  // the same surface again as 144 bent quads
  const int first_extra = (int)S.mat.size();
  // slivers: the corner at v00 from a right angle down to a sine of 2^-14, each with a repeated id
  for (int k = 0; k < 15; k++) {
    const float s = std::ldexp(1.f, -k), x = 0.1f + 0.05f * k;
    const int32_t a = S.point(x, 0.4f, 0.2f), b = S.point(x + 0.1f, 0.4f, 0.2f);
    const int32_t c = S.point(x + 0.1f * std::sqrt(1.f - s * s), 0.4f, 0.2f + 0.1f * s);
    S.cell(a, b, c, c, 2);
  }
  // equal by value, not by id; +0 against -0
  {
    const int32_t a = S.point(0.3f, 0.6f, 0.5f), b = S.point(0.4f, 0.62f, 0.5f);
    const int32_t c = S.point(0.0f, 0.65f, 0.55f), e = S.point(-0.0f, 0.65f, 0.55f);
    S.cell(a, b, c, e, 1);
  }
  // degenerate cells: all four ids one point; (a, a, c, c); a triangle with v10 == v00
  {
    const int32_t a = S.point(0.5f, 0.7f, 0.5f), c = S.point(0.6f, 0.7f, 0.6f);
    S.cell(a, a, a, a, 0);
    S.cell(a, a, c, c, 0);
    S.cell(a, c, a, a, 0);
  }
  const Built B = build_and_check(S);
  const int n_tri = 288, n_bent = 144;
  int unb_tri = 0, unb_bent = 0;
  for (int q = 3; q < 3 + n_tri; q++) unb_tri += B.pads[q] == kHuge;
  for (int q = 3 + n_tri; q < 3 + n_tri + n_bent; q++) unb_bent += B.pads[q] == kHuge;
  EXPECT(unb_tri == 0 && unb_bent > n_bent / 2);
  // the slivers: bounded down to a sine of 2^-9, unbounded from 2^-11 (at 2^-10 the pad is about the reach and
  // the float32 vertices decide)
  for (int k = 0; k < 15; k++) {
    if (k <= 9) check_triangle_box(S, B, first_extra + k);
    if (k >= 11) EXPECT(B.pads[first_extra + k] == kHuge);
  }
  check_triangle_box(S, B, first_extra + 15);
  for (int k = 16; k < 19; k++) EXPECT(B.pads[first_extra + k] == kHuge);  // no area: unbounded, never hit
  scan(S);
}

int main() {
  triangle_terrain(30, 30);    // the 1800 triangle cells of the tests' hills
  triangle_terrain(181, 181);  // 65 522 triangle cells
  mixed();
  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
