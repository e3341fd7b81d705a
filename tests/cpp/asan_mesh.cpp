// asan_mesh.cpp -- the device-free builder of a mesh scene's quad BVH
// (csrc/rtp_mesh_host.cpp, rtp_mesh_build_host) under the host
// AddressSanitizer + UBSan (built by build.build_asan() like asan_scene.cpp).
//
// It creates no context and touches no device: a tessellated room of the
// size of tests/_meshes.py's tess and a 65 536-quad terrain, both generated
// here, go through the builder; the outputs are checked for shape, and the
// refusals decided before anything is built are exercised.  Prints "OK" and
// exits 0 when every check passes.
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

// a room's light (points 8..11 of three leading quads) over an nx x nz ridged terrain on shared vertices
struct Terrain {
  std::vector<float> pts;
  std::vector<int32_t> quads, mat, tex;
  int32_t sphere_point = 0, sphere_mat = 4, sphere_tex = 0;
  float radius = 0.1f;
  int32_t mat_type[5] = {0, 0, 0, 1, 2}, tex_type[5] = {0, 1, 2, 3, 0};
  float tex_rgb[12] = {0.65f, 0.05f, 0.05f, 0.73f, 0.73f, 0.73f, 0.12f, 0.45f, 0.15f, 15.f, 15.f, 15.f};
  rtp_scene_desc d{};

  int32_t point(float x, float y, float z) {
    pts.push_back(x), pts.push_back(y), pts.push_back(z);
    return (int32_t)(pts.size() / 3 - 1);
  }
  void quad(int32_t a, int32_t b, int32_t c, int32_t e, int32_t m) {
    quads.insert(quads.end(), {a, b, c, e});
    mat.push_back(m), tex.push_back(m);
  }
  Terrain(int nx, int nz) {
    for (int k = 0; k < 3; k++) {  // two walls and the light: points 0..11
      const float y = k == 2 ? 0.998f : 0.f, x0 = k == 2 ? 0.375f : (float)k, x1 = k == 2 ? 0.625f : (float)k;
      const int32_t a = k == 2 ? point(x0, y, 0.375f) : point(x0, 0, 0);
      const int32_t b = k == 2 ? point(x1, y, 0.375f) : point(x0, 1, 0);
      const int32_t c = k == 2 ? point(x1, y, 0.625f) : point(x0, 1, 1);
      const int32_t e = k == 2 ? point(x0, y, 0.625f) : point(x0, 0, 1);
      quad(a, b, c, e, k == 2 ? 3 : k);
    }
    sphere_point = point(0.5f, 0.5f, 0.5f);
    const int32_t base = (int32_t)(pts.size() / 3);
    for (int i = 0; i <= nx; i++)
      for (int j = 0; j <= nz; j++) point((float)i / nx, 0.05f * std::sin(9.f * i / nx), (float)j / nz);
    for (int i = 0; i < nx; i++)
      for (int j = 0; j < nz; j++) {
        const int32_t a = base + i * (nz + 1) + j;
        quad(a, a + nz + 1, a + nz + 2, a + 1, 1);
      }
    d.points = pts.data(), d.n_points = (int32_t)(pts.size() / 3);
    d.quad_points = quads.data(), d.quad_mat = mat.data(), d.quad_tex = tex.data(), d.n_quads = (int32_t)mat.size();
    d.sphere_point = &sphere_point, d.sphere_radius = &radius, d.sphere_mat = &sphere_mat, d.sphere_tex = &sphere_tex;
    d.n_spheres = 1;
    d.mat_type = mat_type, d.n_mat = 5, d.tex_type = tex_type, d.n_tex_type = 5, d.tex_rgb = tex_rgb, d.n_tex = 4;
    for (int k = 0; k < 4; k++) d.light_quad_points[k] = 8 + k;
    d.light_sphere_point = sphere_point;
    d.ior = 1.5f;
  }
};

static void build_and_check(int nx, int nz) {
  Terrain T(nx, nz);
  const int nq = T.d.n_quads;
  std::vector<Node> nodes((size_t)2 * nq);
  std::vector<int32_t> order(nq);
  std::vector<float> boxes((size_t)6 * nq), pads(nq);
  float g[2] = {0, 0};
  for (int oct = 0; oct < 8; oct += 7) {
    int32_t nn = 0;
    EXPECT(rtp_mesh_build_host(&T.d, oct, (int32_t)nodes.size(), &nn, nodes.data(), order.data(), boxes.data(),
                               pads.data(), g) == RTP_OK);
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
  EXPECT(rtp_mesh_build_host(&T.d, 0, 1, nullptr, nodes.data(), nullptr, nullptr, nullptr, nullptr) ==
         RTP_ERR_INVALID_ARGUMENT);  // node_cap too small
  // the host scan on a few rays from above: each hits the terrain or a wall
  const float rays[12] = {0.31f, 0.9f, 0.47f, 0.01f, -1.f, 0.02f, 0.7f, 0.5f, 0.2f, -1.f, -0.1f, 0.3f};
  uint32_t hit[4] = {0, 0, 0, 0};
  EXPECT(rtp_mesh_scan_host(&T.d, rays, 2, hit) == RTP_OK);
  EXPECT((int32_t)hit[1] >= 3 && (int32_t)hit[1] < nq);
  EXPECT((int32_t)hit[3] >= 0 && (int32_t)hit[3] < nq);
}

static void refusals() {
  Terrain T(4, 4);
  rtp_scene_desc d = T.d;
  d.n_quads = 0;
  EXPECT(rtp_mesh_build_host(&d, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == RTP_ERR_INVALID_ARGUMENT);
  d = T.d;
  d.n_spheres = 9;  // (refused on the count, before the arrays are read)
  EXPECT(rtp_mesh_build_host(&d, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == RTP_ERR_INVALID_ARGUMENT);
  d = T.d;
  T.quads[5] = T.d.n_points;
  EXPECT(rtp_mesh_build_host(&d, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == RTP_ERR_INVALID_ARGUMENT);
  T.quads[5] = 0;
  EXPECT(rtp_mesh_build_host(&d, 8, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == RTP_ERR_INVALID_ARGUMENT);
  EXPECT(rtp_mesh_build_host(nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
         RTP_ERR_INVALID_ARGUMENT);
}

int main() {
  build_and_check(23, 24);    // 555 quads, the size of the tessellated Cornell box
  build_and_check(256, 256);  // 65 536 terrain quads
  refusals();
  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
