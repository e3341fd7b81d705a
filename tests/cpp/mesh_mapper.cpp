// mesh_mapper.cpp -- rtp::MapperPathTracer on a cell set of more than 256
// distinct quads (rtp/rendering.hpp chooses rtp_set_scene_mesh): reads a scene
// and a render's parameters from a file the test wrote, renders through
// RenderCells from the default camera and dumps the colour buffer raw.
//   mesh_mapper <scene.bin> <out.raw>
// scene.bin: 15 int32 (the counts of points, quads, spheres, materials,
// texture types and textures; the light quad's 4 point ids, the light sphere's
// point; nx, ny, samples, depth), then the arrays in the order of the reads
// below.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <vector>

#include "rtp/rendering.hpp"

template <class T>
static std::vector<T> take(std::ifstream& in, size_t n) {
  std::vector<T> v(n);
  in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)));
  return v;
}

int main(int argc, char** argv) {
  using namespace rtp;
  if (argc < 3) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  const std::vector<int32_t> h = take<int32_t>(in, 15);
  const int np = h[0], nq = h[1], ns = h[2], nm = h[3], ntt = h[4], nt = h[5];
  const std::vector<float> pts = take<float>(in, 3 * (size_t)np);
  const std::vector<int32_t> quads = take<int32_t>(in, 4 * (size_t)nq);
  std::vector<int32_t> matIdx[2], texIdx[2];
  matIdx[0] = take<int32_t>(in, nq), texIdx[0] = take<int32_t>(in, nq);
  const std::vector<int32_t> sph = take<int32_t>(in, ns);
  const std::vector<float> radii = take<float>(in, ns);
  matIdx[1] = take<int32_t>(in, ns), texIdx[1] = take<int32_t>(in, ns);
  std::vector<int32_t> matType = take<int32_t>(in, nm), texType = take<int32_t>(in, ntt);
  const std::vector<float> texf = take<float>(in, 3 * (size_t)nt);
  if (!in) {
    std::cerr << "mesh_mapper: short scene file" << std::endl;
    return 2;
  }
  CellSet cells;
  for (int q = 0; q < nq; q++) cells.quads.push_back({quads[4 * q], quads[4 * q + 1], quads[4 * q + 2], quads[4 * q + 3]});
  cells.spheres = sph;
  cells.radii = radii;
  CoordinateSystem coords;
  for (int p = 0; p < np; p++) coords.push_back(Vec3f(pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]));
  std::vector<Vec3f> tex;
  for (int t = 0; t < nt; t++) tex.push_back(Vec3f(texf[3 * t], texf[3 * t + 1], texf[3 * t + 2]));
  try {
    rendering::CanvasRayTracer canvas(h[11], h[12]);
    rendering::MapperPathTracer mapper(h[13], h[14], matIdx, texIdx, matType, texType, tex);
    mapper.SetLights({h[6], h[7], h[8], h[9]}, h[10]);
    mapper.SetCanvas(&canvas);
    mapper.RenderCells(cells, coords, rendering::Field(), rendering::ColorTable(), DefaultCamera(), rendering::Range());
    std::ofstream out(argv[2], std::ios::binary);
    out.write(reinterpret_cast<const char*>(canvas.GetColorBuffer().data()),
              (std::streamsize)(canvas.GetColorBuffer().size() * sizeof(Vec4f)));
  } catch (const std::exception& e) {
    std::cerr << "mesh_mapper: " << e.what() << std::endl;
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
