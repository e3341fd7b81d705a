// rtp_base_host.cpp -- the part of the C ABI (include/rtp.h) that touches
// neither a context nor a device: the thread-local last error every unit of
// librtp.so reports through, the ABI version, and the image helpers of the
// reference's main.cc.  No HIP call: stand-alone programs link it without a
// device (tests/cpp/scene_build_check.cpp).
#include <cmath>
#include <cstdio>
#include <string>

#include "rtp_host_base.hpp"

using namespace rtp_host;

namespace {
thread_local std::string g_err;
}  // namespace

// error reporting for the other translation units of librtp.so
rtp_status rtp_internal_fail(rtp_status st, const std::string& msg) {
  g_err = msg;
  return st;
}

extern "C" {

const char* rtp_last_error(void) { return g_err.c_str(); }
int32_t rtp_abi_version(void) { return RTP_ABI_VERSION; }

// NormalizeFunctor (main.cc:253-287): de-NaN rgb, then sqrt(c / spp) on all
// four channels.
rtp_status rtp_normalize(float* rgba, int64_t n, int32_t spp) {
  if (!rgba || n < 0) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_normalize: bad arguments");
  const float samplecount = (float)spp;
  for (int64_t i = 0; i < n; i++) {
    float* px = rgba + 4 * i;
    for (int k = 0; k < 3; k++)
      if (!(px[k] == px[k])) px[k] = 0;
    for (int k = 0; k < 4; k++) px[k] = std::sqrt(px[k] / samplecount);
  }
  return RTP_OK;
}

// save() (main.cc:325-384): P3 header "nx ny 255", one "r g b" line per
// pixel in buffer order (row 0 = camera bottom), int(255.99*c) unclamped,
// NaN pixels written as 0.
rtp_status rtp_write_pnm(const char* path, const float* rgba, int32_t nx, int32_t ny) {
  if (!path || !rgba || nx <= 0 || ny <= 0) return fail(RTP_ERR_INVALID_ARGUMENT, "rtp_write_pnm: bad arguments");
  FILE* f = std::fopen(path, "w");
  if (!f) return fail(RTP_ERR_INVALID_ARGUMENT, std::string("Couldn't save pnm: ") + path);
  std::fprintf(f, "P3\n%d %d 255\n", nx, ny);
  const int64_t n = (int64_t)nx * ny;
  for (int64_t i = 0; i < n; i++) {
    float c[3] = {rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2]};
    if ((c[0] != c[0]) || (c[1] != c[1]) || (c[2] != c[2])) c[0] = c[1] = c[2] = 0.0f;
    std::fprintf(f, "%d %d %d\n", (int)(255.99 * c[0]), (int)(255.99 * c[1]), (int)(255.99 * c[2]));
  }
  std::fclose(f);
  return RTP_OK;
}

}  // extern "C"
