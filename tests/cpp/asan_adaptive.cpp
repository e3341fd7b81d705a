// asan_adaptive.cpp -- the host-only part of the adaptive entry points
// (include/rtp_adaptive.h) under the host AddressSanitizer + UBSan (built by
// build.build_asan() like asan_scene.cpp: every host translation unit of
// librtp sanitized, device code unchanged).
//
// It creates no context and touches no device: rtp_normalize_counts, and the
// refusals of rtp_refine and rtp_noise that are decided before a context is
// used.  The adaptive passes themselves (scratch growth, gather, resume,
// scatter) are not run under a sanitizer: that would put a sanitized process
// on the GPU.  Prints "OK" and exits 0 when every check passes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rtp_adaptive.h"

static int failures = 0;
#define EXPECT(cond)                                               \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::fprintf(stderr, "FAIL %d: %s (%s)\n", __LINE__, #cond,  \
                   rtp_last_error() ? rtp_last_error() : "");      \
      failures++;                                                  \
    }                                                              \
  } while (0)

static rtp_camera cornell_camera() {
  // main.cc:616-622 (rtp::DefaultCamera)
  rtp_camera c{};
  const float a = (float)(278 / 555.0), b = (float)(-800 / 555.0);
  for (int k = 0; k < 3; k++) c.position[k] = k == 2 ? b : a, c.look_at[k] = a, c.view_up[k] = k == 1 ? 1.f : 0.f;
  c.fov_y_deg = 40.f;
  return c;
}

static void host_helpers() {
  std::vector<float> px = {4.f, NAN, 16.f, 0.f, 9.f, 1.f, 4.f, 0.f};
  const std::vector<int32_t> count = {4, 1};
  EXPECT(rtp_normalize_counts(px.data(), count.data(), 2) == RTP_OK);
  EXPECT(px[0] == 1.f && px[1] == 0.f && px[2] == 2.f && px[4] == 3.f && px[6] == 2.f);
  EXPECT(rtp_normalize_counts(nullptr, count.data(), 2) == RTP_ERR_INVALID_ARGUMENT);
  const rtp_camera cam = cornell_camera();
  const rtp_refine_params prm{0.1f, 4, 16};
  int64_t sel = -77;
  std::vector<float> rgba(16, 0.f), m2(4, 0.f), noise(4, 0.f);
  std::vector<uint32_t> seed(4, 0u);
  std::vector<int32_t> cnt(4, 0);
  const rtp_render_state st{rgba.data(), seed.data(), nullptr, m2.data()};
  EXPECT(rtp_refine(nullptr, &cam, 2, 2, 8, &st, cnt.data(), &prm, &sel, nullptr) == RTP_ERR_INVALID_ARGUMENT);
  EXPECT(rtp_noise(nullptr, rgba.data(), m2.data(), cnt.data(), 4, noise.data(), nullptr) == RTP_ERR_INVALID_ARGUMENT);
  EXPECT(sel == -77);
}

int main() {
  host_helpers();
  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
