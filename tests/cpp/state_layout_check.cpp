// Prints the layout of rtp_render_state (include/rtp.h) for the ctypes mirror
// check of tests/test_progressive_api.py: size, then the offsets of rgba,
// seed, live_bounces, m2.  Header only: links nothing.
#include <cstddef>
#include <cstdio>

#include "rtp.h"

int main() {
  std::printf("%zu %zu %zu %zu %zu\n", sizeof(rtp_render_state), offsetof(rtp_render_state, rgba),
              offsetof(rtp_render_state, seed), offsetof(rtp_render_state, live_bounces),
              offsetof(rtp_render_state, m2));
  return 0;
}
