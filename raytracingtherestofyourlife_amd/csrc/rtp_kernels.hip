// rtp_kernels.hip -- the translation unit of the path-tracing kernels (one
// code object):
//   rtp_trace.hpp   the per-ray device code (tests, BVH walks, bounce);
//   rtp_pool.hpp    the two render kernels (v1 lockstep, v2 the persistent-wave
//                   pool and its scheduling loop) and their tunables;
//   rtp_diag.hpp    the diagnostic and utility kernels;
//   rtp_launch.hpp  the host side: the table of render-kernel instances, the
//                   occupancy planning and the launchers (extern "C", called
//                   by rtp_host.cpp).
#include <hip/hip_runtime.h>

#include "rtp_trace.hpp"
#include "rtp_pool.hpp"
#include "rtp_diag.hpp"
#include "rtp_launch.hpp"
