// rtp_ff.hpp -- the RNG jump tables (rtp_ff_host.cpp) as the launches of
// rtp_host.cpp and rtp_eval_primitive (rtp_debug_host.cpp) see them.  Internal.
#pragma once
#include <cstdint>

#include "rtp_layout.hpp"

// (internal to librtp.so: these names are no part of what the library exports)
#pragma GCC visibility push(hidden)
namespace rtp_host {

// What one launch reads of a device's tables: a copy taken under the tables'
// lock, so a later stage being built by another thread cannot change it.
struct FfSnap {
  const uint32_t* t[rtp::kFfTables] = {};
  const uint32_t* direct = nullptr;
  int d_first = 0, d_count = 0;
};

// The tables a launch of `samples` samples on `device` uses under `policy`
// (built first when the policy says so).  The tables, once published, stay
// until the process ends.
FfSnap ff_tables(int device, int policy, uint64_t samples);

// the policy a new context starts with (RTP_FF_POLICY)
int ff_policy_default();

}  // namespace rtp_host
#pragma GCC visibility pop
