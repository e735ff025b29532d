// Layout of the transition statistics and the launcher of their kernel
// (em_kernels.hip), used by the C ABI in capi.cpp. Not part of the public ABI.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace hyg {

constexpr int kEmTile = 256;     // sites of one transition_stats workgroup
constexpr int kEmMaxDcap = 4096; // 2 * (dcap + 1) int32 bins in LDS: 32 KiB at the cap
constexpr int kEmTable = 4;      // stats[2 * m(x) + m(y)]: the merged trials' 2 x 2 table

// stats (int64): table [4], trials [dcap + 1], events [dcap + 1]
constexpr size_t em_stats_len(int dcap) { return (size_t)kEmTable + 2 * ((size_t)dcap + 1); }

// desc (device, int64) as launch_cp_site_events: group begins [n_groups], group ends [n_groups],
// block rows [n_groups][n_seeds]. Adds into stats (device, [em_stats_len(dcap)]).
int launch_em_transition_stats(const int16_t* merged, const int16_t* control, const int16_t* kase, int B,
                               const int64_t* desc, int n_groups, int n_seeds, int64_t n_sites, int minimum_duration,
                               int dcap, int64_t* stats, void* stream);

}  // namespace hyg
