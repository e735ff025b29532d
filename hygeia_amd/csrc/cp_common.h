// Launchers of the change-point kernels (cp_kernels.hip), used by the C ABI
// in capi.cpp. Not part of the public ABI.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace hyg {

constexpr int kCpMaxTrajectories = 16384;  // window_counts: s_p [P] int32 in LDS (64 KiB)
constexpr int kCpKinds = 5;                // control, case, any, split, merge: the event matrix's columns

// desc (device, int64): group begins [n_groups], group ends [n_groups], block rows [n_groups][n_seeds]
// merged may be null in launch_cp_site_events (columns 3, 4 = 0) and for kinds 0-2 of launch_cp_window_counts.
int launch_cp_site_events(const int16_t* merged, const int16_t* control, const int16_t* kase, int B,
                          const int64_t* desc, int n_groups, int n_seeds, int64_t n_sites, int32_t* events,
                          void* stream);
int launch_cp_window_counts(const int16_t* merged, const int16_t* control, const int16_t* kase, int B,
                            const int64_t* desc, int n_groups, int n_seeds, int64_t n_sites, int kind,
                            const int64_t* windows, int64_t n_windows, int32_t* counts, void* stream);
int launch_cp_window_intervals(const int32_t* events, int stride, int column, int64_t n_sites, const int64_t* windows,
                               int64_t n_windows, int level_num, int level_den, int64_t* out, void* stream);

}  // namespace hyg
