// Launchers of the region (DMR) kernels (dmr_kernels.hip), used by the C ABI
// in capi.cpp. Not part of the public ABI.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace hyg {

constexpr int kDmrMaxTrajectories = 16384;  // region_counts: s_p [P] int32 in LDS (64 KiB)
constexpr int kDmrMaxStride = 4096;         // region_sums: one int64 per column in LDS (32 KiB)

// scratch of dmr_scan_u64 for an array of m entries (bytes)
size_t dmr_scan_temp_bytes(int64_t m);
// blocks of the site pass / of the region pass (one entry of block sums each)
int64_t dmr_blocks(int64_t n);

// Pass 1 over the sites: block sums of (starts << 32 | ends), scanned in place
// (exclusive); *total (device) = (number of runs << 32 | number of runs).
int launch_dmr_site_sums(const int32_t* counts, int stride, int col, int64_t n_sites, int min_count,
                         const int64_t* positions, int64_t max_gap, uint64_t* block_sums, void* scan_temp,
                         uint64_t* total, void* stream);
// Pass 2: run r's begin -> runs[2r], end -> runs[2r + 1] (ascending).
int launch_dmr_site_emit(const int32_t* counts, int stride, int col, int64_t n_sites, int min_count,
                         const int64_t* positions, int64_t max_gap, const uint64_t* block_sums, int64_t* runs,
                         void* stream);
// Second compaction: the runs of at least min_sites sites, in order.
int launch_dmr_run_sums(const int64_t* runs, int64_t n_runs, int64_t min_sites, uint64_t* block_sums,
                        void* scan_temp, uint64_t* total, void* stream);
int launch_dmr_run_emit(const int64_t* runs, int64_t n_runs, int64_t min_sites, const uint64_t* block_sums,
                        int64_t* regions, void* stream);

// desc (device, int64): group begins [n_groups], group ends [n_groups], block rows [n_groups][n_seeds]
int launch_dmr_region_counts(const int16_t* control, const int16_t* kase, int B, const int64_t* desc, int n_groups,
                             int n_seeds, int64_t n_sites, const int64_t* regions, int64_t n_regions, int frac_num,
                             int frac_den, int32_t* region_counts, void* stream);
int launch_dmr_region_sums(const int32_t* counts, int stride, int64_t n_sites, const int64_t* regions,
                           int64_t n_regions, int64_t* sums, void* stream);

}  // namespace hyg
