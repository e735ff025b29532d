// em_kernels.hip -- sufficient statistics of the transition law's three
// settings (omega_case, merge_log_prob, split_prob) from the joint trajectories
// that stay resident in HBM after hyg_tg_run_chains (no counterpart in the
// reference pipeline). The definitions are in include/hygeia_amd.h,
// "transition statistics".
//
//   em_transition_stats_kernel  over every (site t that is not its group's
//                               first row, trajectory p), x = row t - 1 and
//                               y = row t of the same seed block: the 2 x 2
//                               table of the merged trials and the trials /
//                               events histograms of the case hazard by d_k(x)
//
// Everything here is integer arithmetic, so the results are exact and do not
// depend on the order of the adds.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "em_common.h"

namespace hyg {

// First group that ends behind site t (groups sorted and disjoint).
__device__ __forceinline__ int em_first_group(const int64_t* __restrict__ gend, int n_groups, int64_t t) {
  int lo = 0, hi = n_groups;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (gend[mid] > t) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// One workgroup per tile of kEmTile consecutive sites, with
// cp_site_events_kernel's addressing: inside a group the rows of a seed block
// are consecutive, so the tile's part of a (group, seed block) is one
// contiguous range of rows x B words; thread i takes words i, i + 256, ... of
// it, and the word of the row before lies B words back in the same range. No
// statistic is kept per site, so a word's row is never needed: there is no
// (row, column) pair to step and no division. The six loads of a word (y and x
// of merged, control and case) are issued before the first use.
//
// The histograms are LDS integer bins: bins [0, dcap) take LDS adds; the four
// table cells and the pooled last bin (d_k(x) >= dcap), which most lanes of a
// wave would hit at once, are counted in registers and meet the LDS bins after
// the loop. After the tile's last barrier the nonzero bins are flushed once,
// as 64-bit integer adds to stats.
__global__ void __launch_bounds__(256)
em_transition_stats_kernel(const int16_t* __restrict__ merged, const uint32_t* __restrict__ control,
                           const uint32_t* __restrict__ kase, int B, const int64_t* __restrict__ gbeg,
                           const int64_t* __restrict__ gend, const int64_t* __restrict__ blk, int n_groups, int n_seeds,
                           int64_t n_sites, uint32_t minimum_duration, uint32_t dcap,
                           unsigned long long* __restrict__ stats) {
  extern __shared__ int32_t bins[];  // table [4], trials [dcap + 1], events [dcap + 1]
  const int tid = threadIdx.x;
  const int n_bins = kEmTable + 2 * ((int)dcap + 1);
  int32_t* __restrict__ trials = bins + kEmTable;
  int32_t* __restrict__ events = trials + dcap + 1;
  const int64_t t0 = (int64_t)blockIdx.x * kEmTile;
  const int64_t t1 = t0 + kEmTile < n_sites ? t0 + kEmTile : n_sites;
  for (int i = tid; i < n_bins; i += 256) bins[i] = 0;
  __syncthreads();
  int32_t n00 = 0, n01 = 0, n10 = 0, n11 = 0, t_cap = 0, e_cap = 0;
  for (int g = em_first_group(gend, n_groups, t0); g < n_groups && gbeg[g] < t1; ++g) {
    const int64_t gb = gbeg[g];
    const int64_t u0 = gb > t0 ? gb : t0, u1 = gend[g] < t1 ? gend[g] : t1;
    const int64_t e0 = u0 == gb ? u0 + 1 : u0;  // the first row that has a predecessor
    if (e0 >= u1) continue;
    const int n = (int)(u1 - e0) * B;  // <= 256 * 16384 words
    for (int s = 0; s < n_seeds; ++s) {
      const int64_t w0 = (blk[(int64_t)g * n_seeds + s] + (e0 - gb)) * B;
      const uint32_t* __restrict__ pc = control + w0;
      const uint32_t* __restrict__ pk = kase + w0;
      const int16_t* __restrict__ pm = merged + w0;
      for (int i = tid; i < n; i += 256) {
        const uint32_t c = pc[i], cb = pc[i - B], k = pk[i], kb = pk[i - B];
        const bool my = pm[i] != 0, mx = pm[i - B] != 0;
        // packed (d, r) words, d the low half: durations as uint16 of the stored word
        const uint32_t dcx = cb & 0xffffu, dkx = kb & 0xffffu;
        if ((dcx < dkx ? dcx : dkx) >= minimum_duration) {  // merged trial
          n00 += (!mx && !my) ? 1 : 0;
          n01 += (!mx && my) ? 1 : 0;
          n10 += (mx && !my) ? 1 : 0;
          n11 += (mx && my) ? 1 : 0;
        }
        // case-hazard trial: the fourth branch of the case transition
        const bool forced_split = mx && (c & 0xffffu) != 1u;      // branch 2
        const bool onto_case = !mx && (c >> 16) == (kb >> 16);    // branch 3
        if (!my && !forced_split && !onto_case) {
          const bool ev = (k & 0xffffu) == 1u;
          if (dkx >= dcap) {
            t_cap += 1;
            e_cap += ev ? 1 : 0;
          } else {
            atomicAdd(trials + dkx, 1);
            if (ev) atomicAdd(events + dkx, 1);
          }
        }
      }
    }
  }
  if (n00) atomicAdd(bins + 0, n00);
  if (n01) atomicAdd(bins + 1, n01);
  if (n10) atomicAdd(bins + 2, n10);
  if (n11) atomicAdd(bins + 3, n11);
  if (t_cap) atomicAdd(trials + dcap, t_cap);
  if (e_cap) atomicAdd(events + dcap, e_cap);
  __syncthreads();
  for (int i = tid; i < n_bins; i += 256) {
    const int32_t v = bins[i];
    if (v) atomicAdd(stats + i, (unsigned long long)v);
  }
}

// ---------------------------------------------------------------- launcher
int launch_em_transition_stats(const int16_t* merged, const int16_t* control, const int16_t* kase, int B,
                               const int64_t* desc, int n_groups, int n_seeds, int64_t n_sites, int minimum_duration,
                               int dcap, int64_t* stats, void* stream) {
  if (n_sites <= 0 || n_groups <= 0) return 0;
  const int64_t nb = (n_sites + kEmTile - 1) / kEmTile;
  const size_t lds = sizeof(int32_t) * em_stats_len(dcap);
  // the trajectory arrays are [rows][B][2] int16: one 32-bit word per (d, r) pair
  hipLaunchKernelGGL(em_transition_stats_kernel, dim3((unsigned)nb), dim3(256), lds, (hipStream_t)stream, merged,
                     (const uint32_t*)control, (const uint32_t*)kase, B, desc, desc + n_groups, desc + 2 * n_groups,
                     n_groups, n_seeds, n_sites, (uint32_t)minimum_duration, (uint32_t)dcap,
                     (unsigned long long*)stats);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace hyg
