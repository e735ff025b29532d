// dmr_kernels.hip -- differentially methylated regions from the joint
// trajectories that stay resident in HBM after hyg_tg_run_chains (the region
// caller has no counterpart in the reference pipeline).
//
//   dmr_site_*_kernel      candidate regions: maximal runs of linked seed sites.
//                          Each site computes its start and end flag; the i-th
//                          start pairs with the i-th end, so one exclusive scan
//                          of (starts << 32 | ends) numbers both.
//   dmr_run_*_kernel       second compaction: the runs of >= min_sites sites
//   scan_*_kernel          exclusive scan of u64 in separate launches: tile
//                          sums, a scan of the sums (recursing while they
//                          exceed one tile), apply. No workgroup waits for
//                          another, no atomics: the order is the site order.
//   dmr_region_counts_kernel  per region, s_p = #(r_ctrl != r_case) over the
//                          region's sites for each of the P trajectories, then
//                          #(s_p == n) and #(s_p den >= num n)
//   dmr_region_sums_kernel segmented column sums of an int32 matrix (int64)
//
// Everything here is integer arithmetic, so the results are exact and do not
// depend on the order of the adds.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dmr_common.h"

namespace hyg {

constexpr int kDmrTile = 256;  // one entry per thread

// Exclusive scan of one value per thread over the workgroup (Hillis-Steele in
// LDS); *total = the workgroup's sum. sh may be reused on return.
__device__ __forceinline__ uint64_t tile_excl_u64(uint64_t v, uint64_t* sh, uint64_t* total) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int off = 1; off < kDmrTile; off <<= 1) {
    const uint64_t x = (tid >= off) ? sh[tid - off] : 0ull;
    __syncthreads();
    sh[tid] += x;
    __syncthreads();
  }
  const uint64_t inc = sh[tid];
  *total = sh[kDmrTile - 1];
  __syncthreads();
  return inc - v;
}

// ------------------------------------------------------------------ scan
__global__ void __launch_bounds__(kDmrTile)
scan_reduce_kernel(const uint64_t* __restrict__ a, int64_t m, uint64_t* __restrict__ sums) {
  __shared__ uint64_t sh[kDmrTile];
  const int64_t i = (int64_t)blockIdx.x * kDmrTile + threadIdx.x;
  uint64_t tot;
  (void)tile_excl_u64(i < m ? a[i] : 0ull, sh, &tot);
  if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// m <= kDmrTile entries in place; *total (when given) = their sum
__global__ void __launch_bounds__(kDmrTile) scan_block_kernel(uint64_t* __restrict__ a, int64_t m, uint64_t* total) {
  __shared__ uint64_t sh[kDmrTile];
  const int i = threadIdx.x;
  uint64_t tot;
  const uint64_t e = tile_excl_u64(i < m ? a[i] : 0ull, sh, &tot);
  if (i < m) a[i] = e;
  if (i == 0 && total) *total = tot;
}

// a[i] = exclusive prefix inside its tile + the tile's scanned sum
__global__ void __launch_bounds__(kDmrTile)
scan_apply_kernel(uint64_t* __restrict__ a, int64_t m, const uint64_t* __restrict__ sums) {
  __shared__ uint64_t sh[kDmrTile];
  const int64_t i = (int64_t)blockIdx.x * kDmrTile + threadIdx.x;
  uint64_t tot;
  const uint64_t e = tile_excl_u64(i < m ? a[i] : 0ull, sh, &tot);
  if (i < m) a[i] = e + sums[blockIdx.x];
}

int64_t dmr_blocks(int64_t n) { return (n + kDmrTile - 1) / kDmrTile; }

size_t dmr_scan_temp_bytes(int64_t m) {
  size_t b = 0;
  while (m > kDmrTile) {
    m = dmr_blocks(m);
    b += sizeof(uint64_t) * (size_t)m;
  }
  return b;
}

// Exclusive scan of a[0, m) in place; *total (device) = the sum.
static void dmr_scan_u64(uint64_t* a, int64_t m, uint64_t* temp, uint64_t* total, hipStream_t s) {
  if (m <= kDmrTile) {
    hipLaunchKernelGGL(scan_block_kernel, dim3(1), dim3(kDmrTile), 0, s, a, m, total);
    return;
  }
  const int64_t nb = dmr_blocks(m);
  hipLaunchKernelGGL(scan_reduce_kernel, dim3((unsigned)nb), dim3(kDmrTile), 0, s, a, m, temp);
  dmr_scan_u64(temp, nb, temp + nb, total, s);
  hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)nb), dim3(kDmrTile), 0, s, a, m, temp);
}

// ------------------------------------------------------- region finding
struct SiteArgs {
  const int32_t* __restrict__ counts;
  const int64_t* __restrict__ positions;
  int64_t n_sites, max_gap;
  int stride, col, min_count;
};

// (start << 32 | end) of site t: a seed site starts a run unless it is linked
// to a seed predecessor, and ends one unless linked to a seed successor. A link
// needs 0 < pos[t + 1] - pos[t] <= max_gap.
__device__ __forceinline__ uint64_t site_flags(const SiteArgs& A, int64_t t) {
  if (t >= A.n_sites) return 0ull;
  if (A.counts[t * A.stride + A.col] < A.min_count) return 0ull;
  const int64_t p = A.positions[t];
  bool lp = false, ln = false;
  if (t > 0 && A.counts[(t - 1) * A.stride + A.col] >= A.min_count) {
    const int64_t q = A.positions[t - 1];
    lp = p > q && p - q <= A.max_gap;
  }
  if (t + 1 < A.n_sites && A.counts[(t + 1) * A.stride + A.col] >= A.min_count) {
    const int64_t q = A.positions[t + 1];
    ln = q > p && q - p <= A.max_gap;
  }
  return ((uint64_t)(lp ? 0 : 1) << 32) | (uint64_t)(ln ? 0 : 1);
}

__global__ void __launch_bounds__(kDmrTile) dmr_site_sums_kernel(SiteArgs A, uint64_t* __restrict__ block_sums) {
  __shared__ uint64_t sh[kDmrTile];
  const int64_t t = (int64_t)blockIdx.x * kDmrTile + threadIdx.x;
  uint64_t tot;
  (void)tile_excl_u64(site_flags(A, t), sh, &tot);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(kDmrTile)
dmr_site_emit_kernel(SiteArgs A, const uint64_t* __restrict__ block_sums, int64_t* __restrict__ runs) {
  __shared__ uint64_t sh[kDmrTile];
  const int64_t t = (int64_t)blockIdx.x * kDmrTile + threadIdx.x;
  const uint64_t f = site_flags(A, t);
  uint64_t tot;
  const uint64_t e = tile_excl_u64(f, sh, &tot) + block_sums[blockIdx.x];
  if (f >> 32) runs[2 * (int64_t)(e >> 32)] = t;
  if (f & 1ull) runs[2 * (int64_t)(e & 0xffffffffull) + 1] = t + 1;
}

__device__ __forceinline__ uint64_t run_keep(const int64_t* __restrict__ runs, int64_t n_runs, int64_t min_sites,
                                             int64_t i) {
  return (i < n_runs && runs[2 * i + 1] - runs[2 * i] >= min_sites) ? 1ull : 0ull;
}

__global__ void __launch_bounds__(kDmrTile)
dmr_run_sums_kernel(const int64_t* __restrict__ runs, int64_t n_runs, int64_t min_sites,
                    uint64_t* __restrict__ block_sums) {
  __shared__ uint64_t sh[kDmrTile];
  const int64_t i = (int64_t)blockIdx.x * kDmrTile + threadIdx.x;
  uint64_t tot;
  (void)tile_excl_u64(run_keep(runs, n_runs, min_sites, i), sh, &tot);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(kDmrTile)
dmr_run_emit_kernel(const int64_t* __restrict__ runs, int64_t n_runs, int64_t min_sites,
                    const uint64_t* __restrict__ block_sums, int64_t* __restrict__ regions) {
  __shared__ uint64_t sh[kDmrTile];
  const int64_t i = (int64_t)blockIdx.x * kDmrTile + threadIdx.x;
  const uint64_t k = run_keep(runs, n_runs, min_sites, i);
  uint64_t tot;
  const int64_t e = (int64_t)(tile_excl_u64(k, sh, &tot) + block_sums[blockIdx.x]);
  if (k) {
    regions[2 * e] = runs[2 * i];
    regions[2 * e + 1] = runs[2 * i + 1];
  }
}

// ------------------------------------------------------- region counts
// One workgroup per region [a, b). Trajectory p = seed block * B + b is column
// p of the region's [n][P] indicator matrix. With P <= 256 the workgroup's
// first G P threads (G = 256 / P) are G rows of P lanes: lane p of row j walks
// the sites a + j, a + j + G, ... of trajectory p, so consecutive lanes load
// consecutive (d, r) pairs of a trajectory row (contiguous within a seed
// block's B pairs) and a thread keeps one partial s_p in a register. With
// P > 256 a thread walks every site for the trajectories tid, tid + 256, ...
// The partials of the threads that share a trajectory meet in LDS integer adds.
// Groups are sorted and disjoint, so a thread moves through them forwards; a
// site inside no group adds nothing and is not read.
__global__ void __launch_bounds__(256)
dmr_region_counts_kernel(const uint32_t* __restrict__ control, const uint32_t* __restrict__ kase, int B,
                         const int64_t* __restrict__ gbeg, const int64_t* __restrict__ gend,
                         const int64_t* __restrict__ blk, int n_groups, int n_seeds, int64_t n_sites,
                         const int64_t* __restrict__ regions, int frac_num, int frac_den,
                         int32_t* __restrict__ out) {
  extern __shared__ int32_t sp[];  // [P]
  __shared__ int32_t cnt[2];
  const int tid = threadIdx.x;
  const int P = B * n_seeds;
  int64_t a = regions[2 * (int64_t)blockIdx.x], b = regions[2 * (int64_t)blockIdx.x + 1];
  a = a < 0 ? 0 : a;
  b = b > n_sites ? n_sites : b;
  const int64_t n = b > a ? b - a : 0;
  for (int p = tid; p < P; p += 256) sp[p] = 0;
  if (tid < 2) cnt[tid] = 0;
  __syncthreads();
  const int G = (P <= 256) ? 256 / P : 1;
  const int active = (P <= 256) ? G * P : 256;
  const int pstep = (P <= 256) ? P : 256;
  if (tid < active && n > 0 && n_groups > 0) {
    const int j = (P <= 256) ? tid / P : 0;
    int lo = 0, hi = n_groups;  // first group that ends behind a
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (gend[mid] > a) hi = mid; else lo = mid + 1;
    }
    const int g0 = lo;
    for (int p = tid - j * P; p < P; p += pstep) {
      const int s = p / B, bb = p - s * B;
      int g = g0, acc = 0;
      int64_t t = a + j;
      while (t < b) {
        while (g < n_groups && t >= gend[g]) ++g;
        if (g >= n_groups) break;
        const int64_t gb = gbeg[g];
        if (t < gb) {  // sites inside no group: on to this thread's first site of the group
          t += (gb - t + G - 1) / G * G;
          continue;
        }
        const int64_t stop = gend[g] < b ? gend[g] : b;
        // the group's rows of this seed block are consecutive: a fixed stride from site to site
        const int64_t i0 = (blk[(int64_t)g * n_seeds + s] + (t - gb)) * B + bb, di = (int64_t)G * B;
        const uint32_t* __restrict__ pc = control + i0;
        const uint32_t* __restrict__ pk = kase + i0;
        // (d, r) int16 pairs: r is the high half. Four sites' loads are issued before the first use.
        for (; t + 3 * (int64_t)G < stop; t += 4 * (int64_t)G, pc += 4 * di, pk += 4 * di) {
          const uint32_t c0 = pc[0], c1 = pc[di], c2 = pc[2 * di], c3 = pc[3 * di];
          const uint32_t k0 = pk[0], k1 = pk[di], k2 = pk[2 * di], k3 = pk[3 * di];
          acc += (((c0 ^ k0) >> 16) ? 1 : 0) + (((c1 ^ k1) >> 16) ? 1 : 0) + (((c2 ^ k2) >> 16) ? 1 : 0) +
                 (((c3 ^ k3) >> 16) ? 1 : 0);
        }
        for (; t < stop; t += G, pc += di, pk += di) acc += ((*pc ^ *pk) >> 16) ? 1 : 0;
      }
      if (acc) atomicAdd(&sp[p], acc);
    }
  }
  __syncthreads();
  int n_all = 0, n_frac = 0;
  const int64_t need = (int64_t)frac_num * n;
  for (int p = tid; p < P; p += 256) {
    const int64_t v = sp[p];
    n_all += (v == n) ? 1 : 0;
    n_frac += (v * frac_den >= need) ? 1 : 0;
  }
  if (n_all) atomicAdd(&cnt[0], n_all);
  if (n_frac) atomicAdd(&cnt[1], n_frac);
  __syncthreads();
  if (tid < 2) out[2 * (int64_t)blockIdx.x + tid] = cnt[tid];
}

// --------------------------------------------------------- region sums
// One workgroup per region: the region's rows are one contiguous range of the
// matrix. With stride <= 256 the first G stride threads are G rows of `stride`
// lanes, each lane one column; wider matrices go tid, tid + 256, ...
__global__ void __launch_bounds__(256)
dmr_region_sums_kernel(const int32_t* __restrict__ counts, int stride, int64_t n_sites,
                       const int64_t* __restrict__ regions, int64_t* __restrict__ sums) {
  extern __shared__ unsigned long long cs[];  // [stride]
  const int tid = threadIdx.x;
  int64_t a = regions[2 * (int64_t)blockIdx.x], b = regions[2 * (int64_t)blockIdx.x + 1];
  a = a < 0 ? 0 : a;
  b = b > n_sites ? n_sites : b;
  for (int c = tid; c < stride; c += 256) cs[c] = 0ull;
  __syncthreads();
  const int G = (stride <= 256) ? 256 / stride : 1;
  const int active = (stride <= 256) ? G * stride : 256;
  const int cstep = (stride <= 256) ? stride : 256;
  if (tid < active) {
    const int j = (stride <= 256) ? tid / stride : 0;
    for (int c = tid - j * stride; c < stride; c += cstep) {
      int64_t acc = 0;
      for (int64_t t = a + j; t < b; t += G) acc += counts[t * stride + c];
      if (acc) atomicAdd(&cs[c], (unsigned long long)acc);
    }
  }
  __syncthreads();
  for (int c = tid; c < stride; c += 256) sums[(int64_t)blockIdx.x * stride + c] = (int64_t)cs[c];
}

// ---------------------------------------------------------------- launchers
static SiteArgs site_args(const int32_t* counts, int stride, int col, int64_t n_sites, int min_count,
                          const int64_t* positions, int64_t max_gap) {
  SiteArgs A;
  A.counts = counts;
  A.positions = positions;
  A.n_sites = n_sites;
  A.max_gap = max_gap;
  A.stride = stride;
  A.col = col;
  A.min_count = min_count;
  return A;
}

int launch_dmr_site_sums(const int32_t* counts, int stride, int col, int64_t n_sites, int min_count,
                         const int64_t* positions, int64_t max_gap, uint64_t* block_sums, void* scan_temp,
                         uint64_t* total, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int64_t nb = dmr_blocks(n_sites);
  hipLaunchKernelGGL(dmr_site_sums_kernel, dim3((unsigned)nb), dim3(kDmrTile), 0, s,
                     site_args(counts, stride, col, n_sites, min_count, positions, max_gap), block_sums);
  dmr_scan_u64(block_sums, nb, (uint64_t*)scan_temp, total, s);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_dmr_site_emit(const int32_t* counts, int stride, int col, int64_t n_sites, int min_count,
                         const int64_t* positions, int64_t max_gap, const uint64_t* block_sums, int64_t* runs,
                         void* stream) {
  hipLaunchKernelGGL(dmr_site_emit_kernel, dim3((unsigned)dmr_blocks(n_sites)), dim3(kDmrTile), 0,
                     (hipStream_t)stream, site_args(counts, stride, col, n_sites, min_count, positions, max_gap),
                     block_sums, runs);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_dmr_run_sums(const int64_t* runs, int64_t n_runs, int64_t min_sites, uint64_t* block_sums,
                        void* scan_temp, uint64_t* total, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int64_t nb = dmr_blocks(n_runs);
  hipLaunchKernelGGL(dmr_run_sums_kernel, dim3((unsigned)nb), dim3(kDmrTile), 0, s, runs, n_runs, min_sites,
                     block_sums);
  dmr_scan_u64(block_sums, nb, (uint64_t*)scan_temp, total, s);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_dmr_run_emit(const int64_t* runs, int64_t n_runs, int64_t min_sites, const uint64_t* block_sums,
                        int64_t* regions, void* stream) {
  hipLaunchKernelGGL(dmr_run_emit_kernel, dim3((unsigned)dmr_blocks(n_runs)), dim3(kDmrTile), 0,
                     (hipStream_t)stream, runs, n_runs, min_sites, block_sums, regions);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_dmr_region_counts(const int16_t* control, const int16_t* kase, int B, const int64_t* desc, int n_groups,
                             int n_seeds, int64_t n_sites, const int64_t* regions, int64_t n_regions, int frac_num,
                             int frac_den, int32_t* region_counts, void* stream) {
  if (n_regions <= 0) return 0;
  const size_t lds = sizeof(int32_t) * (size_t)B * (size_t)n_seeds;
  // the trajectory arrays are [rows][B][2] int16: one 32-bit word per (d, r) pair
  hipLaunchKernelGGL(dmr_region_counts_kernel, dim3((unsigned)n_regions), dim3(256), lds, (hipStream_t)stream,
                     (const uint32_t*)control, (const uint32_t*)kase, B, desc, desc + n_groups, desc + 2 * n_groups,
                     n_groups, n_seeds, n_sites, regions, frac_num, frac_den, region_counts);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_dmr_region_sums(const int32_t* counts, int stride, int64_t n_sites, const int64_t* regions,
                           int64_t n_regions, int64_t* sums, void* stream) {
  if (n_regions <= 0) return 0;
  hipLaunchKernelGGL(dmr_region_sums_kernel, dim3((unsigned)n_regions), dim3(256),
                     sizeof(unsigned long long) * (size_t)stride, (hipStream_t)stream, counts, stride, n_sites,
                     regions, sums);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace hyg
