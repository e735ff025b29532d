// cp_kernels.hip -- change points from the joint trajectories that stay
// resident in HBM after hyg_tg_run_chains (no counterpart in the reference
// pipeline). The definitions are in include/hygeia_amd.h, "change points".
//
//   cp_site_events_kernel       c_t of the five event kinds for every site: an
//                               event compares row t of a trajectory with row
//                               t - 1 of the same seed block
//   cp_window_counts_kernel     per window, s_p = #events of trajectory p over
//                               the window's sites, then #(s_p >= 1), #(s_p == 1)
//   cp_window_intervals_kernel  per window, from one column of the event matrix:
//                               the number of events, the modal site and the
//                               central interval of the events' locations
//
// Everything here is integer arithmetic, so the results are exact and do not
// depend on the order of the adds.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cp_common.h"

namespace hyg {

constexpr int kCpTile = 64;  // sites of one site_events workgroup

// The packed (d, r) word (d the low half) that continues the word w of the row
// before: the same regime, the duration one more modulo 2^16.
__device__ __forceinline__ uint32_t cp_next(uint32_t w) { return (w & 0xffff0000u) | ((w + 1u) & 0xffffu); }

// First group that ends behind site t (groups sorted and disjoint).
__device__ __forceinline__ int cp_first_group(const int64_t* __restrict__ gend, int n_groups, int64_t t) {
  int lo = 0, hi = n_groups;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (gend[mid] > t) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// ---------------------------------------------------------- site events
// One workgroup per tile of kCpTile consecutive sites. Inside a group the rows
// of a seed block are consecutive, so the tile's part of a (group, seed block)
// is one contiguous range of rows x B words: thread i takes words i, i + 256,
// ... of it, and the word of the row before lies B words back in the same
// range (it is the word another lane of the workgroup reads as its own). The
// five counts of a site are LDS integer adds, issued only where an event is.
// A group's first row has no predecessor: it is covered (written as zeros) but
// not compared. A site inside no group is neither read nor written.
__global__ void __launch_bounds__(256)
cp_site_events_kernel(const int16_t* __restrict__ merged, const uint32_t* __restrict__ control,
                      const uint32_t* __restrict__ kase, int B, const int64_t* __restrict__ gbeg,
                      const int64_t* __restrict__ gend, const int64_t* __restrict__ blk, int n_groups, int n_seeds,
                      int64_t n_sites, int32_t* __restrict__ events) {
  __shared__ int32_t ev[kCpTile * kCpKinds];
  __shared__ int32_t covered[kCpTile];
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * kCpTile;
  const int64_t t1 = t0 + kCpTile < n_sites ? t0 + kCpTile : n_sites;
  for (int i = tid; i < kCpTile * kCpKinds; i += 256) ev[i] = 0;
  if (tid < kCpTile) covered[tid] = 0;
  __syncthreads();
  const int row0 = tid / B, col0 = tid - row0 * B;  // of word tid in a range of rows x B words
  const int drow = 256 / B, dcol = 256 - drow * B;  // and the step of 256 words
  for (int g = cp_first_group(gend, n_groups, t0); g < n_groups && gbeg[g] < t1; ++g) {
    const int64_t gb = gbeg[g];
    const int64_t u0 = gb > t0 ? gb : t0, u1 = gend[g] < t1 ? gend[g] : t1;
    if (u0 >= u1) continue;
    for (int i = tid; i < (int)(u1 - u0); i += 256) covered[(int)(u0 - t0) + i] = 1;
    const int64_t e0 = u0 == gb ? u0 + 1 : u0;  // the first row that has a predecessor
    const int n = (int)(u1 - e0) * B;           // <= 64 * 16384 words
    const int base = (int)(e0 - t0);
    for (int s = 0; s < n_seeds; ++s) {
      const int64_t w0 = (blk[(int64_t)g * n_seeds + s] + (e0 - gb)) * B;
      const uint32_t* __restrict__ pc = control + w0;
      const uint32_t* __restrict__ pk = kase + w0;
      const int16_t* __restrict__ pm = merged ? merged + w0 : nullptr;
      int row = row0, col = col0;
      for (int i = tid; i < n; i += 256) {
        const uint32_t c = pc[i], cb = pc[i - B], k = pk[i], kb = pk[i - B];
        const bool fc = c != cp_next(cb), fk = k != cp_next(kb);
        bool fs = false, fm = false;
        if (pm) {
          const int16_t m = pm[i], mb = pm[i - B];
          fs = mb != 0 && m == 0;
          fm = mb == 0 && m != 0;
        }
        if (fc || fk || fs || fm) {
          int32_t* e = ev + (base + row) * kCpKinds;
          if (fc) atomicAdd(e + 0, 1);
          if (fk) atomicAdd(e + 1, 1);
          if (fc || fk) atomicAdd(e + 2, 1);
          if (fs) atomicAdd(e + 3, 1);
          if (fm) atomicAdd(e + 4, 1);
        }
        row += drow;
        col += dcol;
        if (col >= B) {
          col -= B;
          ++row;
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < (int)(t1 - t0) * kCpKinds; i += 256)
    if (covered[i / kCpKinds]) events[t0 * kCpKinds + i] = ev[i];
}

// -------------------------------------------------------- window counts
// Event of kind KIND at word i of a trajectory row (the row before is B words
// back). Kinds 0 to 2 read control / kase only, kinds 3 and 4 merged only.
template <int KIND>
__device__ __forceinline__ int cp_event(const int16_t* __restrict__ m, const uint32_t* __restrict__ c,
                                        const uint32_t* __restrict__ k, int64_t i, int B) {
  if (KIND >= 3) {
    const int16_t mb = m[i - B], mt = m[i];
    return KIND == 3 ? (mb != 0 && mt == 0) : (mb == 0 && mt != 0);
  }
  bool e = false;
  if (KIND != 1) e |= c[i] != cp_next(c[i - B]);
  if (KIND != 0) e |= k[i] != cp_next(k[i - B]);
  return e ? 1 : 0;
}

// One workgroup per window [a, b), with dmr_region_counts_kernel's lane
// layout: with P <= 256 the first G P threads (G = 256 / P) are G rows of P
// lanes, lane p of row j walks the sites a + j, a + j + G, ... of trajectory
// p; with P > 256 a thread walks every site for the trajectories tid, tid +
// 256, ... The row before a site's row is the row the lane row above reads as
// its own. The partials of a trajectory meet in LDS integer adds. Groups are
// sorted and disjoint, so a thread moves through them forwards; a site inside
// no group and a group's first row add nothing and are not read.
template <int KIND>
__global__ void __launch_bounds__(256)
cp_window_counts_kernel(const int16_t* __restrict__ merged, const uint32_t* __restrict__ control,
                        const uint32_t* __restrict__ kase, int B, const int64_t* __restrict__ gbeg,
                        const int64_t* __restrict__ gend, const int64_t* __restrict__ blk, int n_groups, int n_seeds,
                        int64_t n_sites, const int64_t* __restrict__ windows, int32_t* __restrict__ out) {
  extern __shared__ int32_t sp[];  // [P]
  __shared__ int32_t cnt[2];
  const int tid = threadIdx.x;
  const int P = B * n_seeds;
  int64_t a = windows[2 * (int64_t)blockIdx.x], b = windows[2 * (int64_t)blockIdx.x + 1];
  a = a < 0 ? 0 : a;
  b = b > n_sites ? n_sites : b;
  for (int p = tid; p < P; p += 256) sp[p] = 0;
  if (tid < 2) cnt[tid] = 0;
  __syncthreads();
  const int G = (P <= 256) ? 256 / P : 1;
  const int active = (P <= 256) ? G * P : 256;
  const int pstep = (P <= 256) ? P : 256;
  if (tid < active && b > a && n_groups > 0) {
    const int j = (P <= 256) ? tid / P : 0;
    const int g0 = cp_first_group(gend, n_groups, a);
    for (int p = tid - j * P; p < P; p += pstep) {
      const int s = p / B, bb = p - s * B;
      int g = g0, acc = 0;
      int64_t t = a + j;
      while (t < b) {
        while (g < n_groups && t >= gend[g]) ++g;
        if (g >= n_groups) break;
        const int64_t gb = gbeg[g];
        if (t <= gb) {  // sites inside no group, or the group's first row: on to this thread's first site behind it
          t += (gb + 1 - t + G - 1) / G * G;
          continue;
        }
        const int64_t stop = gend[g] < b ? gend[g] : b;
        // the group's rows of this seed block are consecutive: a fixed stride from site to site
        int64_t i = (blk[(int64_t)g * n_seeds + s] + (t - gb)) * B + bb;
        const int64_t di = (int64_t)G * B;
        // four sites' loads are independent, so they are in flight together
        for (; t + 3 * (int64_t)G < stop; t += 4 * (int64_t)G, i += 4 * di)
          acc += cp_event<KIND>(merged, control, kase, i, B) + cp_event<KIND>(merged, control, kase, i + di, B) +
                 cp_event<KIND>(merged, control, kase, i + 2 * di, B) +
                 cp_event<KIND>(merged, control, kase, i + 3 * di, B);
        for (; t < stop; t += G, i += di) acc += cp_event<KIND>(merged, control, kase, i, B);
      }
      if (acc) atomicAdd(&sp[p], acc);
    }
  }
  __syncthreads();
  int n_any = 0, n_one = 0;
  for (int p = tid; p < P; p += 256) {
    const int v = sp[p];
    n_any += (v >= 1) ? 1 : 0;
    n_one += (v == 1) ? 1 : 0;
  }
  if (n_any) atomicAdd(&cnt[0], n_any);
  if (n_one) atomicAdd(&cnt[1], n_one);
  __syncthreads();
  if (tid < 2) out[2 * (int64_t)blockIdx.x + tid] = cnt[tid];
}

// ----------------------------------------------------- window intervals
// sh[0] = the sum of one value per thread; sh may be reused on return.
__device__ __forceinline__ int64_t cp_block_sum(int64_t v, int64_t* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) sh[tid] += sh[tid + off];
    __syncthreads();
  }
  const int64_t r = sh[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ int64_t cp_block_min(int64_t v, int64_t* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off && sh[tid + off] < sh[tid]) sh[tid] = sh[tid + off];
    __syncthreads();
  }
  const int64_t r = sh[0];
  __syncthreads();
  return r;
}

// One workgroup per window [a, b) of column `col` of the int32 matrix: a first
// walk gives E_tot, max c and its first site; a second walk goes over the
// window in chunks of 256 sites with the running sum C carried from chunk to
// chunk (an inclusive Hillis-Steele scan in LDS per chunk), every site testing
// the two int64 conditions of lo and hi. tail = level_den - level_num.
__global__ void __launch_bounds__(256)
cp_window_intervals_kernel(const int32_t* __restrict__ events, int stride, int col, int64_t n_sites,
                           const int64_t* __restrict__ windows, int tail, int den, int64_t* __restrict__ out) {
  __shared__ int64_t sh[256];
  __shared__ int64_t sh_v[256], sh_t[256];
  const int tid = threadIdx.x;
  int64_t a = windows[2 * (int64_t)blockIdx.x], b = windows[2 * (int64_t)blockIdx.x + 1];
  a = a < 0 ? 0 : a;
  b = b > n_sites ? n_sites : b;
  const int64_t kNone = INT64_MAX;
  int64_t sum = 0, best = INT64_MIN, best_t = kNone;
  for (int64_t t = a + tid; t < b; t += 256) {
    const int64_t v = events[t * stride + col];
    sum += v;
    if (v > best) {  // ascending t: the first site of the thread's maximum stays
      best = v;
      best_t = t;
    }
  }
  const int64_t e_tot = cp_block_sum(sum, sh);
  if (e_tot <= 0) {  // uniform over the workgroup
    if (tid == 0) {
      int64_t* o = out + 4 * (int64_t)blockIdx.x;
      o[0] = 0;
      o[1] = a;
      o[2] = a;
      o[3] = b - 1;
    }
    return;
  }
  sh_v[tid] = best;
  sh_t[tid] = best_t;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      const int64_t v = sh_v[tid + off], t = sh_t[tid + off];
      if (v > sh_v[tid] || (v == sh_v[tid] && t < sh_t[tid])) {
        sh_v[tid] = v;
        sh_t[tid] = t;
      }
    }
    __syncthreads();
  }
  const int64_t mode = sh_t[0];
  const int64_t thr = (int64_t)tail * e_tot, den2 = 2 * (int64_t)den;
  int64_t carry = 0, lo = kNone, hi = -1;
  for (int64_t base = a; base < b; base += 256) {
    const int64_t t = base + tid;
    const int64_t v = t < b ? (int64_t)events[t * stride + col] : 0;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const int64_t x = tid >= off ? sh[tid - off] : 0;
      __syncthreads();
      sh[tid] += x;
      __syncthreads();
    }
    const int64_t c_incl = carry + sh[tid];  // C(t)
    carry += sh[255];
    __syncthreads();
    if (t < b) {
      if (lo == kNone && den2 * c_incl > thr) lo = t;
      if (den2 * (e_tot - (c_incl - v)) > thr) hi = t;
    }
  }
  lo = cp_block_min(lo, sh);
  hi = -cp_block_min(-hi, sh);
  if (tid == 0) {
    int64_t* o = out + 4 * (int64_t)blockIdx.x;
    o[0] = e_tot;
    o[1] = mode;
    o[2] = lo;
    o[3] = hi;
  }
}

// ---------------------------------------------------------------- launchers
int launch_cp_site_events(const int16_t* merged, const int16_t* control, const int16_t* kase, int B,
                          const int64_t* desc, int n_groups, int n_seeds, int64_t n_sites, int32_t* events,
                          void* stream) {
  if (n_sites <= 0 || n_groups <= 0) return 0;
  const int64_t nb = (n_sites + kCpTile - 1) / kCpTile;
  // the trajectory arrays are [rows][B][2] int16: one 32-bit word per (d, r) pair
  hipLaunchKernelGGL(cp_site_events_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, merged,
                     (const uint32_t*)control, (const uint32_t*)kase, B, desc, desc + n_groups, desc + 2 * n_groups,
                     n_groups, n_seeds, n_sites, events);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int KIND>
static void cp_launch_counts(const int16_t* merged, const int16_t* control, const int16_t* kase, int B,
                             const int64_t* desc, int n_groups, int n_seeds, int64_t n_sites, const int64_t* windows,
                             int64_t n_windows, int32_t* counts, hipStream_t s) {
  const size_t lds = sizeof(int32_t) * (size_t)B * (size_t)n_seeds;
  hipLaunchKernelGGL(cp_window_counts_kernel<KIND>, dim3((unsigned)n_windows), dim3(256), lds, s, merged,
                     (const uint32_t*)control, (const uint32_t*)kase, B, desc, desc + n_groups, desc + 2 * n_groups,
                     n_groups, n_seeds, n_sites, windows, counts);
}

int launch_cp_window_counts(const int16_t* merged, const int16_t* control, const int16_t* kase, int B,
                            const int64_t* desc, int n_groups, int n_seeds, int64_t n_sites, int kind,
                            const int64_t* windows, int64_t n_windows, int32_t* counts, void* stream) {
  if (n_windows <= 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  switch (kind) {
    case 0: cp_launch_counts<0>(merged, control, kase, B, desc, n_groups, n_seeds, n_sites, windows, n_windows, counts, s); break;
    case 1: cp_launch_counts<1>(merged, control, kase, B, desc, n_groups, n_seeds, n_sites, windows, n_windows, counts, s); break;
    case 2: cp_launch_counts<2>(merged, control, kase, B, desc, n_groups, n_seeds, n_sites, windows, n_windows, counts, s); break;
    case 3: cp_launch_counts<3>(merged, control, kase, B, desc, n_groups, n_seeds, n_sites, windows, n_windows, counts, s); break;
    case 4: cp_launch_counts<4>(merged, control, kase, B, desc, n_groups, n_seeds, n_sites, windows, n_windows, counts, s); break;
    default: return -1;
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_cp_window_intervals(const int32_t* events, int stride, int column, int64_t n_sites, const int64_t* windows,
                               int64_t n_windows, int level_num, int level_den, int64_t* out, void* stream) {
  if (n_windows <= 0) return 0;
  hipLaunchKernelGGL(cp_window_intervals_kernel, dim3((unsigned)n_windows), dim3(256), 0, (hipStream_t)stream, events,
                     stride, column, n_sites, windows, level_den - level_num, level_den, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace hyg
