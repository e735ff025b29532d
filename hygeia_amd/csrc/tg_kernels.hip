// tg_kernels.hip -- CDNA4 (gfx950) kernels of the two-group change-point path.
//
//   tg_emission_kernel   per-site Beta-Binomial emission table (HBM streaming)
//   tg_forward_kernel    particle filter with optimal finite-state resampling,
//                        one workgroup per chain, persistent over the T sites
//   tg_backward_kernel   backward simulation of B trajectories, one workgroup
//                        per chain, regenerating each step's particles from the
//                        forward's ancestor history (read one step ahead)
//
// The chain kernels stand in headers, each including the one before it:
// tg_dev.h (priorities, sort keys, the model in LDS, the LDS layout),
// tg_weights.h (a step's weights), tg_resample.h (the resampling paths),
// tg_forward.h and tg_backward.h (the two kernels); tg_rows.h (on tg_forward.h)
// holds the row tables and the launch thunks. Here: the emission kernels, the
// rows of the full builds, the plans, the forward schedule and the launchers.
// tg_kernels_fo.hip, tg_kernels_trc.hip and tg_kernels_res.hip hold the
// forward-only (REC = false), traced (TRC) and resuming (RES) builds of
// tg_forward_kernel and their rows, on tg_rows.h alone: no backward kernel.
//
// Every index decision uses the arithmetic contract of include/hyg_arith.h
// (exact integer mass sums, deterministic exp/log, Philox streams), so the
// results are bit-identical to the CPU oracle (oracle/tg_oracle.c) whatever the
// reduction tree; that freedom is what the kernels use to parallelise.
//
// Latency design (one chain = a sequential recursion of ~110k steps, so the
// per-step critical path is what matters): model constants and hazard rows
// are read from LDS (hazard rows of the next step's ancestors are prefetched
// one step ahead), the resampling sort runs in registers / wave shuffles with
// LDS only for cross-wave stages, the K / log c search runs in one wave with
// 64-way probes, and reductions are fused to two block barriers per step.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <vector>

#include "tg_backward.h"
#include "tg_rows.h"

namespace hyg {

// --------------------------------------------------------------- kernels
// One thread per site of a 256-site tile; the tile's rows [256][2K] f64 are
// assembled in LDS and written out as whole 16-byte pieces by consecutive
// lanes (a thread writing its own 96-byte row in 8-byte stores left partial
// lines: 1.36x the algorithmic write bytes at K = 6).
constexpr int kETile = 256;
__global__ void __launch_bounds__(kETile)
tg_emission_kernel(const double* __restrict__ lf, const double* __restrict__ lg, const double* __restrict__ cst,
                   int L, int K, const uint16_t* __restrict__ meth_c, const uint16_t* __restrict__ tot_c, int s_c,
                   const uint16_t* __restrict__ meth_k, const uint16_t* __restrict__ tot_k, int s_k, int64_t T,
                   double* __restrict__ E) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* tile = (double*)smem;  // [kETile][2K]
  const int K2 = 2 * K;
  for (int64_t t0 = (int64_t)blockIdx.x * kETile; t0 < T; t0 += (int64_t)gridDim.x * kETile) {
    const int64_t t = t0 + threadIdx.x;
    if (t < T) {
      for (int g = 0; g < 2; ++g) {
        const int S = g ? s_k : s_c;
        const uint16_t* my = g ? meth_k + t * s_k : meth_c + t * s_c;
        const uint16_t* nt = g ? tot_k + t * s_k : tot_c + t * s_c;
        double e[HYG_KMAX];
        for (int r = 0; r < K; ++r) e[r] = 0.0;
        for (int s = 0; s < S; ++s) {
          const int n = nt[s], y = my[s];
          if (n == 0) continue;
          if (y > n || n >= L) {  // invalid input: poison the row
            for (int r = 0; r < K; ++r) e[r] = HYG_NAN;
            break;
          }
          double base = lf[n] - lf[y];
          base = base - lf[n - y];
          for (int r = 0; r < K; ++r) {
            double term = base + lg[(size_t)(r * 3 + 0) * L + y];
            term = term + lg[(size_t)(r * 3 + 1) * L + (n - y)];
            term = term - lg[(size_t)(r * 3 + 2) * L + n];
            term = term + cst[r];
            e[r] = e[r] + term;
          }
        }
        for (int r = 0; r < K; ++r) tile[threadIdx.x * K2 + g * K + r] = e[r];
      }
    }
    __syncthreads();
    // the tile's rows are contiguous in E: 16-byte pieces, consecutive lanes
    const int64_t rows = (T - t0) < kETile ? (T - t0) : kETile;
    const int n = (int)rows * K2;  // doubles; E rows start 16-byte aligned when K2 is even
    double* dst = E + t0 * K2;
    for (int i = 2 * threadIdx.x; i + 1 < n; i += 2 * kETile)
      *(double2*)(dst + i) = make_double2(tile[i], tile[i + 1]);
    if ((n & 1) && threadIdx.x == 0) dst[n - 1] = tile[n - 1];
    __syncthreads();
  }
}

// The same sums from the per-(n, y) term table (hyg_bb_term_table: every
// regime's term of a sample in one row of K doubles, built with the per-term
// kernel's operations, so each entry has the bits that kernel forms): one row
// load per sample instead of 3 + 3K table gathers. The table is L2-sized at
// the pipeline's coverage (0.7 MB at K = 6), so the kernel streams the counts
// in and the rows out at close to the HBM rate. KT > 0: the regime count at
// compile time (rows as 16-byte loads).
template <int KT>
__global__ void __launch_bounds__(kETile)
tg_emission_tab_kernel(const double* __restrict__ bbt, int L, int Kr, const uint16_t* __restrict__ meth_c,
                       const uint16_t* __restrict__ tot_c, int s_c, const uint16_t* __restrict__ meth_k,
                       const uint16_t* __restrict__ tot_k, int s_k, int64_t T, double* __restrict__ E) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* tile = (double*)smem;  // [kETile][2K]
  const int K = KT ? KT : Kr, K2 = 2 * K;
  for (int64_t t0 = (int64_t)blockIdx.x * kETile; t0 < T; t0 += (int64_t)gridDim.x * kETile) {
    const int64_t t = t0 + threadIdx.x;
    if (t < T) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int S = g ? s_k : s_c;
        const uint16_t* my = g ? meth_k + t * s_k : meth_c + t * s_c;
        const uint16_t* nt = g ? tot_k + t * s_k : tot_c + t * s_c;
        double e[KT ? KT : HYG_KMAX];
#pragma unroll
        for (int r = 0; r < (KT ? KT : HYG_KMAX); ++r) e[r] = 0.0;
        bool bad = false;
        // samples in chunks of kCh: every count load of the chunk issued first,
        // then every row load, then the sums in sample order (a sample with
        // n = 0 adds nothing, as the per-term kernel skips it)
        constexpr int kCh = 4;
        // (an even sample count with 4-byte aligned rows: the counts as pairs)
        const bool pairs = (S % 2 == 0) && ((((uintptr_t)my) | ((uintptr_t)nt)) & 3) == 0;
        for (int s0 = 0; s0 < S; s0 += kCh) {
          int nn[kCh], yy[kCh];
          if (pairs) {
#pragma unroll
            for (int j = 0; j < kCh; j += 2) {
              const int sj = s0 + j < S ? s0 + j : S - 2;
              const uint32_t a = *(const uint32_t*)(nt + sj), b = *(const uint32_t*)(my + sj);
              nn[j] = (int)(a & 0xffffu);
              nn[j + 1] = (int)(a >> 16);
              yy[j] = (int)(b & 0xffffu);
              yy[j + 1] = (int)(b >> 16);
            }
          } else {
#pragma unroll
            for (int j = 0; j < kCh; ++j) {
              const int sj = s0 + j < S ? s0 + j : S - 1;
              nn[j] = nt[sj];
              yy[j] = my[sj];
            }
          }
          size_t off[kCh];
          bool use[kCh];
#pragma unroll
          for (int j = 0; j < kCh; ++j) {
            const int n = nn[j], y = yy[j];
            use[j] = s0 + j < S && n != 0;
            bad = bad || (use[j] && (y > n || n >= L));  // invalid input: poison the row
            use[j] = use[j] && y <= n && n < L;
            off[j] = use[j] ? ((size_t)n * (size_t)(n + 1) / 2 + (size_t)y) * (size_t)K : 0;
          }
          if constexpr (KT > 0 && KT % 2 == 0) {
            double2 v[kCh][KT / 2];
#pragma unroll
            for (int j = 0; j < kCh; ++j)
#pragma unroll
              for (int r = 0; r < KT / 2; ++r) v[j][r] = *(const double2*)(bbt + off[j] + 2 * r);
#pragma unroll
            for (int j = 0; j < kCh; ++j)
#pragma unroll
              for (int r = 0; r < KT / 2; ++r) {
                e[2 * r] = use[j] ? e[2 * r] + v[j][r].x : e[2 * r];
                e[2 * r + 1] = use[j] ? e[2 * r + 1] + v[j][r].y : e[2 * r + 1];
              }
          } else {
#pragma unroll
            for (int j = 0; j < kCh; ++j)
              if (use[j])
                for (int r = 0; r < K; ++r) e[r] = e[r] + bbt[off[j] + r];
          }
        }
        for (int r = 0; r < K; ++r) tile[threadIdx.x * K2 + g * K + r] = bad ? HYG_NAN : e[r];
      }
    }
    __syncthreads();
    const int64_t rows = (T - t0) < kETile ? (T - t0) : kETile;
    const int n = (int)rows * K2;
    double* dst = E + t0 * K2;
    for (int i = 2 * threadIdx.x; i + 1 < n; i += 2 * kETile)
      *(double2*)(dst + i) = make_double2(tile[i], tile[i + 1]);
    if ((n & 1) && threadIdx.x == 0) dst[n - 1] = tile[n - 1];
    __syncthreads();
  }
}

// -------------------------------------------------------------- launchers
// Optional per-kernel timing with HIP events recorded on the launch stream
// (bench.py reads them back with hyg_tg_last_kernel_ms). The events belong to
// the device they were created on and are recreated when the calling thread's
// device changes; one mutex orders every use of them.
namespace {
std::mutex g_ev_mu;
bool g_timing = false;
int g_ev_dev = -1;
hipEvent_t g_ev[6] = {};
bool g_ev_used[3] = {false, false, false};
void ev_record(int k, bool end, hipStream_t s) {
  std::lock_guard<std::mutex> lock(g_ev_mu);
  if (!g_timing) return;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  if (dev != g_ev_dev) {  // new device: the old device's events cannot be recorded here
    for (int i = 0; i < 6; ++i) {
      if (g_ev[i]) (void)hipEventDestroy(g_ev[i]);
      g_ev[i] = nullptr;
    }
    for (int i = 0; i < 3; ++i) g_ev_used[i] = false;
    g_ev_dev = dev;
  }
  hipEvent_t& e = g_ev[2 * k + (end ? 1 : 0)];
  if (!e) (void)hipEventCreate(&e);
  (void)hipEventRecord(e, s);
  g_ev_used[k] = true;
}
// A launch without kernel k (launch_filter has no backward): last_kernel_ms reports -1 for it.
void ev_unused(int k) {
  std::lock_guard<std::mutex> lock(g_ev_mu);
  g_ev_used[k] = false;
}
// CUs of each device (the launch-width and tail-overlap choices depend on
// them), cached per device: a process that switches devices (hyg_set_device)
// sees each device's own count. hyg_tg_set_device_cus overrides an entry
// (tests fake devices of other sizes); 0 = unknown / query again.
constexpr int kMaxDevices = 64;
std::atomic<int> g_cus[kMaxDevices];
int query_cus(int dev) {
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 0;
  return n;
}
int cus_of(int dev) {
  if (dev < 0) return 0;
  if (dev >= kMaxDevices) return query_cus(dev);
  int n = g_cus[dev].load(std::memory_order_relaxed);
  if (n > 0) return n;
  n = query_cus(dev);
  if (n > 0) g_cus[dev].store(n, std::memory_order_relaxed);
  return n;
}
int device_cus() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  const int n = cus_of(dev);
  return n > 0 ? n : 256;
}
int g_force_threads[2] = {0, 0};  // hyg_tg_force_threads (tests): forward, backward; 0 = automatic
bool valid_width(int x) { return x == 64 || x == 128 || x == 256 || x == 512 || x == 768; }
// hyg_tg_set_gather_window: sorted positions of the top set whose ancestors
// the forward gathers ahead (Ahead; a kernel takes what its idle waves and its
// dead LDS hold of it). The top set has at most 256 positions.
constexpr int kMaxGatherWindow = 256;
constexpr int kDefaultGatherWindow = 192;
std::atomic<int> g_gather_window{kDefaultGatherWindow};
}  // namespace

int tg_set_gather_window(int positions) {
  if (positions < -1 || positions > kMaxGatherWindow) return HYG_EINVAL;
  g_gather_window.store(positions < 0 ? kDefaultGatherWindow : positions, std::memory_order_relaxed);
  return HYG_OK;
}

// hyg_tg_set_priority_rotation: whether the 256-thread forward kernels rotate
// their waves' base priorities (prio_base); reaches them in Lay::prio_rot.
std::atomic<int> g_prio_rot{1};
void tg_set_priority_rotation(bool on) { g_prio_rot.store(on ? 1 : 0, std::memory_order_relaxed); }
// hyg_tg_set_fine_list_walk: whether the 256-thread forward kernels with their
// weights in LDS walk their candidate lists per 64 entries (list_walk);
// reaches them in Lay::list_fine.
std::atomic<int> g_list_fine{1};
void tg_set_fine_list_walk(bool on) { g_list_fine.store(on ? 1 : 0, std::memory_order_relaxed); }
int tg_fine_list_walk() { return g_list_fine.load(std::memory_order_relaxed); }
int tg_priority_base(unsigned long long ticks, int slot) {
  return slot < 0 ? -1 : prio_base_at(ticks, slot % 3);
}
int tg_priority_epoch_ticks() { return 1 << kPrioEpochShift; }

int tg_force_threads(int fwd, int bwd) {
  if ((fwd && !valid_width(fwd)) || (bwd && !valid_width(bwd))) return HYG_EINVAL;
  g_force_threads[0] = fwd;
  g_force_threads[1] = bwd;
  return HYG_OK;
}

int tg_device_cus(int dev) { return cus_of(dev); }
int tg_set_device_cus(int dev, int cus) {
  if (dev < 0 || dev >= kMaxDevices || cus < 0) return HYG_EINVAL;
  g_cus[dev].store(cus, std::memory_order_relaxed);
  return HYG_OK;
}

void set_kernel_timing(bool on) {
  std::lock_guard<std::mutex> lock(g_ev_mu);
  g_timing = on;
}

int last_kernel_ms(float* out3) {
  std::lock_guard<std::mutex> lock(g_ev_mu);
  for (int k = 0; k < 3; ++k) {
    out3[k] = -1.0f;
    if (!g_ev_used[k] || !g_ev[2 * k] || !g_ev[2 * k + 1]) continue;
    if (hipEventSynchronize(g_ev[2 * k + 1]) != hipSuccess) return HYG_EDEVICE;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, g_ev[2 * k], g_ev[2 * k + 1]) != hipSuccess) return HYG_EDEVICE;
    out3[k] = ms;
  }
  return HYG_OK;
}


int launch_emission(const ModelDev& md, const hyg_tg_consts& c, const uint16_t* meth_c, const uint16_t* tot_c,
                    int s_c, const uint16_t* meth_k, const uint16_t* tot_k, int s_k, int64_t n_sites, double* E,
                    void* stream) {
  if (n_sites <= 0) return HYG_OK;
  int64_t blocks = (n_sites + kETile - 1) / kETile;
  if (blocks > 256 * 16) blocks = 256 * 16;
  ev_record(0, false, (hipStream_t)stream);
  const size_t lds = sizeof(double) * kETile * 2 * c.K;
  const int L = md.nmax_reads + 1;
  if (md.bbt && c.K == 6) {
    hipLaunchKernelGGL(tg_emission_tab_kernel<6>, dim3((unsigned)blocks), dim3(kETile), lds, (hipStream_t)stream,
                       md.bbt, L, c.K, meth_c, tot_c, s_c, meth_k, tot_k, s_k, n_sites, E);
  } else if (md.bbt && c.K == 12) {
    hipLaunchKernelGGL(tg_emission_tab_kernel<12>, dim3((unsigned)blocks), dim3(kETile), lds, (hipStream_t)stream,
                       md.bbt, L, c.K, meth_c, tot_c, s_c, meth_k, tot_k, s_k, n_sites, E);
  } else if (md.bbt) {
    hipLaunchKernelGGL(tg_emission_tab_kernel<0>, dim3((unsigned)blocks), dim3(kETile), lds, (hipStream_t)stream,
                       md.bbt, L, c.K, meth_c, tot_c, s_c, meth_k, tot_k, s_k, n_sites, E);
  } else {
    hipLaunchKernelGGL(tg_emission_kernel, dim3((unsigned)blocks), dim3(kETile), lds, (hipStream_t)stream, md.lf,
                       md.lg, md.cst, L, c.K, meth_c, tot_c, s_c, meth_k, tot_k, s_k, n_sites, E);
  }
  ev_record(0, true, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? HYG_OK : HYG_EDEVICE;
}

// ------------------------------------------------- which chain kernel runs
// plan() below is the one place that decides it, per direction of a launch:
// the width, whether the full-N arrays are global (GW), the LDS layout and the
// instantiation. The launch, the occupancy query and the diagnostics of the C
// ABI read its KernelPlan (DESIGN.md section 3 points here).
constexpr size_t kCuLdsBytes = 160 * 1024;  // LDS of one CU

// The launch thunk of a backward row, over tg_backward_kernel's template arguments (the forward's: tg_rows.h).
template <int NT, int KC, int MC, int BC, bool PHS, bool GW, bool MM = false>
void backward_thunk(const ChainLaunch& a) {
  hipLaunchKernelGGL((tg_backward_kernel<NT, KC, MC, BC, PHS, GW, MM>), dim3(a.grid), dim3(NT), a.lds, a.stream,
                     model_arg<MM>(a.m), a.chains, a.E, (const uint8_t*)a.ws, (const int32_t*)a.out.status,
                     a.out.merged, a.out.control, a.out.kase, a.out.split_probs, a.out.regime_probs, a.out.status,
                     a.lay, a.dbg, a.ws);
}
#define FWD(...) TG_ROW(forward, __VA_ARGS__)
#define BWD(...) TG_ROW(backward, __VA_ARGS__)
// Of the GW builds only the C5 backward's has phase timers. (Rows in the order
// the code object has always held the kernels, which is the order of first
// mention: any other order moves every kernel's address.)
static const KernelRow kFwdRows[] = {
    FWD(64, 0, 0, 0, false, false),  FWD(128, 0, 0, 0, false, false),  FWD(256, 0, 0, 0, false, true),
    FWD(256, 6, 50, 25, true, false),  FWD(256, 0, 0, 0, true, false),  FWD(256, 6, 50, 25, false, false),
    FWD(256, 0, 0, 0, false, false),  FWD(768, 6, 50, 25, true, false),  FWD(768, 0, 0, 0, true, false),
    FWD(768, 6, 50, 25, false, false),  FWD(768, 12, 50, 25, false, false),  FWD(768, 0, 0, 0, false, false),
    FWD(512, 6, 50, 25, true, false),  FWD(512, 12, 50, 25, true, false),  FWD(512, 0, 0, 0, true, false),
    FWD(512, 6, 50, 25, false, false),  FWD(512, 12, 50, 25, false, false),  FWD(512, 0, 0, 0, false, false),
};
static const KernelRow kBwdRows[] = {
    BWD(64, 0, 0, 0, false, false),  BWD(128, 0, 0, 0, false, false),  BWD(256, 0, 0, 0, false, true),
    BWD(256, 12, 50, 25, true, true),  BWD(256, 12, 50, 25, false, true),  BWD(256, 6, 50, 25, true, false),
    BWD(256, 0, 0, 0, true, false),  BWD(256, 6, 50, 25, false, false),  BWD(256, 0, 0, 0, false, false),
    BWD(768, 6, 50, 25, true, false),  BWD(768, 0, 0, 0, true, false),  BWD(768, 6, 50, 25, false, false),
    BWD(768, 12, 50, 25, false, false),  BWD(768, 0, 0, 0, false, false),  BWD(512, 6, 50, 25, true, false),
    BWD(512, 0, 0, 0, true, false),  BWD(512, 6, 50, 25, false, false),  BWD(512, 12, 50, 25, false, false),
    BWD(512, 0, 0, 0, false, false),
};
#undef BWD
#undef FWD
// The multi-model builds (MM, the seventh argument, which their names carry):
// the forward's are the plain builds of tg_rows.h, the backward's those and
// the C5 GW one at 256. No phase-timer builds: a phase-timer request on a
// multi-model launch runs the plain build (find_row). They stand behind the
// single-model rows, whose kernels so keep their order.
#define FWD_MM(NT, KC, MC, BC, GW) TG_ROW(forward, NT, KC, MC, BC, false, GW,true),
#define BWD_MM(NT, KC, MC, BC, GW) TG_ROW(backward, NT, KC, MC, BC, false, GW,true)
static const KernelRow kFwdRowsMm[] = {TG_PLAIN_BUILDS(FWD_MM)};
static const KernelRow kBwdRowsMm[] = {
    BWD_MM(64, 0, 0, 0, false),     BWD_MM(128, 0, 0, 0, false),    BWD_MM(256, 0, 0, 0, true),
    BWD_MM(256, 12, 50, 25, true),  BWD_MM(256, 6, 50, 25, false),  BWD_MM(256, 0, 0, 0, false),
    BWD_MM(768, 6, 50, 25, false),  BWD_MM(768, 12, 50, 25, false), BWD_MM(768, 0, 0, 0, false),
    BWD_MM(512, 6, 50, 25, false),  BWD_MM(512, 12, 50, 25, false), BWD_MM(512, 0, 0, 0, false),
};
#undef BWD_MM
#undef FWD_MM

// The row of a request, by preference: the shape's phase-timer build, the
// generic one (both only when phase timers are wanted), the shape's plain
// build, the generic one. So a shape at a width without a build of it runs the
// generic build, a phase-timer request where no such build exists a plain one
// (and C5 where only its plain build exists is timed in the generic build).
// Every width has a generic plain row, and 256 a generic GW one. The same
// among the multi-model rows (mm), which have plain builds only, and among the
// forward-only rows (!rec: the forward of a launch_filter), which have plain
// builds only as well, and among the traced rows (trc: a launch_trace).
static const KernelRow* find_row(bool backward, int nt, Shape shape, bool phases, bool gw, bool mm, bool rec = true,
                                 bool trc = false) {
  size_t n = 0;
  const KernelRow* rows = backward ? pick_rows(kBwdRows, kBwdRowsMm, mm, &n) : pick_rows(kFwdRows, kFwdRowsMm, mm, &n);
  if (!rec) rows = backward ? nullptr : (trc ? trc_rows(mm, &n) : fo_rows(mm, &n));
  if (!rows) return nullptr;
  for (int pref = phases ? 0 : 2; pref < 4; ++pref) {
    const Shape sh = (pref & 1) ? kGeneric : shape;
    for (size_t i = 0; i < n; ++i)
      if (rows[i].nt == nt && rows[i].shape == sh && rows[i].phases == (pref < 2) && rows[i].gw == gw) return &rows[i];
  }
  return nullptr;
}

static Shape shape_of(const hyg_tg_consts& c) {
  static const bool off = tuning_env("HYG_NO_SHAPE") != nullptr;
  if (off || c.M != 50 || c.B != 25) return kGeneric;
  if (c.K == 6 && c.I == 48 && c.Nmax == 2400) return kC3;
  if (c.K == 12 && c.I == 168 && c.Nmax == 8400) return kC5;
  return kGeneric;
}
// A shape keeps its particle arrays in global memory exactly when the forward's
// LDS layout at the default width exceeds a CU's LDS (every shape that fits
// keeps its kernels, its layouts and its workspace).
bool forward_global_w(const hyg_tg_consts& c) {
  return make_layout(c.K, c.M, c.B, c.Nmax, kDefaultThreads, false).total > kCuLdsBytes;
}
bool backward_global_w(const hyg_tg_consts& c) { return shape_of(c) == kC5 || forward_global_w(c); }
size_t chain_scratch_bytes(const hyg_tg_consts& c) {
  if (forward_global_w(c)) return align_up(fwd_scratch_bytes(c.Nmax, 256), 256);
  return backward_global_w(c) ? align_up((size_t)c.Nmax * sizeof(double), 256) : 0;
}
// Only the 256-thread kernels have builds with the full-N arrays in global memory.
static bool width_gw(bool backward, const hyg_tg_consts& c, int nt) {
  return nt == 256 && (backward ? backward_global_w(c) : forward_global_w(c));
}
static Lay layout_at(bool backward, const hyg_tg_consts& c, int nt) {
  return make_layout(c.K, c.M, c.B, c.Nmax, nt, backward, width_gw(backward, c, nt));
}
// Whether a chain kernel of a width can run the shape: its LDS layout within a
// CU's LDS and one thread per resampled ancestor (the record read-ahead).
static bool width_fits(bool backward, const hyg_tg_consts& c, int nt) {
  return c.M <= nt && layout_at(backward, c, nt).total <= kCuLdsBytes;
}

// The width asked for. HYG_THREADS (or HYG_THREADS_FWD / _BWD) if set.
// Otherwise by what the launch's chains leave of the GPU:
//  - the forward's LDS at 256 threads already forces one workgroup per CU
//    (K = 12, C5: 145 KB): 512 (forward) / 768 (backward), more waves on the
//    CU's one chain;
//  - at most one chain per CU (e.g. an 8-GPU rank of the C3 job, 73 chains):
//    kLowOccThreads (forward) / kLowOccThreadsBwd (backward), whose extra
//    waves shorten the parallel phases of each step of the sequential chain
//    (HYG_LOWOCC_THREADS: 256, 512 or 768 for both);
//  - else 256, up to three chains per CU (<= 168 VGPRs: C3 on one GPU, 582
//    chains; an 8-GPU rank of C4, 291). A 384-thread workgroup does not buy
//    two chains per CU: its six waves land 2-2-1-1 on the SIMDs, so a second
//    one would need four waves on a SIMD that holds three.
static int tuning_int(const char* name, const char* fallback = nullptr) {
  const char* v = tuning_env(name);
  if (!v && fallback) v = tuning_env(fallback);
  return v ? atoi(v) : 0;
}
static int pick_threads(bool backward, const hyg_tg_consts& c, int n_chains) {
  const int k = backward ? 1 : 0;
  if (g_force_threads[k]) return g_force_threads[k];
  static const int env[2] = {tuning_int("HYG_THREADS_FWD", "HYG_THREADS"), tuning_int("HYG_THREADS_BWD", "HYG_THREADS")};
  static const int lowocc_env = tuning_int("HYG_LOWOCC_THREADS");
  const int lowocc = (lowocc_env == 256 || lowocc_env == 512 || lowocc_env == 768) ? lowocc_env : 0;
  if (valid_width(env[k])) return env[k];
  const int def = backward ? kDefaultThreadsBwd : kDefaultThreads;
  if (c.M > 64) return def;  // the wider kernels assume the pipeline's M <= 64 (one ancestor per lane)
  const size_t lds = make_layout(c.K, c.M, c.B, c.Nmax, def, false).total;
  // (C5: the backward's list path keeps its 12 waves busy: 768 threads, 6 %
  // faster than 512 in r03d; the forward is faster at 512). With more chains
  // than CUs the C5 backward runs at 256 threads with its full-N weights in
  // global memory (GW): three chains per CU instead of one.
  if (backward && backward_global_w(c) && n_chains > device_cus()) return 256;
  if (2 * lds > kCuLdsBytes) return backward ? 768 : 512;
  if (n_chains <= device_cus()) return lowocc ? lowocc : (backward ? kLowOccThreadsBwd : kLowOccThreads);
  return def;
}

struct KernelPlan {
  int status;  // HYG_EUNSUPPORTED: no width runs the shape (M > 256)
  int nt;      // threads per chain workgroup
  bool gw;     // the instantiation keeps its full-N arrays in the chain's global scratch
  Lay lay;     // make_layout for exactly (nt, direction, gw), the HYG_TOPSET_R override applied
  const KernelRow* k;  // the instantiation: function pointer, phase-timer build or not, name
  size_t lds;          // dynamic LDS of the launch: lay.total and, traced, the class sums behind it
};
// The plan of one direction of a launch of n_chains chains. The width is the
// one picked above (forced, tuned or automatic) where its kernel can run the
// shape, else 256. A shape whose particle arrays exceed LDS (forward_global_w)
// has the one width 256, whose kernels keep them in global memory; a shape just
// under that limit fits at 256 threads but not with the few hundred bytes more
// of a wider workgroup's layout; a forced width below M has too few threads. So
// no choice or override of the width makes a supported shape fail; M > 256 has
// no width, which the status says. A multi-model launch (mm) is planned from
// the shape its models share and its chain count, exactly as a single-model
// launch of that many chains, and takes the multi-model row of the result. A
// forward-only launch (!rec, launch_filter) is planned exactly as the forward
// of a full launch of that many chains, and takes the REC = false row of the
// result. A traced launch (trc, launch_trace) is planned as the forward-only
// launch of that many chains, with its layout, and takes the TRC row; its LDS
// is the layout's and, from K = 9, the class sums behind it (trace_bins_extra),
// which in a shape within that many bytes of a CU's LDS moves the launch to 256
// threads as a layout that does not fit does.
static KernelPlan plan(bool backward, const hyg_tg_consts& c, int n_chains, bool mm = false, bool rec = true,
                       bool trc = false) {
  KernelPlan p{};
  p.nt = forward_global_w(c) ? 256 : pick_threads(backward, c, n_chains);
  const size_t more = trc ? trace_bins_extra(c.K) : 0;
  auto fits = [&](int nt) { return width_fits(backward, c, nt) && layout_at(backward, c, nt).total + more <= kCuLdsBytes; };
  if (!fits(p.nt)) p.nt = 256;
  p.gw = width_gw(backward, c, p.nt);
  p.lay = layout_at(backward, c, p.nt);
  p.lds = p.lay.total + more;
  p.status = fits(p.nt) ? HYG_OK : HYG_EUNSUPPORTED;
  static const int topset_r = tuning_int("HYG_TOPSET_R");  // tuning: 1 (A <= 64 per wave) or 2
  if (!backward && (topset_r == 1 || topset_r == 2)) p.lay.topset_r = topset_r;
  static const char* window_env = tuning_env("HYG_GATHER_WINDOW");  // tuning: overrides hyg_tg_set_gather_window
  if (!backward) p.lay.gather_w = window_env ? atoi(window_env) : g_gather_window.load(std::memory_order_relaxed);
  if (!backward) p.lay.prio_rot = g_prio_rot.load(std::memory_order_relaxed);
  if (!backward) p.lay.list_fine = g_list_fine.load(std::memory_order_relaxed);
  // HYG_DEBUG_PHASES=1 (tuning build) asks for the phase-timer instantiations
  static const bool phases = tuning_env("HYG_DEBUG_PHASES") != nullptr;
  p.k = find_row(backward, p.nt, shape_of(c), phases, p.gw, mm, rec, trc);
  return p;
}

int tg_threads_per_chain(const hyg_tg_consts& c, int n_chains) { return plan(false, c, n_chains).nt; }
int tg_threads_per_chain_bwd(const hyg_tg_consts& c, int n_chains) { return plan(true, c, n_chains).nt; }
int tg_kernel_name(const hyg_tg_consts& c, int n_chains, bool backward, const char** name, bool multi) {
  const KernelPlan p = plan(backward, c, n_chains, multi);
  *name = p.k->name;
  return p.status;
}
int tg_filter_kernel_name(const hyg_tg_consts& c, int n_chains, const char** name, bool multi) {
  const KernelPlan p = plan(false, c, n_chains, multi, false);
  *name = p.k->name;
  return p.status;
}
int tg_trace_kernel_name(const hyg_tg_consts& c, int n_chains, const char** name, bool multi) {
  const KernelPlan p = plan(false, c, n_chains, multi, false, true);
  *name = p.k->name;
  return p.status;
}
size_t tg_trace_lds_bytes(const hyg_tg_consts& c, int n_chains) { return plan(false, c, n_chains, false, false, true).lds; }
size_t tg_layout_bytes(const hyg_tg_consts& c, int threads, bool backward) {
  if (!valid_width(threads)) return 0;
  if (forward_global_w(c) && threads != 256) return 0;  // such a shape has no other width
  return layout_at(backward, c, threads).total;
}
// Forward workgroups one CU holds at the width a launch of n_chains uses
// (the occupancy query on the kernel instantiation and its dynamic LDS).
static int resident_per_cu(const KernelPlan& pf) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, pf.k->fn, pf.nt, pf.lds) != hipSuccess) return -1;
  return nb;
}
int tg_resident_per_cu(const hyg_tg_consts& c, int n_chains) { return resident_per_cu(plan(false, c, n_chains)); }

// ------------------------------------------------- the forward in rounds
// A launch of n chains on a device of C CUs puts blocks b, b + C, b + 2C on
// one CU, so with k = n / C and e = n % C the first e CUs hold k + 1 chains for
// the whole launch and the others k, and a chain beside k others advances more
// slowly than one beside k - 1 (kStepUs). A forward chain is a pure function
// of its history record, so the forward can be cut in time instead: round 1
// runs every chain up to a cut of its own, the kernel ends, and round 2 (the
// resuming build, RES) takes every chain up from its last record in another
// block order, in which the chains of round 1's heavy CUs sit on light ones.
// forward_schedule is the one place that decides it, as data: the cuts and
// round 2's block order ("Launch scheduling").
//
// Microseconds per step of the slowest chain on a CU that holds `load` chains
// of the 256-thread forward, in round 1 and in round 2, from the census of a
// launch in rounds (profiles/r09_census_rounds.txt). Round 1 runs the launch's
// order, longest first, so the third chain of a three-chain CU is one of the
// launch's shortest and ends early; round 2 gives such a CU three chains of
// nearly equal length, and puts the chains with the most left to do into the
// first blocks of the two-chain CUs, which run a little faster than the
// second. 0: never measured, and a launch that mixes such a load is not cut
// unless rounds are forced.
constexpr double kStepUs[][2] = {{0.0, 0.0}, {0.0, 0.0}, {14.44, 14.03}, {15.60, 15.98}};
static double step_us(int load, int round) {
  return load >= 0 && load < (int)(sizeof kStepUs / sizeof *kStepUs) ? kStepUs[load][round] : 0.0;
}
// A launch is only cut when its longest chain has this many steps: an empty
// relaunch measures 0.012 ms (profiles/r09_premeasure.txt), under one percent
// of what the split gains (about 3 %) from about 2 700 steps of 15 us on.
constexpr int kMinSplitSteps = 4096;
constexpr int kCutEvery = 64;  // cuts are 64 q + 1 (tg_forward_kernel, RES)
std::atomic<int> g_forward_rounds{1};  // hyg_tg_set_forward_rounds: 0 one launch, 1 automatic, 2 forced

struct ForwardRounds {
  int rounds = 1;           // 1: one launch, as without this section
  std::vector<int> cut;     // per chain: the first step of round 2 (its T: all of it in round 1)
  std::vector<int> order2;  // round 2's blocks: the chains still running, by block
};
// The legal cut (64 q + 1, from 65 to T - 1) of a chain of T steps nearest to `want`, or T (no cut).
static int legal_cut(int T, double want) {
  long q = std::lround((want - 1.0) / kCutEvery);
  const long qmax = ((long)T - 2) / kCutEvery;  // 64 q + 1 <= T - 1: round 2 has a step to run
  if (q > qmax) q = qmax;
  if (q < 1) q = qmax >= 1 ? 1 : 0;
  return q >= 1 ? (int)(q * kCutEvery + 1) : T;
}
// `splittable`: the launch's forward is the recording 256-thread build with its
// arrays in LDS, no phase timers and no tail overlap. mode as g_forward_rounds.
static ForwardRounds forward_schedule(const int* T, int n, int cus, int resident, int mode, bool splittable) {
  ForwardRounds r;
  r.cut.assign(T, T + n);
  // (one residency round: every block of the launch is on a CU from the start)
  if (mode <= 0 || !splittable || n < 1 || cus < 1 || (long)n > (long)cus * resident) return r;
  const int k = n / cus, e = n % cus;
  // a, b: a heavy and a light CU's rate in round 1; c, d: a light and a heavy CU's in round 2
  const double a = step_us(k + 1, 0), b = step_us(k, 0), c = step_us(k, 1), d = step_us(k + 1, 1);
  const bool rates = a > 0.0 && b > 0.0 && c > 0.0 && d > 0.0;
  const int longest = *std::max_element(T, T + n);
  if (mode == 1 && !(k >= 1 && e > 0 && k + 1 <= resident && (long)e * (k + 1) <= (long)(cus - e) * k && rates &&
                     longest >= kMinSplitSteps))
    return r;
  // Both rounds end together when a heavy chain does the fraction fh of its
  // steps in round 1 and a light one fl: a fh = b fl (round 1) and
  // c (1 - fh) = d (1 - fl) (round 2: the heavy chains on light CUs, light
  // ones on the heavy CUs). Forced rounds on loads never measured, or rates
  // without such a point, cut every chain in half.
  double fh = 0.5, fl = 0.5;
  if (rates && a * d > b * c) {
    const double h = (d - c) * b / (a * d - b * c), l = h * a / b;
    if (h > 0.0 && h < 1.0 && l > 0.0 && l < 1.0) fh = h, fl = l;
  }
  auto heavy1 = [&](int blk) { return k >= 1 && blk % cus < e; };
  std::vector<int> H, L;  // the chains round 2 runs: round 1's heavy ones, the others
  for (int i = 0; i < n; ++i) {
    r.cut[i] = legal_cut(T[i], (heavy1(i) ? fh : fl) * T[i]);
    if (r.cut[i] < T[i]) (heavy1(i) ? H : L).push_back(i);
  }
  const int n2 = (int)(H.size() + L.size());
  if (n2 == 0) return r;  // no chain long enough for a cut
  r.rounds = 2;
  // Round 2: heavy chains into light blocks; the light chains with the least
  // left to do into the heavy blocks; the rest stay light.
  const int k2 = n2 / cus, e2 = n2 % cus;
  auto heavy2 = [&](int p) { return k2 >= 1 && p % cus < e2; };
  std::stable_sort(L.begin(), L.end(), [&](int a, int b) { return T[a] - r.cut[a] < T[b] - r.cut[b]; });
  int n_light = 0;
  for (int p = 0; p < n2; ++p) n_light += !heavy2(p);
  const size_t fit = std::min(H.size(), (size_t)n_light);
  std::vector<int> rest(L);  // least left first, behind them the heavy chains no light block is left for
  rest.insert(rest.end(), H.begin() + fit, H.end());
  r.order2.resize(n2);
  size_t ih = 0, ir = 0, tail = (size_t)(n2 - n_light);  // rest[0, tail): the heavy blocks'; rest[tail, ...): light ones
  for (int p = 0; p < n2; ++p) {
    if (heavy2(p)) r.order2[p] = rest[ir++];
    else r.order2[p] = ih < fit ? H[ih++] : rest[tail++];
  }
  return r;
}

int tg_set_forward_rounds(int mode) {
  if (mode < 0 || mode > 2) return HYG_EINVAL;
  g_forward_rounds.store(mode, std::memory_order_relaxed);
  return HYG_OK;
}
static int forward_rounds_mode() {
  static const char* env = tuning_env("HYG_FORWARD_ROUNDS");  // tuning: overrides hyg_tg_set_forward_rounds
  const int m = env ? atoi(env) : g_forward_rounds.load(std::memory_order_relaxed);
  return m < 0 ? 0 : (m > 2 ? 2 : m);
}
// Whether the forward of a launch may be cut at all (forward_schedule's `splittable`).
static bool forward_splittable(const KernelPlan& pf, bool rec) {
  return rec && pf.status == HYG_OK && pf.nt == 256 && !pf.gw && !pf.k->phases;
}
// hyg_tg_forward_schedule: the schedule of a launch of these lengths on `cus`
// CUs (0: the current device's, as the launcher takes them), per round r < max_rounds and n chains: blocks[r] the
// grid, order[r n + p] the chain of block p (-1 behind the grid), [begin, end)
// [r n + i] the steps chain i runs (empty: not in the round). Returns the rounds.
int tg_forward_schedule(const hyg_tg_consts& c, const int* T, int n, bool multi, bool forward_only, int cus, int resident,
                        int max_rounds, int* blocks, int* order, int* begin, int* end) {
  if (!T || n < 1 || cus < 0 || max_rounds < 2 || !blocks || !order || !begin || !end) return HYG_EINVAL;
  for (int i = 0; i < n; ++i)
    if (T[i] < 1) return HYG_EINVAL;
  const KernelPlan pf = plan(false, c, n, multi, !forward_only);
  if (pf.status != HYG_OK) return pf.status;
  const ForwardRounds fr =
      forward_schedule(T, n, cus ? cus : device_cus(), resident, forward_rounds_mode(), forward_splittable(pf, !forward_only));
  for (int j = 0; j < max_rounds * n; ++j) {
    order[j] = -1;
    begin[j] = end[j] = 0;
  }
  for (int r = 0; r < max_rounds; ++r) blocks[r] = 0;
  blocks[0] = n;
  for (int i = 0; i < n; ++i) {
    order[i] = i;
    begin[i] = 1;
    end[i] = fr.cut[i];
  }
  if (fr.rounds == 2) {
    blocks[1] = (int)fr.order2.size();
    for (size_t p = 0; p < fr.order2.size(); ++p) {
      const int i = fr.order2[p];
      order[n + p] = i;
      begin[n + i] = fr.cut[i];
      end[n + i] = T[i];
    }
  }
  return fr.rounds;
}

// Phase timers (tuning build): a phase-timer instantiation adds its kPh
// counters per chain into a buffer; after the launch they are copied back,
// summed over the chains and reported on stderr.
static unsigned long long* phase_buffer(int n_chains, hipStream_t s) {
  unsigned long long* dbg = nullptr;
  (void)hipMalloc((void**)&dbg, sizeof(unsigned long long) * kPh * n_chains);
  if (dbg) (void)hipMemsetAsync(dbg, 0, sizeof(unsigned long long) * kPh * n_chains, s);
  return dbg;
}
static void phase_totals(unsigned long long* dbg, int n_chains, hipStream_t s, unsigned long long (&tot)[kPh]) {
  std::vector<unsigned long long> h((size_t)kPh * n_chains);
  (void)hipStreamSynchronize(s);
  (void)hipMemcpy(h.data(), dbg, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost);
  (void)hipFree(dbg);
  for (int k = 0; k < kPh; ++k) tot[k] = 0;
  for (int i = 0; i < n_chains; ++i)
    for (int k = 0; k < kPh; ++k) tot[k] += h[(size_t)i * kPh + k];
}
static void report_forward_phases(unsigned long long* dbg, int nt, int n_chains, hipStream_t s) {
  unsigned long long tot[kPh];
  phase_totals(dbg, n_chains, s, tot);
  const double steps = (double)tot[kPh - 1];
  fprintf(stderr, "[hyg phases NT=%d] chains=%d steps=%.0f cycles/step:", nt, n_chains, steps);
  const char* nm[9] = {"top", "lse", "compact", "resample", "fallback", "gather", "wmax", "wgen", "wstore"};
  double sum = 0;
  for (int k = 0; k < 9; ++k) {
    fprintf(stderr, " %s=%.0f", nm[k], tot[k] / steps);
    sum += tot[k] / steps;
  }
  fprintf(stderr, " total=%.0f | keep_steps=%.0f mean_nsig=%.1f mean_n2=%.1f", sum, (double)tot[10],
          tot[9] / (steps - tot[10]), 0.0);
  fprintf(stderr, " | list=%.0f lse loop=%.0f cut sums=%.0f lse reduce=%.0f", tot[22] / steps, tot[23] / steps,
          tot[12] / steps, tot[11] / steps);
  const double opt = steps - tot[10];
  fprintf(stderr, " | topset: compact=%.0f mass=%.0f gatherA=%.0f sort=%.0f prefix=%.0f kloop_sys=%.0f",
          tot[24] / opt, tot[25] / opt, tot[26] / opt, tot[27] / opt, tot[28] / opt, tot[29] / opt);
  fprintf(stderr, " | kloop_sys split: c(a)=%.0f loop=%.0f systematic=%.0f (targets=%.0f search=%.0f tail=%.0f)",
          tot[30] / opt, tot[32] / opt, tot[31] / opt + tot[34] / opt + tot[33] / opt, tot[31] / opt, tot[34] / opt,
          tot[33] / opt);
  fprintf(stderr, " | per optimal step: topset=%.0f fallbacks=%.4f | per fallback: hist=%.0f bscan=%.0f scatter=%.0f "
          "bsort=%.0f scan=%.0f kloop=%.0f systematic=%.0f\n", tot[20] / opt, tot[21] / opt,
          tot[17] / (tot[21] + 1e-9), tot[18] / (tot[21] + 1e-9), tot[19] / (tot[21] + 1e-9),
          tot[13] / (tot[21] + 1e-9), tot[14] / (tot[21] + 1e-9), tot[15] / (tot[21] + 1e-9),
          tot[16] / (tot[21] + 1e-9));
}
static void report_backward_phases(unsigned long long* dbg, int nt, int n_chains, hipStream_t s) {
  unsigned long long tot[kPh];
  phase_totals(dbg, n_chains, s, tot);
  const double steps = (double)tot[kPh - 1];
  const char* nm[7] = {"copy+gen", "issue", "groups", "list", "wave0", "general", "traj"};
  fprintf(stderr, "[hyg backward phases NT=%d] cycles/step:", nt);
  double sum = 0;
  for (int k = 0; k < 7; ++k) {
    fprintf(stderr, " %s=%.0f", nm[k], tot[k] / steps);
    sum += tot[k] / steps;
  }
  fprintf(stderr, " total(+tail)=%.0f | groups/step=%.2f finite logits/group=%.1f", sum, tot[10] / steps,
          (double)(tot[11] & 0xffffffffull) / (tot[10] > 0 ? (double)tot[10] : 1.0));
  fprintf(stderr, " | wave0 split: entries=%.0f max=%.0f exp=%.0f scan=%.0f total=%.0f draw=%.0f\n", tot[12] / steps,
          tot[13] / steps, tot[14] / steps, tot[15] / steps, tot[16] / steps, tot[4] / steps);
}

static int launch_forward(const KernelPlan& p, const ModelRef& m, const ChainDev* chains_dev, int n_chains,
                          const double* E, uint8_t* ws, const hyg_tg_outputs& out, hipStream_t s, bool timed,
                          const TraceArg<true>* trace = nullptr) {
  if (p.status != HYG_OK) return p.status;
  if (p.k->mm != (m.table != nullptr) || p.k->trc != (trace != nullptr) || p.k->res) return HYG_EINVAL;
  if (hipFuncSetAttribute(p.k->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds) != hipSuccess)
    return HYG_EDEVICE;
  unsigned long long* dbg = p.k->phases ? phase_buffer(n_chains, s) : nullptr;
  if (timed) ev_record(1, false, s);
  p.k->launch({(unsigned)n_chains, p.lds, s, m, chains_dev, E, ws, out, p.lay, dbg, trace, nullptr});
  if (timed) ev_record(1, true, s);
  if (hipGetLastError() != hipSuccess) return HYG_EDEVICE;
  if (dbg) report_forward_phases(dbg, p.nt, n_chains, s);
  return HYG_OK;
}
static int launch_backward(const KernelPlan& p, const ModelRef& m, const ChainDev* chains_dev, int n_chains,
                           const double* E, uint8_t* ws, const hyg_tg_outputs& out, hipStream_t s, bool timed) {
  if (p.status != HYG_OK) return p.status;
  if (p.k->mm != (m.table != nullptr)) return HYG_EINVAL;
  if (hipFuncSetAttribute(p.k->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lay.total) != hipSuccess)
    return HYG_EDEVICE;
  unsigned long long* dbg = p.k->phases ? phase_buffer(n_chains, s) : nullptr;
  if (timed) ev_record(2, false, s);
  p.k->launch({(unsigned)n_chains, p.lay.total, s, m, chains_dev, E, ws, out, p.lay, dbg, nullptr, nullptr});
  if (timed) ev_record(2, true, s);
  if (dbg) report_backward_phases(dbg, p.nt, n_chains, s);
  return hipGetLastError() == hipSuccess ? HYG_OK : HYG_EDEVICE;
}

// One wave that sleeps about 0.1 ms (32 x s_sleep 127, ~8 k cycles each). It
// sits between the head's forward and its backward on the second stream so that
// the tail's forward, released by the same event on the launch stream, takes its
// CUs before the backward's workgroups fill them (see launch_chains).
__global__ void tg_dispatch_guard_kernel() {
  for (int i = 0; i < 32; ++i) __builtin_amdgcn_s_sleep(127);
}

namespace {
// The per-chain outputs of chains [c0, ...) of a launch; the per-site outputs
// are addressed through each chain's out_begin and need no offset.
hyg_tg_outputs outputs_from(const hyg_tg_outputs& o, const hyg_tg_consts& c, int c0) {
  hyg_tg_outputs r = o;
  r.status = o.status + c0;
  r.log_z = o.log_z + c0;
  if (o.final_log_weights) r.final_log_weights = o.final_log_weights + (size_t)c0 * c.Nmax;
  return r;
}
// The second stream and two events of a device for the tail overlap
// (created on first use, kept for the process).
struct TailAux {
  std::mutex mu;  // one split launch enqueued at a time (the events are shared)
  hipStream_t s = nullptr;
  hipEvent_t head_done = nullptr, bwd_done = nullptr;
  bool ok = false, tried = false;
};
TailAux* tail_aux() {
  static TailAux aux[32];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) return nullptr;
  TailAux& a = aux[dev];
  static std::mutex init_mu;
  std::lock_guard<std::mutex> lock(init_mu);
  if (!a.tried) {
    a.tried = true;
    a.ok = hipStreamCreateWithFlags(&a.s, hipStreamNonBlocking) == hipSuccess &&
           hipEventCreateWithFlags(&a.head_done, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&a.bwd_done, hipEventDisableTiming) == hipSuccess;
  }
  return a.ok ? &a : nullptr;
}
bool g_tail_overlap = true;  // hyg_tg_set_tail_overlap

// The round tables of a device's launches in rounds (forward_schedule): round
// 1's descriptors (the launch's with T = the chain's cut) and round 2's block
// entries, a few tens of KB, in a device buffer and a pinned host buffer that
// the library owns per device (created on first use, grown on demand, kept for
// the process). One launch fills and enqueues them at a time. The host waits
// only for the previous launch's copy out of the pinned buffer (`copied`); the
// device buffer is guarded on the device: the launch stream waits for the event
// behind the last kernel that read it (`read`) before the next copy into it.
// Only growing the buffers waits for that kernel on the host.
struct RoundTables {
  std::mutex mu;
  void* dev = nullptr;
  void* host = nullptr;
  size_t cap = 0;
  hipEvent_t copied = nullptr, read = nullptr;
  bool copy_pending = false, read_pending = false;
  bool reserve(size_t bytes) {  // (under mu)
    if (!copied && hipEventCreateWithFlags(&copied, hipEventDisableTiming) != hipSuccess) return false;
    if (!read && hipEventCreateWithFlags(&read, hipEventDisableTiming) != hipSuccess) return false;
    if (copy_pending && hipEventSynchronize(copied) != hipSuccess) return false;
    copy_pending = false;
    if (bytes <= cap) return true;
    if (read_pending && hipEventSynchronize(read) != hipSuccess) return false;
    read_pending = false;
    if (dev) (void)hipFree(dev);
    if (host) (void)hipHostFree(host);
    dev = host = nullptr;
    cap = 0;
    const size_t want = (bytes + 65535) / 65536 * 65536;
    if (hipMalloc(&dev, want) != hipSuccess || hipHostMalloc(&host, want, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      if (dev) (void)hipFree(dev);
      dev = host = nullptr;
      return false;
    }
    cap = want;
    return true;
  }
};
RoundTables* round_tables() {
  static RoundTables tabs[kMaxDevices];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return nullptr;
  return &tabs[dev];
}
constexpr int kNoRoundTables = 1;  // launch_forward_rounds: nothing enqueued, run the one launch
}  // namespace

// The forward of a launch in two rounds (forward_schedule; hd: the launch's
// descriptors on the host): round 1 is the launch's own kernel on descriptors
// cut short, round 2 the resuming build of the same shape on the launch's own
// descriptors, back to back on the launch stream. The kernel boundary is the
// only synchronisation. Round 1 leaves status, log Z and final weights of
// every chain; round 2 overwrites those of the chains it runs and skips a
// chain that failed in round 1, whose values are already the unsplit launch's.
static int launch_forward_rounds(const KernelPlan& p, const KernelRow* res, const ForwardRounds& fr, const ModelRef& m,
                                 const ChainDev* chains_dev, const ChainDev* hd, int n_chains, const double* E,
                                 uint8_t* ws, const hyg_tg_outputs& out, hipStream_t s) {
  RoundTables* rt = round_tables();
  if (!rt) return kNoRoundTables;  // (a device index past the table)
  if (!res->res || res->mm != (m.table != nullptr)) return HYG_EINVAL;
  if (hipFuncSetAttribute(res->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds) != hipSuccess)
    return HYG_EDEVICE;
  const size_t cd_bytes = sizeof(ChainDev) * (size_t)n_chains, n2 = fr.order2.size();
  std::lock_guard<std::mutex> lock(rt->mu);
  if (!rt->reserve(cd_bytes + sizeof(ResEntry) * n2)) return kNoRoundTables;  // (no memory for them)
  ChainDev* cd1 = (ChainDev*)rt->host;
  ResEntry* en = (ResEntry*)((uint8_t*)rt->host + cd_bytes);
  for (int i = 0; i < n_chains; ++i) {
    cd1[i] = hd[i];
    cd1[i].T = fr.cut[i];
  }
  for (size_t b = 0; b < n2; ++b) en[b] = ResEntry{fr.order2[b], fr.cut[fr.order2[b]]};
  // the previous launch's kernels (any stream) have read the device tables before this copy replaces them
  if (rt->read_pending && hipStreamWaitEvent(s, rt->read, 0) != hipSuccess) return HYG_EDEVICE;
  if (hipMemcpyAsync(rt->dev, rt->host, cd_bytes + sizeof(ResEntry) * n2, hipMemcpyHostToDevice, s) != hipSuccess)
    return HYG_EDEVICE;
  if (hipEventRecord(rt->copied, s) == hipSuccess) rt->copy_pending = true;
  else (void)hipStreamSynchronize(s);
  // (from here the stream reads the tables: every path records the event)
  ev_record(1, false, s);
  int rc = launch_forward(p, m, (const ChainDev*)rt->dev, n_chains, E, ws, out, s, false);
  if (rc == HYG_OK) {
    const ResArg<true> ra{(const ResEntry*)((const uint8_t*)rt->dev + cd_bytes)};
    res->launch({(unsigned)n2, p.lds, s, m, chains_dev, E, ws, out, p.lay, nullptr, nullptr, &ra});
    if (hipGetLastError() != hipSuccess) rc = HYG_EDEVICE;
  }
  ev_record(1, true, s);
  if (hipEventRecord(rt->read, s) == hipSuccess) rt->read_pending = true;
  else (void)hipStreamSynchronize(s);
  return rc;
}

void tg_set_tail_overlap(bool on) { g_tail_overlap = on; }

// The whole launch: forward of every chain, then the backward of every chain.
//
// Tail overlap. When the forward's LDS holds one chain per CU (the C5 shape)
// and the chains fill more than one round of CUs with a partial last round, the
// last round leaves most CUs idle for a full chain's latency (C5: 1 164 chains
// = four rounds of 256 and a fifth of 140, 52 of them full length). The
// launch is then split: the forward of the full rounds (the head, the first
// chains in launch order) and of the rest (the tail) run back to back on the
// launch stream, and the head's backward runs on a second stream as soon as
// the head's forward is done, on the CUs the tail's forward leaves free; the
// tail's backward follows its forward. Each chain's forward still precedes its
// backward, no chain's buffers are shared, and the widths are those of the
// whole launch, so the outputs are those of the unsplit launch (GPU test).
//
// A multi-model launch (md.table) is the same launch with the multi-model rows
// of the same plans: a split hands each part its own chains' descriptors
// (chains_dev + head), which carry each chain's model index.
static int launch_chains_of(const ModelRef& md, const hyg_tg_consts& c, const ChainDev* chains_dev, int n_chains,
                            const double* E, uint8_t* ws, const hyg_tg_outputs& out, void* stream,
                            const ChainDev* chains_host) {
  if (n_chains <= 0) return HYG_OK;
  hipStream_t s = (hipStream_t)stream;
  const bool mm = md.table != nullptr;
  const KernelPlan pf = plan(false, c, n_chains, mm), pb = plan(true, c, n_chains, mm);  // of the whole launch
  if (pf.status != HYG_OK) return pf.status;
  if (pb.status != HYG_OK) return pb.status;
  int head = n_chains;
  TailAux* aux = nullptr;
  if (g_tail_overlap && n_chains > device_cus() && n_chains % device_cus() != 0 && resident_per_cu(pf) == 1 &&
      (aux = tail_aux()) != nullptr)
    head = n_chains - n_chains % device_cus();
  if (head == n_chains) {
    // the forward in rounds, where the host knows the lengths and the schedule cuts them
    const int mode = chains_host ? forward_rounds_mode() : 0;
    const KernelRow* res = nullptr;
    if (mode > 0 && forward_splittable(pf, true)) {
      size_t nr = 0;
      const KernelRow* rows = res_rows(mm, &nr);
      for (size_t i = 0; i < nr && !res; ++i)
        if (rows[i].nt == pf.nt && rows[i].shape == pf.k->shape) res = &rows[i];
    }
    int rc = kNoRoundTables;
    ForwardRounds fr;
    if (res) {
      std::vector<int> T((size_t)n_chains);
      for (int i = 0; i < n_chains; ++i) T[i] = chains_host[i].T;
      // the schedule's own conditions first: only a launch they would cut pays the occupancy queries
      fr = forward_schedule(T.data(), n_chains, device_cus(), n_chains, mode, true);
      if (fr.rounds == 2) {
        KernelPlan pr = pf;  // (the occupancy of the resuming build)
        pr.k = res;
        const int resident = std::min(resident_per_cu(pf), resident_per_cu(pr));
        fr = forward_schedule(T.data(), n_chains, device_cus(), resident, mode, true);
      }
    }
    if (fr.rounds == 2) rc = launch_forward_rounds(pf, res, fr, md, chains_dev, chains_host, n_chains, E, ws, out, s);
    // (no tables for this device, or no memory for them: the one launch needs none)
    if (rc == kNoRoundTables) rc = launch_forward(pf, md, chains_dev, n_chains, E, ws, out, s, true);
    if (rc != HYG_OK) return rc;
    return launch_backward(pb, md, chains_dev, n_chains, E, ws, out, s, true);
  }
  const int tail = n_chains - head;
  const hyg_tg_outputs out_t = outputs_from(out, c, head);
  std::lock_guard<std::mutex> lock(aux->mu);
  ev_record(1, false, s);
  int rc = launch_forward(pf, md, chains_dev, head, E, ws, out, s, false);
  if (rc != HYG_OK) return rc;
  if (hipEventRecord(aux->head_done, s) != hipSuccess) return HYG_EDEVICE;
  rc = launch_forward(pf, md, chains_dev + head, tail, E, ws, out_t, s, false);
  if (rc != HYG_OK) return rc;
  ev_record(1, true, s);
  // From here the second stream holds work: every return path below makes the
  // launch stream wait for it, so the call's stream covers the whole launch
  // whatever fails.
  auto join = [&](int code) {
    const bool ok = hipEventRecord(aux->bwd_done, aux->s) == hipSuccess &&
                    hipStreamWaitEvent(s, aux->bwd_done, 0) == hipSuccess;
    if (code == HYG_OK && !ok) return (int)HYG_EDEVICE;
    if (!ok) (void)hipStreamSynchronize(aux->s);  // the events failed: drain the second stream instead
    return code;
  };
  if (hipStreamWaitEvent(aux->s, aux->head_done, 0) != hipSuccess) return join(HYG_EDEVICE);
  // The guard kernel is a scheduling heuristic, not a dependency: it only makes
  // the tail's forward (released by head_done on the launch stream) likely to
  // take its CUs before the head's backward fills them. The outputs do not
  // depend on which dispatch wins.
  hipLaunchKernelGGL(tg_dispatch_guard_kernel, dim3(1), dim3(64), 0, aux->s);
  ev_record(2, false, aux->s);
  rc = launch_backward(pb, md, chains_dev, head, E, ws, out, aux->s, false);
  if (rc != HYG_OK) return join(rc);
  rc = launch_backward(pb, md, chains_dev + head, tail, E, ws, out_t, s, false);
  rc = join(rc);
  if (rc != HYG_OK) return rc;
  ev_record(2, true, s);
  return hipGetLastError() == hipSuccess ? HYG_OK : HYG_EDEVICE;
}

int launch_chains(const ModelDev& md, const hyg_tg_consts& c, const ChainDev* chains_dev, int n_chains,
                  const double* E, uint8_t* ws, const hyg_tg_outputs& out, void* stream, const ChainDev* chains_host) {
  return launch_chains_of(ModelRef{md, nullptr}, c, chains_dev, n_chains, E, ws, out, stream, chains_host);
}
int launch_chains_multi(const ModelDev* models_dev, const hyg_tg_consts& c, const ChainDev* chains_dev, int n_chains,
                        const double* E, uint8_t* ws, const hyg_tg_outputs& out, void* stream,
                        const ChainDev* chains_host) {
  if (!models_dev) return HYG_EINVAL;
  return launch_chains_of(ModelRef{ModelDev{}, models_dev}, c, chains_dev, n_chains, E, ws, out, stream, chains_host);
}

// A forward-only launch: the forward of every chain in its REC = false build,
// which writes log Z, the final weights and the status and no history (ws
// holds the header and, for a forward_global_w shape, each chain's scratch at
// ChainDev::wg_offset). One kernel on the launch stream: no tail overlap, no
// second stream. The timing events stand around the forward; the backward's
// are marked unused.
static int launch_filter_of(const ModelRef& md, const hyg_tg_consts& c, const ChainDev* chains_dev, int n_chains,
                            const double* E, uint8_t* ws, const hyg_tg_outputs& out, void* stream,
                            const TraceArg<true>* trace = nullptr) {
  if (n_chains <= 0) return HYG_OK;
  const KernelPlan pf = plan(false, c, n_chains, md.table != nullptr, false, trace != nullptr);
  if (pf.status != HYG_OK) return pf.status;
  ev_unused(2);
  return launch_forward(pf, md, chains_dev, n_chains, E, ws, out, (hipStream_t)stream, true, trace);
}
int launch_filter(const ModelDev& md, const hyg_tg_consts& c, const ChainDev* chains_dev, int n_chains,
                  const double* E, uint8_t* ws, const hyg_tg_outputs& out, void* stream) {
  return launch_filter_of(ModelRef{md, nullptr}, c, chains_dev, n_chains, E, ws, out, stream);
}
int launch_filter_multi(const ModelDev* models_dev, const hyg_tg_consts& c, const ChainDev* chains_dev, int n_chains,
                        const double* E, uint8_t* ws, const hyg_tg_outputs& out, void* stream) {
  if (!models_dev) return HYG_EINVAL;
  return launch_filter_of(ModelRef{ModelDev{}, models_dev}, c, chains_dev, n_chains, E, ws, out, stream);
}
// A traced forward-only launch: launch_filter[_multi] in the TRC build of its
// kernel, which also writes rows out_begin + t of the trace arrays (device
// pointers, at least one of them non-null).
int launch_trace(const ModelDev& md, const hyg_tg_consts& c, const ChainDev* chains_dev, int n_chains, const double* E,
                 uint8_t* ws, const hyg_tg_outputs& out, const hyg_tg_trace& trace, void* stream) {
  const TraceArg<true> t{trace.log_z_t, trace.split_probs, trace.regime_probs};
  return launch_filter_of(ModelRef{md, nullptr}, c, chains_dev, n_chains, E, ws, out, stream, &t);
}
int launch_trace_multi(const ModelDev* models_dev, const hyg_tg_consts& c, const ChainDev* chains_dev, int n_chains,
                       const double* E, uint8_t* ws, const hyg_tg_outputs& out, const hyg_tg_trace& trace,
                       void* stream) {
  if (!models_dev) return HYG_EINVAL;
  const TraceArg<true> t{trace.log_z_t, trace.split_probs, trace.regime_probs};
  return launch_filter_of(ModelRef{ModelDev{}, models_dev}, c, chains_dev, n_chains, E, ws, out, stream, &t);
}
}  // namespace hyg
