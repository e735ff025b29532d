// tg_dev.h -- what the two-group chain kernels (tg_kernels.hip) share below a
// step: wave priorities, sort keys, the model constants in LDS (ConstLds), the
// transition density and the hazard rows, the LDS layout (Shared, Lay,
// make_layout: the host plans with it too), list_walk and the emission ring.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/hyg_arith.h"
#include "tg_common.h"
#include "hyg_dev.h"  // wave / block primitives (DPP, readlane, LDS-only barriers)

namespace hyg {

enum { MODE_KEEP = 0, MODE_OPTIMAL = 1, MODE_UNBIASED = 2, MODE_INIT = 3 };

// Wave priority of the single-wave serial sections (the K loop + systematic
// draws, the backward's one-wave categorical): while one wave of a chain works
// alone, the others wait at a barrier, so its issue slots are the chain's
// critical path; the other chains sharing the CU fill the gaps.
#ifndef HYG_SERIAL_PRIO
#define HYG_SERIAL_PRIO 1
#endif
// `pb` is the wave's base priority (0 where priorities do not rotate, below).
__device__ __forceinline__ void set_prio(int p) {  // p wave-uniform; s_setprio takes an immediate
  switch (p) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
  }
}
__device__ __forceinline__ void serial_begin(int pb = 0) {
  if constexpr (HYG_SERIAL_PRIO > 0) set_prio((pb & 3) + HYG_SERIAL_PRIO);
}
__device__ __forceinline__ void serial_end(int pb = 0) {
  if constexpr (HYG_SERIAL_PRIO > 0) set_prio(pb & 3);
}

// Rotating base priorities (the 256-thread forward, up to three chains per CU).
// A SIMD issues by priority, then by age, so at equal priority the chains of a CU
// advance at fixed, unequal rates for the whole launch: measured at C3, 12.8,
// 14.7 and 17.4 us per step for the first, second and third workgroup a CU
// received, whether or not there is a third, and the launch ends with the third
// (profiles/r08_*). Each wave therefore takes a base priority 0 .. 2 from its
// wave slot in the SIMD (HW_ID.WAVE_ID: 0, 1, 2 in dispatch order, so the waves
// that compete on one SIMD hold different slots) and an epoch of the constant
// 100 MHz clock that all of them read alike: the six orders of three priorities
// in turn, so every pair of slots leads half of the time and every slot of
// three holds each rank a third of the time. Priorities change when a wave
// issues, never what it computes. The backward keeps one priority: with the
// same rotation its C3 launch took 660 ms against 614 (profiles/r08_*).
#ifndef HYG_PRIO_ROT
#define HYG_PRIO_ROT 1  // (A/B builds: -DHYG_PRIO_ROT=0)
#endif
constexpr int kPrioEpochShift = 15;  // 2^15 ticks of 10 ns: 0.33 ms, about 25 steps
constexpr int kPrioEvery = 8;        // steps between two looks at the clock
__device__ __forceinline__ int wave_slot3() {
  unsigned s;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID, 0, 4)" : "=s"(s));
  return (int)(s % 3u);
}
constexpr unsigned long long prio_orders() {  // 2 bits per (order, slot)
  const int o[6][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {2, 1, 0}, {1, 0, 2}};
  unsigned long long v = 0;
  for (int e = 0; e < 6; ++e)
    for (int s = 0; s < 3; ++s) v |= (unsigned long long)o[e][s] << (2 * (3 * e + s));
  return v;
}
__host__ __device__ constexpr int prio_base_at(unsigned long long ticks, int slot3) {  // the base priority at a clock value
  const unsigned e = (unsigned)(ticks >> kPrioEpochShift) % 6u;
  return (int)((prio_orders() >> (2 * (3 * e + (unsigned)slot3))) & 3ull);
}
__device__ __forceinline__ int prio_base(int slot3) { return prio_base_at(__builtin_amdgcn_s_memrealtime(), slot3); }


// sort key: ascending key == descending f32 value, ties by ascending index
__device__ __forceinline__ uint64_t sort_key(float x, int idx) {
  uint32_t u = hyg_f32_bits(x);
  if (u == 0x80000000u) u = 0;
  const uint32_t ord = (u >> 31) ? ~u : (u | 0x80000000u);
  return ((uint64_t)(~ord) << 32) | (uint32_t)idx;
}
__device__ __forceinline__ float key_value(uint64_t k) {
  const uint32_t ord = ~(uint32_t)(k >> 32);
  const uint32_t u = (ord & 0x80000000u) ? (ord & 0x7fffffffu) : ~ord;
  return hyg_bits_f32(u);
}
__device__ __forceinline__ int key_index(uint64_t k) { return (int)(uint32_t)k; }

// n / d for 0 <= n < 2^22, 1 <= d <= 2^22, via a float reciprocal + fixup
__device__ __forceinline__ int fdiv(int n, int d, float rd) {
  int q = (int)((float)n * rd);
  if (q * d > n) --q;
  if ((q + 1) * d <= n) ++q;
  return q;
}

// hyg_exp_fix100(x[i]) (= hyg_fix100(hyg_exp(x[i])), include/hyg_arith.h) for R
// values at once, written statement by statement across the values: the same
// operations in the same order per value (so the same bits), but the R
// dependent f64 chains sit side by side in the instruction stream. Written as
// one function per value, the compiler schedules the chains one after another
// and every f64 operation waits for its predecessor's result. The image is
// formed from the polynomial value and the exponent by shifts (no scaling by
// 2^k, no float floors).
template <int R>
__device__ __forceinline__ void exp_fix100_lockstep(const double (&x)[R], hyg_u128 (&out)[R]) {
  double xc[R], kd[R], r[R], r2[R], r4[R], r8[R], p[R];
  int k[R];
#pragma unroll
  for (int i = 0; i < R; ++i) xc[i] = __builtin_fmin(__builtin_fmax(x[i], -746.0), 710.0);
#pragma unroll
  for (int i = 0; i < R; ++i) kd[i] = __builtin_floor(xc[i] * HYG_INV_LN2 + 0.5);
#pragma unroll
  for (int i = 0; i < R; ++i) {
    k[i] = (int)kd[i];
    const double hi = xc[i] - kd[i] * HYG_LN2_HI;
    r[i] = __builtin_fma(-kd[i], HYG_LN2_LO, hi);
  }
#pragma unroll
  for (int i = 0; i < R; ++i) r2[i] = r[i] * r[i];
#pragma unroll
  for (int i = 0; i < R; ++i) r4[i] = r2[i] * r2[i];
#pragma unroll
  for (int i = 0; i < R; ++i) r8[i] = r4[i] * r4[i];
#pragma unroll
  for (int i = 0; i < R; ++i) {  // hyg__exp_poly, statement by statement
    const double q0 = __builtin_fma(1.0, r[i], 1.0);
    const double q1 = __builtin_fma(1.6666666666666665741e-01, r[i], 0.5);
    const double q2 = __builtin_fma(8.3333333333333332177e-03, r[i], 4.1666666666666664354e-02);
    const double q3 = __builtin_fma(1.9841269841269841253e-04, r[i], 1.3888888888888888889e-03);
    const double q4 = __builtin_fma(2.7557319223985890653e-06, r[i], 2.4801587301587301566e-05);
    const double q5 = __builtin_fma(2.5052108385441718775e-08, r[i], 2.7557319223985890653e-07);
    const double q6 = __builtin_fma(1.6059043836821614599e-10, r[i], 2.0876756987868098979e-09);
    const double s0 = __builtin_fma(q1, r2[i], q0);
    const double s1 = __builtin_fma(q3, r2[i], q2);
    const double s2 = __builtin_fma(q5, r2[i], q4);
    const double u0 = __builtin_fma(s1, r4[i], s0);
    const double u1 = __builtin_fma(q6, r4[i], s2);
    p[i] = __builtin_fma(u1, r8[i], u0);
  }
#pragma unroll
  for (int i = 0; i < R; ++i) out[i] = hyg_exp_fix100_pk(p[i], k[i], x[i]);
}

// --------------------------------------------------------------- model
struct Hz4 {
  double lrc, l1c, lrk, l1k;  // log rho / log(1-rho) of control (d_c, r_c) and case (d_k, r_k)
};

struct ConstLds {  // model constants staged in LDS
  double lPm[4];
  double lU1, lU2, log_M;
  double2 hz1[2][HYG_KMAX];  // hazard rows at d = 1
  float logMa[64];           // (float)log(M - a) for a < min(M, 64) (resampling_functions.py:13)
  int u, K;
  double lPc[HYG_KMAX * HYG_KMAX];  // last: only K*K entries are allocated (const_lds_bytes)
};
__host__ __device__ inline size_t const_lds_bytes(int K) {
  return sizeof(ConstLds) - sizeof(double) * (size_t)(HYG_KMAX * HYG_KMAX - K * K);
}

__device__ __forceinline__ double2 hz_at(const ModelDev& md, int K, int g, int r, int d) {
  d = d < 0 ? 0 : (d >= md.dcap ? md.dcap - 1 : d);
  return *(const double2*)(md.hz + ((size_t)(g * K + r) * md.dcap + d) * 2);
}

__device__ __forceinline__ void load_consts(ConstLds& cl, const hyg_tg_consts* __restrict__ c, const ModelDev& md) {
  const int K = c->K;
  for (int i = threadIdx.x; i < K * K; i += blockDim.x) cl.lPc[i] = c->lPc[i];
  if (threadIdx.x < 4) cl.lPm[threadIdx.x] = c->lPm[threadIdx.x];
  if (threadIdx.x < 2 * K) {
    const int g = threadIdx.x / K, r = threadIdx.x - g * K;
    cl.hz1[g][r] = hz_at(md, K, g, r, 1);
  }
  if (threadIdx.x < 64 && threadIdx.x < c->M) cl.logMa[threadIdx.x] = hyg_logf((float)(c->M - (int)threadIdx.x));
  if (threadIdx.x == 0) {
    cl.lU1 = c->lU1;
    cl.lU2 = c->lU2;
    cl.log_M = c->log_M;
    cl.u = c->u;
    cl.K = K;
  }
}

// log f_t(next | prev), t >= 1 (case_control_regime_model.py:80-193,
// case_control_distributions.py:138-151, 246-291); h = hazard of prev.
// Same branch structure and addition order as oracle/tg_oracle.c:tg_trans.
__device__ __forceinline__ double tg_trans_sel(double lPm_j, double lpc, double lU1, double lU2, int u, int m,
                                               int dc, int rc, int dk, int rk, uint64_t next, const Hz4& h);
__device__ __forceinline__ double tg_trans(const ConstLds& cl, int K, uint64_t prev, uint64_t next, const Hz4& h) {
  const int m = hyg_st_m(prev), dc = hyg_st_dc(prev), rc = hyg_st_rc(prev), dk = hyg_st_dk(prev),
            rk = hyg_st_rk(prev);
  const int m2 = hyg_st_m(next), rc2 = hyg_st_rc(next);
  return tg_trans_sel(cl.lPm[m * 2 + m2], cl.lPc[rc * K + rc2], cl.lU1, cl.lU2, cl.u, m, dc, rc, dk, rk, next, h);
}

// The case analysis of tg_trans as selects: every operand is loaded and every
// candidate sum formed unconditionally (no divergent branches, no loads under
// a lane condition); the selected value is the same expression, so results
// are bit-identical.
__device__ __forceinline__ double tg_trans_sel(double lPm_j, double lpc, double lU1, double lU2, int u, int m,
                                               int dc, int rc, int dk, int rk, uint64_t next, const Hz4& h) {
  const double NINF = HYG_NINF;
  const int m2 = hyg_st_m(next), dc2 = hyg_st_dc(next), rc2 = hyg_st_rc(next), dk2 = hyg_st_dk(next),
            rk2 = hyg_st_rk(next);
  const double lm = ((dk < dc ? dk : dc) >= u) ? lPm_j : ((m2 == m) ? 0.0 : NINF);
  const double lc_cp = h.lrc + lpc;
  const double lc = (dc2 == 1) ? lc_cp : ((dc2 == dc + 1 && rc2 == rc) ? h.l1c : NINF);
  const double v1 = (rk2 == rc2 && dk2 == dc2) ? 0.0 : NINF;
  const double v23 = (dk2 == 1 && rk2 != rc2) ? lU1 : NINF;
  const double lk_cp = h.lrk + ((rc2 == rk) ? lU1 : lU2);
  const double v4a = (rk2 != rc2 && rk2 != rk) ? lk_cp : NINF;
  const double v4b = (dk2 == dk + 1 && rk2 == rk) ? h.l1k : NINF;
  const double v4 = (dk2 == 1) ? v4a : v4b;
  const double lk = (m2 == 1) ? v1 : ((m == 1 && dc2 != 1) ? v23 : ((rc2 == rk && m == 0) ? v23 : v4));
  return (lm + lc) + lk;
}

// proposal slot s of ancestor a (case_control_proposal_mappings.py:11-134)
__device__ __forceinline__ uint64_t tg_xi(int K, uint64_t a, int s) {
  const int m = hyg_st_m(a), dc = hyg_st_dc(a), rc = hyg_st_rc(a), dk = hyg_st_dk(a), rk = hyg_st_rk(a);
  if (s == 0) return hyg_st_pack(m, dc + 1, rc, dk + 1, rk);
  if (s < K) {
    const int r = (s - 1 < rk) ? s - 1 : s;
    return hyg_st_pack(0, 1, r, dk + 1, rk);
  }
  if (s < 2 * K - 1) {
    const int q = s - K;
    const int r = (q < rc) ? q : q + 1;
    return hyg_st_pack(0, dc + 1, rc, 1, r);
  }
  if (s == 2 * K - 1) {
    const int d = (m == 0) ? dc + 1 : 0;
    return hyg_st_pack(1, d, rc, d, rc);
  }
  const int j = s - 2 * K, i = j / K, jj = j - i * K;
  return hyg_st_pack(i == jj, 1, i, 1, jj);
}
__device__ __forceinline__ uint64_t init_state(int K, int n) {
  const int i = n / K, j = n - (n / K) * K;
  return hyg_st_pack(i == j, 1, i, 1, j);
}

// Hazard rows a child may need, prefetched per ancestor: control at
// (d_c + 1, r_c), case at (d_k + 1, r_k), case at (d_c + 1, r_c) (merge slot).
struct Pf3 {
  double2 c1, k1, kc;
};
__device__ __forceinline__ Pf3 prefetch_rows(const ModelDev& md, int K, uint64_t a) {
  Pf3 p;
  const int dc = hyg_st_dc(a), rc = hyg_st_rc(a);
  p.c1 = hz_at(md, K, 0, rc, dc + 1);
  p.k1 = hz_at(md, K, 1, hyg_st_rk(a), hyg_st_dk(a) + 1);
  p.kc = hz_at(md, K, 1, rc, dc + 1);
  return p;
}
// Hazards of the child in slot s of ancestor a (the rows of the child's own
// durations/regimes), from the ancestor's prefetched rows and the d = 1 rows.
__device__ __forceinline__ Hz4 child_hz(const ConstLds& cl, int K, uint64_t a, int s, const Pf3& p,
                                        const ModelDev& md) {
  Hz4 h;
  const uint64_t x = tg_xi(K, a, s);
  // s == 0: both durations continue; s < K: control changes; s < 2K-1: case
  // changes; s == 2K-1 with m = 0: merge (case continues on the control row);
  // m = 1 there: the merge slot's child (1, 0, r, 0, r) has weight -inf, is
  // never resampled and never becomes an ancestor, so its hazards are unused.
  // Value selects (a select of addresses would put p in scratch memory).
  const double2 h1c = cl.hz1[0][hyg_st_rc(x)], h1k = cl.hz1[1][hyg_st_rk(x)];
  const bool merge = (s == 2 * K - 1) && hyg_st_m(a) == 0;
  const bool c_cont = s == 0 || (s >= K && s < 2 * K - 1) || merge;
  const bool k_cont = s < K;
  h.lrc = c_cont ? p.c1.x : h1c.x;
  h.l1c = c_cont ? p.c1.y : h1c.y;
  h.lrk = merge ? p.kc.x : (k_cont ? p.k1.x : h1k.x);
  h.l1k = merge ? p.kc.y : (k_cont ? p.k1.y : h1k.y);
  return h;
}

// tg_xi + child_hz without divergent branches (slot s varies per lane in
// the gather): every slot type's child is formed and the right one selected.
__device__ __forceinline__ uint64_t tg_xi_hz_sel(const ConstLds& cl, int K, float rK, uint64_t a, int s,
                                                 const Pf3& p, Hz4* hout) {
  const int m = hyg_st_m(a), dc = hyg_st_dc(a), rc = hyg_st_rc(a), dk = hyg_st_dk(a), rk = hyg_st_rk(a);
  const int rB = (s - 1 < rk) ? s - 1 : s;
  const int qq = s - K, rC = (qq < rc) ? qq : qq + 1;
  const int dD = (m == 0) ? dc + 1 : 0;
  const int j = s - 2 * K;
  int i = (int)((float)(j > 0 ? j : 0) * rK);
  if (i * K > j) --i;
  if ((i + 1) * K <= j) ++i;
  const int jj = j - i * K;
  const bool tA = s == 0, tB = s < K, tC = s < 2 * K - 1, tD = s == 2 * K - 1;
  int xm, xdc, xrc, xdk, xrk;
  if (tA) { xm = m; xdc = dc + 1; xrc = rc; xdk = dk + 1; xrk = rk; }
  else if (tB) { xm = 0; xdc = 1; xrc = rB; xdk = dk + 1; xrk = rk; }
  else if (tC) { xm = 0; xdc = dc + 1; xrc = rc; xdk = 1; xrk = rC; }
  else if (tD) { xm = 1; xdc = dD; xrc = rc; xdk = dD; xrk = rc; }
  else { xm = (i == jj); xdc = 1; xrc = i; xdk = 1; xrk = jj; }
  // hazard rows: prefetched rows where the duration continues, d = 1 rows at a change
  const bool c_cont = tA || (!tB && tC) || (tD && m == 0);
  const bool k_cont = tA || (tB && !tA);
  // (value selects: a select of the address would put p in scratch memory)
  const double2 h1c = cl.hz1[0][xrc], h1k = cl.hz1[1][xrk];
  const bool kc = tD && m == 0;
  hout->lrc = c_cont ? p.c1.x : h1c.x;
  hout->l1c = c_cont ? p.c1.y : h1c.y;
  hout->lrk = kc ? p.kc.x : (k_cont ? p.k1.x : h1k.x);
  hout->l1k = kc ? p.kc.y : (k_cont ? p.k1.y : h1k.y);
  return hyg_st_pack(xm, xdc, xrc, xdk, xrk);
}

// ------------------------------------------------------------ LDS layout
constexpr int kPh = 36;  // diagnostic phase timers (last entry: timestamp / step count)

struct Shared {  // broadcast scalars of one workgroup
  double mx, logS;
  float c_new, log_c;
  int cnt, n_sig, Kk, status, r_ph, ng, fast;
  float Unext;  // systematic-resampling uniform of the next step, drawn during the gather
  unsigned sig_ctr;
  hyg_u192 R, preK;
  int segc[16];  // backward: finite logits per reachable slot (segment list)
  unsigned long long ph[kPh];
};

__host__ __device__ inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
__host__ __device__ inline int next_pow2(int x) {
  int p = 1;
  while (p < x) p <<= 1;
  return p;
}

constexpr int kBuckets = 512;  // counting-sort buckets of the resampling sort (sqrt-spaced in -lw)
constexpr int kNCut = 8;       // log-weight cutoffs of the top-set resampling path
// candidate-list entries per lane per chunk (lse / top-set gather): ~900 list
// entries at C3 are ~3.5 per lane at 256 threads, under one at 1024
#ifndef HYG_LR256
#define HYG_LR256 4
#endif
#ifndef HYG_LR512
#define HYG_LR512 2
#endif
template <int NT>
constexpr int kLRof = NT >= 768 ? 2 : (NT >= 512 ? HYG_LR512 : HYG_LR256);
// The 256-thread builds with their weights in LDS (three chains per CU, where
// a VALU instruction saved is time saved) walk a list per 64 entries: a list of
// 230 entries pays for 4 x 64 slots of the fully unrolled chunk, one of 260
// for 5 instead of 8 (Lay::list_fine, hyg_tg_set_fine_list_walk).
template <int NT, bool GW>
constexpr bool kFineLists = NT == 256 && !GW;
template <int R>
struct IntC {
  static constexpr int value = R;
};
// body(IntC<R>, b) over the entries [0, n) of a wave's list, R * 64 of them
// from entry b on: whole chunks of kLR * 64 and, with `fine` (wave-uniform),
// the rest in steps of 128 and 64 entries instead of one more whole chunk. Per
// entry the body does the same whatever R is; its last sub-chunk may be partial.
template <int kLR, class Body>
__device__ __forceinline__ void list_walk(int n, bool fine, Body body) {
  static_assert(kLR == 4 || kLR == 2 || kLR == 1, "the rest of a chunk: 128 and 64 entries");
  const int nsub = (n + 63) >> 6;  // sub-chunks of 64 entries
  const int full = fine ? nsub / kLR * (64 * kLR) : n;
  int b = 0;
  for (; b < full; b += 64 * kLR) body(IntC<kLR>{}, b);
  if (fine) {  // uniform; 0 .. kLR - 1 sub-chunks left
    const int rem = nsub - (b >> 6);
    if constexpr (kLR > 2) {
      if (rem & 2) {
        body(IntC<2>{}, b);
        b += 128;
      }
    }
    if constexpr (kLR > 1) {
      if (rem & 1) body(IntC<1>{}, b);
    }
  }
}
// waves that sort the top set A: at most 256 keys (one per lane of 4 waves)
// whatever the workgroup size, so a 512- or 1024-thread chain sorts no more
// keys than a 256-thread one. (Where its scratch fits, the top-set path ends
// in top_set_finish1, the latency-shaped finish.)
template <int NT>
constexpr int kSortWaves = (NT / 64 < 4) ? NT / 64 : 4;

struct Lay {  // byte offsets into the dynamic LDS (32-bit: one SGPR each in the kernels)
  uint32_t W, L, keys, bcnt, bpos, pre64, part, cp, pst, pw, phz, pf, ering, cl, parents, X, grp, gst, rb, xo, red,
      sh, uring, total;
  uint32_t bcnt_bytes;
  int npad, nkeys, nt;
  int topset_r;  // keys per lane of the top-set sort: A holds <= 64 * topset_r per wave
  int lcap;      // backward: doubles of the list / logit area at W (Nmax, or the lists alone with gw)
  int gather_w;  // forward: sorted positions of the top set gathered ahead (hyg_tg_set_gather_window; 0: none)
  int prio_rot;  // forward at 256 threads: rotating base priorities (hyg_tg_set_priority_rotation; 0: none)
  int list_fine;  // forward at 256 threads, weights in LDS: lists walked per 64 entries (hyg_tg_set_fine_list_walk; 0: whole chunks)
};

// The backward's list area without the full-N weights (gw): the segment lists
// (16 slots x 64 logits, then 64 u128 masses and 64 indices), or an appended
// list of up to 4 (NT + 1) logits (its indices in the cp area), or 64 logits
// and their masses: doubles.
__host__ __device__ constexpr int bwd_list_doubles(int NT) {
  return (64 * 16 + 128 + 32) > 4 * (NT + 1) ? (64 * 16 + 128 + 32) : 4 * (NT + 1);
}

// The forward's sort-key area: Nmax keys, or the (NT+1) x u128 prefix array of
// the keep / unbiased-fallback paths where that is larger: bytes.
__host__ __device__ inline size_t fwd_keys_bytes(int Nmax, int NT) {
  size_t kb = sizeof(uint64_t) * (size_t)Nmax;
  if (kb < sizeof(hyg_u128) * (size_t)(NT + 1)) kb = sizeof(hyg_u128) * (size_t)(NT + 1);
  return kb;
}
// The forward's global scratch with gw: the weights, then the key area (Lay::W
// and Lay::keys are then byte offsets into it): bytes.
__host__ __device__ inline size_t fwd_scratch_bytes(int Nmax, int NT) {
  return align_up(sizeof(double) * (size_t)Nmax, 16) + fwd_keys_bytes(Nmax, NT);
}

// gw: the full-N arrays live in the chain's global scratch and cost no LDS:
// the backward's weights (its W area then holds the lists alone), the forward's
// weights and keys.
__host__ __device__ inline Lay make_layout(int K, int M, int B, int Nmax, int NT, bool backward, bool gw = false) {
  // Sized for 3 workgroups per CU at K = 6, M = 50, NT = 256 (<= 53 KiB each).
  Lay l{};
  l.nt = NT;
  l.topset_r = 1;
  l.npad = Nmax;
  l.lcap = (backward && gw && bwd_list_doubles(NT) < Nmax) ? bwd_list_doubles(NT) : Nmax;
  size_t o = 0;
  if (!backward && gw) {
    l.W = 0;
    l.keys = (uint32_t)align_up(sizeof(double) * (size_t)Nmax, 16);
    l.nkeys = (int)(fwd_keys_bytes(Nmax, NT) / sizeof(uint64_t));
  } else {
    l.W = o; o = align_up(o + sizeof(double) * (backward ? l.lcap : l.npad), 16);
  }
  if (backward) {
    // the backward's list / logit area is the weight area: the list path
    // builds no weights and the general path turns the weights into logits
    // in place
    l.L = l.W;
    l.cp = o; o = align_up(o + sizeof(hyg_u128) * (NT + 1), 16);
  } else {
    // sort keys; the unbiased fallback reuses them as its (NT+1) x u128 prefix array
    if (!gw) {
      const size_t kb = fwd_keys_bytes(Nmax, NT);
      l.nkeys = (int)(kb / sizeof(uint64_t));
      l.keys = o; o = align_up(o + kb, 16);
    }
    // bucket counts / positions; the systematic thresholds (M x u192) reuse them
    size_t bb = sizeof(int) * 2 * kBuckets;
    if (bb < sizeof(hyg_u192) * (size_t)M) bb = sizeof(hyg_u192) * (size_t)M;
    l.bcnt = o;
    l.bpos = o + sizeof(int) * kBuckets;
    l.bcnt_bytes = bb;
    o = align_up(o + bb, 16);
    // the fallback's prefix of the first min(M, 64) sorted positions: written
    // after the counting sort's last use of the bucket area, last read before
    // the systematic thresholds are written there (a barrier apart)
    l.pre64 = l.bcnt;
    // per-wave partials of the top-set resampling path (counts per cutoff, mass)
    l.part = o; o = align_up(o + (sizeof(int) * kNCut + sizeof(hyg_u192)) * (NT / 64), 16);
  }
  // the ancestors of the current step, two buffers: the forward gathers the
  // next step's ancestors into the other buffer while this step's are read;
  // the backward holds record t in buffer t & 1 while record t-1 is stored
  // into the other. (The forward's hazard-row prefetch pf is written after
  // the weights, which do not read it: one buffer.)
  l.pst = o; o = align_up(o + sizeof(uint64_t) * M * 2, 16);
  l.pw = o; o = align_up(o + sizeof(double) * M * 2, 16);
  l.phz = o; o = align_up(o + sizeof(Hz4) * M * 2, 16);
  l.pf = o; o = align_up(o + sizeof(Pf3) * M * (backward ? 2 : 1), 16);
  l.ering = o; o = align_up(o + sizeof(double) * 2 * kEBlock * 2 * K, 16);
  l.cl = o; o = align_up(o + const_lds_bytes(K), 16);
  l.parents = o; o = align_up(o + sizeof(int) * (M > B ? M : B), 16);
  if (backward) {
    l.X = o; o = align_up(o + sizeof(uint64_t) * B, 16);
    l.grp = o; o = align_up(o + sizeof(int) * B, 16);
    l.gst = o; o = align_up(o + sizeof(uint64_t) * B, 16);
    l.rb = o; o = align_up(o + 2 * sizeof(uint64_t) * ((B + 3) / 4) * 4, 16);  // draw bits, two steps
    l.xo = o; o = align_up(o + 2 * sizeof(uint64_t) * B, 16);  // sampled states of two steps (deferred outputs)
  }
  l.red = o; o = align_up(o + 2 * 32 * (NT / 64), 16);  // two slots: the step's log-sum-exp has its own
  l.sh = o; o = align_up(o + sizeof(Shared), 16);
  // the forward's systematic uniforms of the next 64 steps, drawn 64 at a time
  // (NT >= 512: one chain per CU); 32 at 256 threads, whose three chains per CU
  // leave the layout ~240 B of LDS
  l.uring = o;
  if (!backward && NT >= 256) o = align_up(o + sizeof(float) * (NT >= 512 ? 64 : 32), 16);
  l.total = o;
  return l;
}

// ---------------------------------------------------------- shared steps
// Workgroup barrier behind which the particle arrays (weights, keys, prefix
// arrays) are handed between threads. In LDS that is the LDS-only barrier; a
// GW instantiation keeps them in global memory, where the hand-off needs a full
// workgroup fence (__syncthreads: a release of every outstanding store).
template <bool GW>
__device__ __forceinline__ void part_barrier() {
  if constexpr (GW) __syncthreads();
  else lds_barrier();
}

// Emission rows live in a 2 x kEBlock ring: row t at ring[((t/EB)&1)*EB + t%EB].
__device__ __forceinline__ void load_eblock(double* ering, const double* __restrict__ Ech, int bi, int T, int K2,
                                            int NT) {
  const int t0 = bi * kEBlock;
  if (t0 >= T) return;
  const int rows = (T - t0) < kEBlock ? (T - t0) : kEBlock;
  double* dst = ering + (size_t)(bi & 1) * kEBlock * K2;
  for (int i = threadIdx.x; i < rows * K2; i += NT) dst[i] = Ech[(size_t)t0 * K2 + i];
}
__device__ __forceinline__ const double* erow(const double* ering, int t, int K2) {
  return ering + ((size_t)((t / kEBlock) & 1) * kEBlock + (t % kEBlock)) * K2;
}

// Weight of the child in slot s of ancestor a at a step t >= 1, from the
// ancestors (pst, pw, phz) and the step scalars (_filter_one_step :235-270).
__device__ __forceinline__ double weight_at(const ConstLds& cl, int K, int a, int s, int mode, float log_c,
                                            double lse, const uint64_t* pst, const double* pw, const Hz4* phz,
                                            const double* Et) {
  const uint64_t par = pst[a];
  const uint64_t x = tg_xi(K, par, s);
  const double tr = tg_trans(cl, K, par, x, phz[a]);
  if (!hyg_isfinite(tr)) return HYG_NINF;
  const double lg = tr + (Et[hyg_st_rc(x)] + Et[K + hyg_st_rk(x)]);
  const double pa = pw[a];
  if (mode == MODE_KEEP) return pa + lg;
  if (mode == MODE_UNBIASED) return (-cl.log_M + lse) + lg;
  const double v = (double)log_c + (pa - lse);
  return (pa + lg) - (v < 0.0 ? v : 0.0);
}
// Weight of particle n = s * np + a.
__device__ __forceinline__ double weight_one(const ConstLds& cl, int K, int n, int np, int mode, float log_c,
                                             double lse, const uint64_t* pst, const double* pw, const Hz4* phz,
                                             const double* Et) {
  const int s = fdiv(n, np, 1.0f / (float)np), a = n - s * np;
  return weight_at(cl, K, a, s, mode, log_c, lse, pst, pw, phz, Et);
}

}  // namespace hyg
