// tg_forward.h -- tg_forward_kernel, the particle filter of the two-group
// chain kernels, behind what its arguments are made of: a chain's model
// (ModelArg, model_of), ResArg, TraceArg and the trace helpers.
#pragma once

#include "tg_resample.h"

namespace hyg {

// The model argument of a chain kernel: the launch's one model by value, or
// (MM, a multi-model launch) the device table of the launch's models, of which
// the workgroup takes the entry its chain names in ChainDev::pad.
template <bool MM>
struct ModelArgOf { using type = ModelDev; };
template <>
struct ModelArgOf<true> { using type = const ModelDev*; };
template <bool MM>
using ModelArg = typename ModelArgOf<MM>::type;
__device__ __forceinline__ ModelDev model_of(const ModelDev& md, const ChainDev*, unsigned) { return md; }
// A pointer read from the table is a generic one to the compiler, which would
// address the model's tables with flat loads (no scalar loads of the constants,
// LDS-counter waits on the step loop's hazard rows); as kernel arguments they
// are known global, so say that here as well (through the integer value: the
// compiler folds a generic -> global -> generic pointer cast away).
template <typename T>
__device__ __forceinline__ const T* global_ptr(const T* p) {
  return (const T*)(const __attribute__((address_space(1))) T*)(uintptr_t)p;
}
__device__ __forceinline__ ModelDev model_of(const ModelDev* __restrict__ table, const ChainDev* __restrict__ chains,
                                             unsigned chain) {
  ModelDev md = table[chains[chain].pad];
  md.consts = global_ptr(md.consts);
  md.hz = global_ptr(md.hz);
  md.lf = global_ptr(md.lf);
  md.lg = global_ptr(md.lg);
  md.cst = global_ptr(md.cst);
  md.bbt = global_ptr(md.bbt);
  return md;
}

// ---- resuming builds (RES, tg_kernels_res.hip)
// What block b of a resuming launch runs: a chain of the launch's descriptors
// and the step its loop starts at. The kernel argument is nothing, or (RES) the
// device array of the grid's entries.
struct ResEntry {
  int32_t chain, t_begin;
};
template <bool RES>
struct ResArg {};
template <>
struct ResArg<true> {
  const ResEntry* __restrict__ entries;
};

// ---- traced forward-only builds (TRC, tg_kernels_trc.hip)
// The trace argument of the forward kernel: nothing, or (TRC) the three per-site
// arrays of a traced launch (device pointers, any of them null), row
// ChainDev::out_begin + t of which the chain writes for every site t.
template <bool TRC>
struct TraceArg {};
template <>
struct TraceArg<true> {
  double* log_z_t;      // [rows]      log Z of the chain's first t + 1 sites
  float* split_probs;   // [rows]      P(merged_t = 0 | y_0..t)
  float* regime_probs;  // [rows][2K]  P(regime_t = r | y_0..t), control first
};
// The class sums of a traced build: 1 + 2K exact u128 sums of F = 100 masses
// (merged == 0, control regime r, case regime r). Up to K = 8 (272 B) they live
// in the phase-timer accumulators Shared::ph (288 B), which only a phase-timer
// build uses and a traced build never is: the traced launch then has the LDS
// of the untraced one, to the byte (the 256-thread pipeline layout is 112 B
// under the 42 allocation granules of 1 280 B that three chains per CU allow:
// 208 B more would leave two). Beyond K = 8 they stand behind the chain's LDS
// layout, at Lay::total, which stays as it is (trace_bins_extra more bytes of
// dynamic LDS): those shapes hold one chain per CU, or keep their particle
// arrays in global memory, and still hold as many chains.
__host__ __device__ inline size_t trace_bins_bytes(int K) { return align_up(sizeof(hyg_u128) * (size_t)(1 + 2 * K), 16); }
__host__ __device__ inline size_t trace_bins_extra(int K) {
  return trace_bins_bytes(K) <= sizeof(Shared::ph) ? 0 : trace_bins_bytes(K);
}

// (merged, control regime, case regime) of candidate n = s * np_prev + a of the
// previous step: the regime part of tg_xi on its ancestor's (m, r_c, r_k), or of
// init_state on the first step. No hazards, no durations.
__device__ __forceinline__ void trace_class(int K, int n, int np_prev, bool init, const uint64_t* pst, int& m,
                                            int& rc, int& rk) {
  if (init) {
    const int i = n / K, j = n - (n / K) * K;
    m = (i == j); rc = i; rk = j;
    return;
  }
  const int s = fdiv(n, np_prev, 1.0f / (float)np_prev), a = n - s * np_prev;
  const uint64_t anc = pst[a];
  const int am = hyg_st_m(anc), arc = hyg_st_rc(anc), ark = hyg_st_rk(anc);
  if (s == 0) { m = am; rc = arc; rk = ark; }
  else if (s < K) { m = 0; rc = (s - 1 < ark) ? s - 1 : s; rk = ark; }
  else if (s < 2 * K - 1) { const int q = s - K; m = 0; rc = arc; rk = (q < arc) ? q : q + 1; }
  else if (s == 2 * K - 1) { m = 1; rc = arc; rk = arc; }
  else { const int j = s - 2 * K, i = j / K, jj = j - i * K; m = (i == jj); rc = i; rk = jj; }
}
// bin += f: two 64-bit LDS atomics, the carry out of the low limb (of this
// add, whatever other adds stand around it) taken into the high one. The sum is
// an integer sum, so the order of the adds does not show in it. (f < 2^101.)
__device__ __forceinline__ void trace_add(hyg_u128* bin, hyg_u128 f) {
  unsigned long long* p = (unsigned long long*)bin;
  const unsigned long long old = __hip_atomic_fetch_add(p, (unsigned long long)f.lo, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_WORKGROUP);
  const unsigned long long hi = (unsigned long long)f.hi + ((old + f.lo < old) ? 1u : 0u);
  if (hi) __hip_atomic_fetch_add(p + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void trace_accumulate(hyg_u128* tbin, int K, int n, int np_prev, bool init,
                                                 const uint64_t* pst, hyg_u128 f) {
  if (hyg_u128_is_zero(f)) return;
  int m, rc, rk;
  trace_class(K, n, np_prev, init, pst, m, rc, rk);
  if (m == 0) trace_add(tbin, f);
  trace_add(tbin + 1 + rc, f);
  trace_add(tbin + 1 + K + rk, f);
}
// One row of the trace, by the lanes of one wave, behind the barrier that
// follows the row's last trace_add: log Z from lane 0, class c's probability
// from lane c, (float)(S_c / S) with one f64 division; the bins are left zero
// for the next row (whose adds are behind further barriers).
__device__ __forceinline__ void trace_store_row(const TraceArg<true>& tr, int64_t row, int K, double lz, hyg_u128 S,
                                                hyg_u128* tbin, bool probs) {
  const int l = lane_id();
  if (l == 0 && tr.log_z_t) tr.log_z_t[row] = lz;
  if (!probs) return;
  const double tot = hyg_u128_to_f64(S, 100);
  for (int c = l; c < 1 + 2 * K; c += 64) {
    const hyg_u128 b = tbin[c];
    tbin[c] = hyg_u128_zero();
    const float p = (float)(hyg_u128_to_f64(b, 100) / tot);
    if (c == 0) {
      if (tr.split_probs) tr.split_probs[row] = p;
    } else if (tr.regime_probs) {
      tr.regime_probs[row * (2 * K) + (c - 1)] = p;
    }
  }
}
// Rows [r0, r1) of a chain whose weights all became -inf (HYG_ENUMERIC):
// log Z = -inf, the probabilities NaN.
template <int NT>
__device__ __forceinline__ void trace_fill(const TraceArg<true>& tr, int64_t r0, int64_t r1, int K) {
  const float nanf_ = hyg_bits_f32(0x7fc00000u);
  for (int64_t r = r0 + threadIdx.x; r < r1; r += NT) {
    if (tr.log_z_t) tr.log_z_t[r] = HYG_NINF;
    if (tr.split_probs) tr.split_probs[r] = nanf_;
    if (tr.regime_probs)
      for (int c = 0; c < 2 * K; ++c) tr.regime_probs[r * (2 * K) + c] = nanf_;
  }
}

// Three waves per SIMD (<= 168 VGPRs) at 256 and 768 threads: a CU holds three
// chains or one (the second argument is the minimum waves per SIMD); 512
// threads (one chain per CU: C5 by its LDS, or a low-occupancy launch) may use
// up to 256 VGPRs.
//
// GW: a shape whose full-N arrays exceed LDS (forward_global_w). The weights W
// and the key area (the sort keys, the candidate list, the prefix arrays of the
// keep / fallback paths and, through the W area, the sorted keys) live in the
// chain's global scratch (ChainDev::wg_offset of `wscr`: the same workspace as
// `ws`, disjoint bytes, passed as its own pointer so that the record stores
// through the restrict-qualified `ws` are not assumed independent of it).
// Every hand-off of those arrays between threads is behind a full workgroup
// fence (part_barrier<GW>), and every optimal step resamples through the
// counting sort: the top-set path's scratch is the W area in LDS.
//
// MM: a multi-model launch (launch_chains_multi). The argument is the launch's
// model table instead of one model, and the workgroup takes its chain's entry
// (ChainDev::pad) once, here at entry: a load that is uniform over the
// workgroup. Everything behind it is the single-model code.
//
// REC: the chain's ancestor history is recorded for the backward kernel. A
// forward-only build (REC = false, launch_filter) has every store into the
// record area compiled out and never forms its address: the launch's workspace
// holds no history. Everything else is the same code, so the chain's log Z,
// final weights and status are those of its full run, bit for bit.
//
// TRC: a traced forward-only build (REC = false only, launch_trace). Where a
// step forms the log-sum-exp of the previous site's weights it also stores
// that site's row of the trace (TraceArg): log Z of the chain up to the site
// and, where a probability array is given (uniform over the workgroup), the
// filtering marginals from 1 + 2K exact class sums of the list's F = 100 masses,
// which every list entry adds into LDS bins behind the layout (trace_add). The
// last wave stores the row behind the reduction's LDS barrier. The first step
// does so for row 0, the closing sum for row T - 1. Nothing the chain computes
// reads the bins, so log Z, final weights and status stay those of REC = false.
//
// RES: a resuming build (REC = true only, 256 threads; tg_kernels_res.hip), the
// later rounds of a launch whose forward is cut in time (forward_schedule).
// Block b takes the chain its entry names (ResArg) instead of chain b, rebuilds
// the loop state at the top of step t_begin from the chain's record t_begin - 1
// as the backward kernel rebuilds a step (record t - 1 holds the ancestors and
// the scalars of step t - 1; the hazard rows and the weights are functions of
// them) and enters the same step loop there. t_begin = 1 (mod 64), >= 65: the
// emission ring, the uniform ring and the priority lookup are then where the
// unsplit loop has them, and the record is never the MODE_INIT one. Status,
// log Z and the final weights go to the chain's own index.
template <int NT, int KC = 0, int MC = 0, int BC = 0, bool PHS = false, bool GW = false,  // PHS: phase-timer build
          bool MM = false, bool REC = true, bool TRC = false, bool RES = false>
__global__ void __launch_bounds__(NT, (NT == 512 ? 1 : 3))
tg_forward_kernel(ModelArg<MM> md_arg, const ChainDev* __restrict__ chains, const double* __restrict__ E,
                  uint8_t* __restrict__ ws, int32_t* status_out, double* __restrict__ logz_out,
                  double* __restrict__ finalw_out, Lay lay_arg, unsigned long long* __restrict__ dbg_arg,
                  uint8_t* __restrict__ wscr, TraceArg<TRC> trc, ResArg<RES> res) {
  static_assert(!GW || KC == 0, "global weights: the generic shape only");
  static_assert(!TRC || (!REC && !PHS), "traced builds: forward-only, no phase timers");
  static_assert(!RES || (REC && !PHS && !GW && !TRC && NT == 256), "resuming builds: recording, 256 threads, in LDS");
  constexpr bool BW = kBatchedWeights<NT, GW, KC>;  // the weights in batches of slots (gen_weights)
  // the timers only exist in the PHS instantiation: a constant null pointer
  // folds every timer test away (no SGPRs, branches or s_memtime in the step loop)
  unsigned long long* __restrict__ const dbg = PHS ? dbg_arg : nullptr;
  unsigned chain = blockIdx.x;  // the chain's index in the launch: descriptor and per-chain outputs
  int t_begin = 1;
  if constexpr (RES) {
    const ResEntry e = res.entries[blockIdx.x];
    chain = (unsigned)e.chain;
    t_begin = e.t_begin;
    if (status_out[chain] != HYG_OK) return;  // uniform: the chain failed in an earlier round
  }
  const ModelDev md = model_of(md_arg, chains, chain);
  const hyg_tg_consts* __restrict__ c = md.consts;
  const int K = KC ? KC : c->K, M = KC ? MC : c->M, I = KC ? 2 * KC + KC * KC : c->I, K2 = 2 * K,
            tid = threadIdx.x;
  const Lay lay = KC ? make_layout(KC, MC, BC, MC * (2 * KC + KC * KC), NT, false) : lay_arg;
  // in a register for the whole chain: a load of c-> inside the step loop is a
  // global load the compiler cannot hoist past the record stores (it may
  // alias them), followed by a vmcnt(0) wait on every outstanding store
  const float sig_thresh = c->sig_thresh;
  const ChainDev ch = chains[chain];
  const int T = ch.T;
  extern __shared__ __align__(16) unsigned char smem[];
  // (GW: lay.W and lay.keys are offsets into the chain's global scratch)
  unsigned char* const pbase = GW ? (unsigned char*)(wscr + ch.wg_offset) : smem;
  double* W = (double*)(pbase + lay.W);
  uint64_t* keys = (uint64_t*)(pbase + lay.keys);
  hyg_u128* cp128 = (hyg_u128*)(pbase + lay.keys);  // prefix arrays of the keep / fallback paths
  int* bcnt = (int*)(smem + lay.bcnt);
  int* bpos = (int*)(smem + lay.bpos);
  hyg_u192* tau = (hyg_u192*)(smem + lay.bcnt);
  hyg_u192* pre64 = (hyg_u192*)(smem + lay.pre64);
  uint64_t* pst0 = (uint64_t*)(smem + lay.pst);  // [2][M]: buffer `cur` holds the current ancestors
  double* pw0 = (double*)(smem + lay.pw);
  Hz4* phz0 = (Hz4*)(smem + lay.phz);
  int cur = 0;
  Pf3* pf = (Pf3*)(smem + lay.pf);
  double* ering = (double*)(smem + lay.ering);
  ConstLds& cl = *(ConstLds*)(smem + lay.cl);
  int* parents = (int*)(smem + lay.parents);
  unsigned char* red = smem + lay.red;
  Shared& sh = *(Shared*)(smem + lay.sh);
  float* uring = (float*)(smem + lay.uring);  // NT >= 256 only (kURing)
  constexpr bool kURing = NT >= 256;
  constexpr int kUR = NT >= 512 ? 64 : 32;  // ring entries
  int* part_cnt = (int*)(smem + lay.part);
  hyg_u192* part_tot = (hyg_u192*)(smem + lay.part + sizeof(int) * kNCut * (NT / 64));
  // TRC: the class sums, zero between rows; whether any probability is wanted; the first row not yet written
  hyg_u128* const tbin = trace_bins_extra(K) ? (hyg_u128*)(smem + lay.total) : (hyg_u128*)sh.ph;
  bool trc_probs = false;
  int trc_next = 0;
  if constexpr (TRC) {
    trc_probs = trc.split_probs != nullptr || trc.regime_probs != nullptr;
    if (tid < 1 + K2) tbin[tid] = hyg_u128_zero();  // (behind the barrier below)
  }

  // phase timers (diagnostic runs only: dbg != nullptr), kept in LDS
  unsigned long long* ph_acc = sh.ph;
  if (tid < kPh) ph_acc[tid] = 0;
#define PH(k)                                                      \
  if (dbg && tid == 0) {                                           \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
    ph_acc[k] += now_ - ph_acc[kPh - 1];                                \
    ph_acc[kPh - 1] = now_;                                             \
  }

  uint8_t* const rec0 = REC ? ws + ch.ws_offset : nullptr;
  const size_t rstride = record_bytes(M);
  const double* Ech = E + ch.site_begin * K2;

  double mloc;
  int cloc;
  int N = K * K, np_prev = 0, prev_mode = MODE_INIT;
  float prev_logc = 0.0f;
  double prev_lse = 0.0;
  double mx;
  int cnt;
  if constexpr (!RES) {
  // ---- t = 0 (_filter_first_step)
  load_consts(cl, c, md);
  load_eblock(ering, Ech, 0, T, K2, NT);
  load_eblock(ering, Ech, 1, T, K2, NT);
  if (tid == 0) {
    sh.Unext = hyg_u01f(hyg_rand64(ch.seed, ch.chain_id, HYG_RNG_SYSTEMATIC, 1, 0));
    sh.r_ph = (int)hyg_mulhi64(hyg_rand64(ch.seed, ch.chain_id, HYG_RNG_PHANTOM, 0, 0), (uint64_t)K);
    sh.status = HYG_OK;
    if constexpr (REC) {
      StepScalars* s0 = (StepScalars*)rec0;
      s0->mode = MODE_INIT; s0->n_par = 0; s0->log_c = 0.0f; s0->r_ph = sh.r_ph; s0->lse = 0.0; s0->pad = 0.0;
    }
  }
  if (kURing && wave_id() == NT / 64 - 1 && lane_id() < kUR)  // steps 1 .. kUR
    uring[(1 + lane_id()) & (kUR - 1)] =
        hyg_u01f(hyg_rand64(ch.seed, ch.chain_id, HYG_RNG_SYSTEMATIC, (uint64_t)(1 + lane_id()), 0));
  lds_barrier();
  gen_weights_init<NT>(cl, K, sh.r_ph, erow(ering, 0, K2), W, &mloc, &cloc);
  if constexpr (GW) __syncthreads();  // global W: read by other threads from the first step on
  block_max_cnt<NT>(mloc, cloc, red, &mx, &cnt);
  } else {
    // ---- the top of step t_begin, from record t_begin - 1 (the backward's
    //      prologue: ancestors as stored, their hazard rows by hz_at, the
    //      children's by prefetch_rows), into buffer `cur` = 0
    static_assert(!RES || kURing, "resuming builds: the uniform ring");
    const int tr = t_begin - 1;
    load_consts(cl, c, md);
    load_eblock(ering, Ech, tr / kEBlock, T, K2, NT);  // rows t_begin - 1 .. (t_begin = 1 mod kEBlock)
    load_eblock(ering, Ech, tr / kEBlock + 1, T, K2, NT);
    const uint8_t* rec = rec0 + (size_t)tr * rstride;
    const StepScalars s = *(const StepScalars*)rec;
    if (tid == 0) {
      sh.r_ph = 0;  // (read by MODE_INIT steps only)
      sh.status = HYG_OK;
    }
    if (tid < s.n_par) {
      const uint64_t* rst = (const uint64_t*)(rec + sizeof(StepScalars));
      const uint64_t st = rst[tid];
      pst0[tid] = st;
      pw0[tid] = ((const double*)(rst + M))[tid];
      const double2 hc = hz_at(md, K, 0, hyg_st_rc(st), hyg_st_dc(st));
      const double2 hk = hz_at(md, K, 1, hyg_st_rk(st), hyg_st_dk(st));
      Hz4 h;
      h.lrc = hc.x; h.l1c = hc.y; h.lrk = hk.x; h.l1k = hk.y;
      phz0[tid] = h;
      pf[tid] = prefetch_rows(md, K, st);
    }
    if (wave_id() == NT / 64 - 1 && lane_id() < kUR)  // steps t_begin .. t_begin + kUR - 1 (t_begin = 1 mod kUR)
      uring[(t_begin + lane_id()) & (kUR - 1)] =
          hyg_u01f(hyg_rand64(ch.seed, ch.chain_id, HYG_RNG_SYSTEMATIC, (uint64_t)(t_begin + lane_id()), 0));
    np_prev = s.n_par;
    prev_mode = s.mode;
    prev_logc = s.log_c;
    prev_lse = s.lse;
    lds_barrier();
    gen_weights<NT, BW>(cl, K, I, np_prev, prev_mode, prev_logc, prev_lse, pst0, pw0, phz0, erow(ering, tr, K2), W,
                        &mloc, &cloc);
    N = I * np_prev;
    block_max_cnt<NT>(mloc, cloc, red, &mx, &cnt);
  }

  // where the top-set path parks the ancestors it gathers ahead (Ahead): the
  // window is the launch's (lay_arg: the compile-time shapes build their own layout)
  Ahead ahead{};
  if constexpr (!GW && kSortWaves<NT> <= 4)
    ahead = ahead_area<NT, kSortWaves<NT>>(smem + lay.W, lay.bcnt - lay.W, lay_arg.gather_w);

  // the wave's base priority (rotating builds: see prio_base), looked up every kPrioEvery steps
  constexpr bool kRot = HYG_PRIO_ROT && NT == 256;
  const bool rot = kRot && lay_arg.prio_rot != 0;  // (the launch's: lay_arg, as gather_w)
  const int slot3 = kRot ? wave_slot3() : 0;
  int pb = 0;
  // candidate lists walked per 64 entries (list_walk; the launch's, as gather_w)
  constexpr bool kFine = kFineLists<NT, GW>;
  const bool fine = kFine && lay_arg.list_fine != 0;

  if (dbg && tid == 0) ph_acc[kPh - 1] = __builtin_amdgcn_s_memtime();
  for (int t = t_begin; t < T; ++t) {
    if constexpr (kRot) {
      if (rot && (t & (kPrioEvery - 1)) == 1) {
        pb = __builtin_amdgcn_readfirstlane(prio_base(slot3));
        set_prio(pb);
      }
    }
    // the ancestors of step t-1's particles (read by the regenerations and the gather)
    const uint64_t* pst = pst0 + cur * M;
    const double* pw = pw0 + cur * M;
    const Hz4* phz = phz0 + cur * M;
    // What candidate n of step t-1 is as an ancestor of step t: its state, its
    // own hazards and its weight, recomputed (the W area may hold the sort):
    // weight_at's arithmetic with the child formed once. (Reading W[n] instead,
    // with the top-set scratch moved out of the W area at 512 threads, measured
    // 0.8 % slower: r03r.) The gather calls it per parent; the top-set path
    // calls it ahead, per sorted position (Ahead).
    auto ancestor_of = [&](int n, uint64_t& s, double& w, Hz4& h) {
      if (prev_mode == MODE_INIT) {
        s = init_state(K, n);
        const double2 hc = cl.hz1[0][hyg_st_rc(s)], hk = cl.hz1[1][hyg_st_rk(s)];
        h.lrc = hc.x; h.l1c = hc.y; h.lrk = hk.x; h.l1k = hk.y;
        const int i = n / K, j = n - (n / K) * K;
        const double* E0 = erow(ering, 0, K2);
        w = (E0[i] + E0[K + j]) + ((i == j) ? cl.lPc[sh.r_ph * K + i] : HYG_NINF);
      } else {
        const int sl = fdiv(n, np_prev, 1.0f / (float)np_prev);
        const int ao = n - sl * np_prev;
        const uint64_t anc = pst[ao];
        const Pf3 pfo = pf[ao];
        const Hz4 hzo = phz[ao];
        const double pao = pw[ao];
        s = tg_xi_hz_sel(cl, K, 1.0f / (float)K, anc, sl, pfo, &h);
        const double tr = tg_trans(cl, K, anc, s, hzo);
        const double* Ep = erow(ering, t - 1, K2);
        w = HYG_NINF;
        if (hyg_isfinite(tr)) {
          const double lg = tr + (Ep[hyg_st_rc(s)] + Ep[K + hyg_st_rk(s)]);
          if (prev_mode == MODE_KEEP) w = pao + lg;
          else if (prev_mode == MODE_UNBIASED) w = (-cl.log_M + prev_lse) + lg;
          else {
            const double v = (double)prev_logc + (pao - prev_lse);
            w = (pao + lg) - (v < 0.0 ? v : 0.0);
          }
        }
      }
    };
    // emission rows one block ahead: issue at the block start, land in the ring later
    const bool eload = ((t % kEBlock) == 0) && (t + kEBlock < T);
    PH(0);
    if (!(mx > HYG_NINF)) {
      if (tid == 0) sh.status = HYG_ENUMERIC;
      break;  // uniform
    }
    // written during step t-1's gather (or, kURing, a multiple of kUR steps ago), before two barriers
    const float Ucur = kURing ? uring[t & (kUR - 1)] : sh.Unext;
    // ---- log_softmax / reduce_logsumexp of the weights of step t-1
    // ---- per wave, the list of candidates with W - mx >= sig_thresh (keys
    //      area): every nonzero F=100 mass (x >= -70) and every significant
    //      f32 log-weight is on it; candidates interleaved over the waves
    int* lst = (int*)keys;
    const int lst_base = wave_id() * (((N + NT - 1) / NT) * 64);
    int lst_cnt = 0;
    const bool topset = !GW && cnt > M && M <= 64;  // this step resamples by the top-set path
    {
      // kCC candidates per lane at a time, their loads issued together (a
      // load / compare / ballot per iteration waits out an LDS round trip each)
      const double cutw = (double)sig_thresh;
      // (the shape-specialised kernel: every candidate in one pass, N <= M I)
      constexpr int kCC = KC ? (MC * (2 * KC + KC * KC) + NT - 1) / NT : 8;
      for (int b0 = wave_id() * 64; b0 < N; b0 += kCC * NT) {
        bool keep[kCC];
#pragma unroll
        for (int j = 0; j < kCC; ++j) {
          const int n = b0 + j * NT + lane_id();
          const double w = W[n < N ? n : 0];
          // `&`, not `&&`: a short-circuit test puts the load under a branch
          // and waits out its round trip before the next candidate's load
          keep[j] = (n < N) & (w - mx >= cutw);
        }
#pragma unroll
        for (int j = 0; j < kCC; ++j) {
          const uint64_t bal = wave_ballot(keep[j]);
          if (keep[j]) lst[lst_base + lst_cnt + lanes_below(bal)] = b0 + j * NT + lane_id();
          lst_cnt += (int)__builtin_popcountll(bal);
        }
      }
      if constexpr (GW) __syncthreads();  // the list is in global memory
      else wave_lds_sync();
    }
    PH(22);
    double logS;
    hyg_u128 trcS = hyg_u128_zero();  // TRC: the mass sum behind logS
    {
      // kLR list entries per lane at a time: every load of the chunk issued
      // first, then kLR independent exp / fixed-point chains in straight-line
      // code (hyg_fix100 is branch-free), so they interleave. fix100(exp(x))
      // is 0 for x < -70; padding lanes take x = -inf (mass 0, no cutoff).
      // Top-set steps also count the list per cutoff (per-lane counters).
      constexpr int kLR = kLRof<NT>;
      hyg_u128 s0 = hyg_u128_zero(), s1 = hyg_u128_zero();
      int ccut[kNCut - 1];
#pragma unroll
      for (int k = 0; k < kNCut - 1; ++k) ccut[k] = 0;
      // (kFineLists builds; the others run the written-out copy in the else branch below: change the two together)
      [[maybe_unused]] auto lse_chunk = [&](auto rc, int b) {  // R entries per lane from entry b on; lst_cnt is wave-uniform
        constexpr int R = decltype(rc)::value;
        int nn[R];
        double xx[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int i = b + r * 64 + lane_id();
          nn[r] = lst[lst_base + (i < lst_cnt ? i : b)];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const double w = W[nn[r]];
          xx[r] = (b + r * 64 + lane_id() < lst_cnt) ? w - mx : HYG_NINF;
        }
        hyg_u128 ff[R];
        exp_fix100_lockstep<R>(xx, ff);
        if constexpr (TRC) {
          if (trc_probs) {  // (uniform; padding lanes hold mass 0)
#pragma unroll
            for (int r = 0; r < R; ++r)
              trace_accumulate(tbin, K, nn[r], np_prev, prev_mode == MODE_INIT, pst, ff[r]);
          }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (r & 1) s1 = hyg_u128_add(s1, ff[r]); else s0 = hyg_u128_add(s0, ff[r]);
        }
        if (topset) {  // wave counts per cutoff by ballots (scalar sums)
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int k = 0; k < kNCut - 1; ++k)
              ccut[k] += (int)__builtin_popcountll(wave_ballot(xx[r] >= -cut_below_top(k)));
        }
      };
      if constexpr (kFine) {
        list_walk<kLR>(lst_cnt, fine, lse_chunk);
      } else {
        // (the other builds keep the loop written out: their code is what it was, register for
        // register; called through the lambda their spills move. This is `lse_chunk` above at
        // R = kLR, statement for statement: change the two together)
        for (int b = 0; b < lst_cnt; b += 64 * kLR) {  // lst_cnt is wave-uniform
          int nn[kLR];
          double xx[kLR];
#pragma unroll
          for (int r = 0; r < kLR; ++r) {
            const int i = b + r * 64 + lane_id();
            nn[r] = lst[lst_base + (i < lst_cnt ? i : b)];
          }
#pragma unroll
          for (int r = 0; r < kLR; ++r) {
            const double w = W[nn[r]];
            xx[r] = (b + r * 64 + lane_id() < lst_cnt) ? w - mx : HYG_NINF;
          }
          hyg_u128 ff[kLR];
          exp_fix100_lockstep<kLR>(xx, ff);
          if constexpr (TRC) {
            if (trc_probs) {  // (uniform; padding lanes hold mass 0)
#pragma unroll
              for (int r = 0; r < kLR; ++r)
                trace_accumulate(tbin, K, nn[r], np_prev, prev_mode == MODE_INIT, pst, ff[r]);
            }
          }
#pragma unroll
          for (int r = 0; r < kLR; ++r) {
            if (r & 1) s1 = hyg_u128_add(s1, ff[r]); else s0 = hyg_u128_add(s0, ff[r]);
          }
          if (topset) {  // wave counts per cutoff by ballots (scalar sums)
#pragma unroll
            for (int r = 0; r < kLR; ++r)
#pragma unroll
              for (int k = 0; k < kNCut - 1; ++k)
                ccut[k] += (int)__builtin_popcountll(wave_ballot(xx[r] >= -cut_below_top(k)));
          }
        }
      }
      PH(23);
      if (topset) {
        if (lane_id() == 0) {  // read after the reduction's barriers below
#pragma unroll
          for (int k = 0; k < kNCut - 1; ++k) part_cnt[wave_id() * kNCut + k] = ccut[k];
          part_cnt[wave_id() * kNCut + kNCut - 1] = lst_cnt;
        }
      }
      const hyg_u128 sacc = hyg_u128_add(s0, s1);
      PH(12);
      // own slot of `red`, whose last reader (this reduction, a step ago) is
      // behind many barriers: no leading barrier
      const hyg_u128 S = block_sum128<NT, false>(sacc, red + 32 * (NT / 64));
      PH(11);
      logS = hyg_log(hyg_u128_to_f64(S, 100));
      if constexpr (TRC) trcS = S;
    }
    const double lse = logS + mx;
    if constexpr (TRC) {
      // row t - 1: every trace_add of the step is behind the reduction's barrier
      if constexpr (NT == 64) wave_lds_sync();
      if (wave_id() == NT / 64 - 1) trace_store_row(trc, ch.out_begin + (t - 1), K, lse, trcS, tbin, trc_probs);
      trc_next = t;
    }
    PH(1);
    int mode, np;
    float log_c = 0.0f;
    bool need_bar = true;  // parents written by many threads, no barrier behind them yet
    bool parked = false;   // the top-set path gathered ancestors ahead (Ahead)
    if (cnt <= M) {
      // ---- keep every particle with non-zero weight, in index order (:207-209)
      mode = MODE_KEEP;
      np = cnt;
      const int cs = (N + NT - 1) / NT;
      const int p0 = tid * cs, p1 = (p0 + cs < N) ? p0 + cs : N;
      int loc = 0;
      for (int n = p0; n < p1; ++n) loc += (W[n] > HYG_NINF);
      hyg_u128 v;
      v.lo = (uint64_t)loc;
      v.hi = 0;
      block_scan128<NT>(v, cp128, red);
      part_barrier<GW>();
      int o = (int)cp128[tid].lo;
      for (int n = p0; n < p1; ++n)
        if (W[n] > HYG_NINF) parents[o++] = n;
      PH(2);
      if (dbg && tid == 0) ph_acc[10]++;
    } else {
      // ---- OptimalFiniteState (resampling_functions.py:7-52)
      PH(2);
      int fs = FAST_FALLBACK;
      if (topset)
        fs = top_set_resample<NT, kSortWaves<NT>, kFine>(W, N, mx, logS, lst, lst_base, lst_cnt, fine, smem + lay.W,
                                  lay.bcnt - lay.W,
                                  (uint64_t*)(smem + lay.bcnt), lay.bcnt_bytes, part_cnt, part_tot, parents, sh, cl,
                                  red, M, cnt, Ucur, lay.topset_r, ahead, ancestor_of, ph_acc, dbg != nullptr, pb);
      parked = fs == FAST_DONE_AHEAD;  // the parents' sorted positions are published beside them
      if (parked) fs = FAST_DONE;
      PH(20);
      if (fs != FAST_DONE) {
        if (fs == FAST_FALLBACK_REGEN) {  // the top-set path used the W area: rebuild step t-1's weights
          if (prev_mode == MODE_INIT) {
            gen_weights_init<NT>(cl, K, sh.r_ph, erow(ering, t - 1, K2), W, &mloc, &cloc);
          } else {
            gen_weights<NT, BW>(cl, K, I, np_prev, prev_mode, prev_logc, prev_lse, pst, pw, phz,
                                erow(ering, t - 1, K2), W, &mloc, &cloc);
          }
          lds_barrier();
        }
        optimal_resample<NT, GW>(W, (uint64_t*)W, N, mx, logS, sig_thresh, keys, bcnt, bpos, pre64, tau, parents,
                             sh, cl, red, M, cnt, ch.seed, ch.chain_id, t, Ucur, ph_acc, dbg != nullptr);
        if (dbg && tid == 0) ph_acc[21]++;
      }
      if (dbg && tid == 0) ph_acc[9] += sh.n_sig;
      PH(3);
      int Kk = sh.Kk;
      log_c = sh.log_c;
      if (Kk >= N) { Kk = N; log_c = HYG_NINFF; }
      np = M;
      if (!hyg_isfinitef(log_c)) {
        // ---- unbiased fallback: M categorical draws from log_weights (:42-47)
        mode = MODE_UNBIASED;
        log_c = 0.0f;
        const double lmax = (double)(float)((mx - mx) - logS);  // the largest f32 log-weight
        part_barrier<GW>();  // the sorted keys in the W area are replaced by the regenerated weights
        if (prev_mode == MODE_INIT) {
          gen_weights_init<NT>(cl, K, sh.r_ph, erow(ering, t - 1, K2), W, &mloc, &cloc);
        } else {
          gen_weights<NT, BW>(cl, K, I, np_prev, prev_mode, prev_logc, prev_lse, pst, pw, phz,
                              erow(ering, t - 1, K2), W, &mloc, &cloc);
        }
        part_barrier<GW>();
        auto logit = [&](int n) -> double {
          const double w = W[n];
          return (w > HYG_NINF) ? (double)(float)((w - mx) - logS) : HYG_NINF;
        };
        auto rnd = [&](int q) -> uint64_t {
          return hyg_rand64(ch.seed, ch.chain_id, HYG_RNG_MULTINOMIAL, (uint64_t)t, (uint64_t)q);
        };
        auto out = [&](int q, int n) { parents[q] = n; };
        auto all = [](int) { return true; };
        part_barrier<GW>();
        categorical_block<NT, GW>(N, lmax, logit, M, all, rnd, out, cp128, red);
      } else {
        mode = MODE_OPTIMAL;
        // the top-set path's parents (wave 0) and sh.* are behind its last barrier
        need_bar = fs != FAST_DONE;
      }
    }
    if (need_bar) part_barrier<GW>();
    PH(4);
    // (np <= M <= 64 at the pipeline shape: the gather is wave 0's alone)
    if (wave_id() == 0) serial_begin(pb);
    // ---- gather the ancestors (state, weight, own hazards), record them,
    //      and start the hazard-row prefetch for their children
    StepScalars* rs = REC ? (StepScalars*)(rec0 + (size_t)t * rstride) : nullptr;
    uint64_t* rst = REC ? (uint64_t*)(rs + 1) : nullptr;
    double* rw = REC ? (double*)(rst + M) : nullptr;
    Pf3 pfa;
    uint64_t gs = 0;
    double gw = 0.0;
    Hz4 gh{};
    const bool have_pf = tid < np;  // np <= M <= NT: one ancestor per thread
    if (have_pf) {
      const int a = tid;
      uint64_t s;
      double w;
      Hz4 h;
      // an optimal step of the top-set path: the entry parked at the parent's
      // sorted position, where one was gathered ahead
      const int pp = (parked && mode == MODE_OPTIMAL) ? ahead.pos[a] : ahead.n;
      if (pp < ahead.n) {
        s = ahead.st[pp];
        w = ahead.w[pp];
        h = ahead.hz[pp];
      } else {
        ancestor_of(parents[a], s, w, h);
      }
      gs = s;
      gw = w;
      gh = h;
      if constexpr (REC) {
        rst[a] = s;
        rw[a] = w;
      }
      pfa = prefetch_rows(md, K, s);  // in flight during the weights
    }
    if constexpr (REC) {
      if (tid == 0) {
        rs->mode = mode; rs->n_par = np; rs->log_c = log_c; rs->r_ph = 0; rs->lse = lse; rs->pad = 0.0;
      }
    }
    if (wave_id() == 0) serial_end(pb);
    if (kURing) {  // steps t+1 .. t+kUR, one per lane, every kUR steps (step t's entry was read above)
      if (wave_id() == NT / 64 - 1 && (t & (kUR - 1)) == 0 && lane_id() < kUR)
        uring[(t + 1 + lane_id()) & (kUR - 1)] =
            hyg_u01f(hyg_rand64(ch.seed, ch.chain_id, HYG_RNG_SYSTEMATIC, (uint64_t)(t + 1 + lane_id()), 0));
    } else if (wave_id() == NT / 64 - 1) {  // a wave with no ancestor (when NT > M): next step's uniform
      const float un = hyg_u01f(hyg_rand64(ch.seed, ch.chain_id, HYG_RNG_SYSTEMATIC, (uint64_t)(t + 1), 0));
      if (lane_id() == 0) sh.Unext = un;
    }
    // emission block prefetch (registers), stored into the ring after the weights
    constexpr int EQ = (kEBlock * 2 * HYG_KMAX + NT - 1) / NT;  // rows of one block per thread
    double ebuf[EQ];
    int e_tot = 0;
    if (eload) {
      const int t0 = (t / kEBlock + 1) * kEBlock;
      const int rows = (T - t0) < kEBlock ? (T - t0) : kEBlock;
      e_tot = rows * K2;
#pragma unroll
      for (int q = 0; q < EQ; ++q) {
        const int i = tid + q * NT;
        ebuf[q] = (i < e_tot) ? Ech[(size_t)t0 * K2 + i] : 0.0;
      }
    }
    np_prev = np;
    prev_mode = mode;
    prev_logc = log_c;
    prev_lse = lse;
    // the new ancestors into the other buffer: its last readers (step t-1's
    // weights) are behind this step's barriers
    if (have_pf) {
      const int o = (cur ^ 1) * M + tid;
      pst0[o] = gs;
      pw0[o] = gw;
      phz0[o] = gh;
    }
    part_barrier<GW>();
    cur ^= 1;
    PH(5);
    // ---- propose and weight the particles of step t
    gen_weights<NT, BW>(cl, K, I, np, mode, log_c, lse, pst0 + cur * M, pw0 + cur * M, phz0 + cur * M,
                        erow(ering, t, K2), W, &mloc, &cloc);
    if constexpr (GW) __syncthreads();  // global W: the next step (or the final sum) reads other threads' weights
    PH(7);
    N = I * np;
    if (have_pf) pf[tid] = pfa;
    if (eload) {
      double* dst = ering + (size_t)((t / kEBlock + 1) & 1) * kEBlock * K2;
#pragma unroll
      for (int q = 0; q < EQ; ++q) {
        const int i = tid + q * NT;
        if (i < e_tot) dst[i] = ebuf[q];
      }
    }
    PH(8);
    // (every read of red by this step's resampling is behind the gather's barriers)
    block_max_cnt<NT, false>(mloc, cloc, red, &mx, &cnt);
    PH(6);
  }
  // ---- final weights: log normalising constant and run()'s second output
  double logS = HYG_NINF;
  if constexpr (TRC) {
    if (mx > HYG_NINF) {  // log_mass_sum with the class sums; row T - 1
      const uint64_t* pst = pst0 + cur * M;
      hyg_u128 s = hyg_u128_zero();
      for (int n = tid; n < N; n += NT) {
        const hyg_u128 f = hyg_exp_fix100(W[n] - mx);
        s = hyg_u128_add(s, f);
        if (trc_probs) trace_accumulate(tbin, K, n, np_prev, prev_mode == MODE_INIT, pst, f);
      }
      const hyg_u128 S = block_sum128<NT>(s, red);
      logS = hyg_log(hyg_u128_to_f64(S, 100));
      if constexpr (NT == 64) wave_lds_sync();
      if (wave_id() == NT / 64 - 1) trace_store_row(trc, ch.out_begin + (T - 1), K, logS + mx, S, tbin, trc_probs);
    } else {  // from the first site whose weights are all -inf
      trace_fill<NT>(trc, ch.out_begin + trc_next, ch.out_begin + T, K);
    }
  } else {
    if (mx > HYG_NINF) logS = log_mass_sum<NT>(W, N, mx, red);
  }
  if (tid == 0) {
    int st = sh.status;
    if (st == HYG_OK && !(mx > HYG_NINF)) st = HYG_ENUMERIC;
    status_out[chain] = st;
    logz_out[chain] = logS + mx;
  }
  if (finalw_out) {
    const int Nmax = c->Nmax;
    for (int n = tid; n < Nmax; n += NT) finalw_out[(size_t)chain * Nmax + n] = (n < N) ? W[n] : HYG_NINF;
  }
  if (dbg && tid == 0) {
    for (int k = 0; k < kPh - 1; ++k) dbg[(size_t)blockIdx.x * kPh + k] = ph_acc[k];
    dbg[(size_t)blockIdx.x * kPh + kPh - 1] = (unsigned long long)T;
  }
#undef PH
}

}  // namespace hyg
