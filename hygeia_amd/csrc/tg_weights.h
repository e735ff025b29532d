// tg_weights.h -- a step's weights in the two-group chain kernels: the
// transition density from registers (TransRegs), gen_weights (slot by slot or
// in batches of slots), gen_weights_init and their exact mass sum (log_mass_sum).
#pragma once

#include "tg_dev.h"

namespace hyg {

// Scalars of the transition density held in registers by gen_weights.
struct TransRegs {
  double lPm0, lPm1, lPm2, lPm3, lU1, lU2;
  int u;
};

// tg_trans with the ancestor decoded in registers (same operands, same
// addition order, so bit-identical); lPc stays in LDS.
__device__ __forceinline__ double tg_trans_r(const TransRegs& q, const double* __restrict__ lPc, int K, int m,
                                             int dc, int rc, int dk, int rk, uint64_t next, const Hz4& h) {
  const int m2 = hyg_st_m(next), rc2 = hyg_st_rc(next);
  const int j = m * 2 + m2;
  const double lPm_j = j == 0 ? q.lPm0 : (j == 1 ? q.lPm1 : (j == 2 ? q.lPm2 : q.lPm3));
  return tg_trans_sel(lPm_j, lPc[rc * K + rc2], q.lU1, q.lU2, q.u, m, dc, rc, dk, rk, next, h);
}

// The shape-specialised 256-thread forward builds (weights in LDS) take a wave's
// proposal slots in batches (gen_weights<NT, true>): a chain's step waits
// for the LDS round trips of this phase, not for issue slots. The generic
// builds keep the slot-by-slot schedule: with K at run time the batches spill
// (DESIGN section 6, round 11). HYG_WGEN_BATCH is the number of slots whose
// loads are in flight together (six more live VGPRs per slot).
#ifndef HYG_WGEN_BATCH
#define HYG_WGEN_BATCH 3
#endif
template <int NT, bool GW, int KC>
constexpr bool kBatchedWeights = NT == 256 && !GW && KC > 0;

// All weights of a step t >= 1; returns this thread's max and count of finite weights.
// With np <= 64 every wave keeps one ancestor per lane in registers and walks
// the proposal slots s = wave, wave + NT/64, ... (slot-uniform control flow);
// otherwise one candidate per thread through weight_one.
// BATCH: the slots in batches of HYG_WGEN_BATCH, every LDS load of a batch
// ahead of its arithmetic (below); K is then a compile-time constant of the caller.
template <int NT, bool BATCH = false>
__device__ __forceinline__ void gen_weights(const ConstLds& cl, int K, int I, int np, int mode, float log_c,
                                            double lse, const uint64_t* __restrict__ pst,
                                            const double* __restrict__ pw, const Hz4* __restrict__ phz,
                                            const double* __restrict__ Et, double* __restrict__ W, double* m_out,
                                            int* c_out) {
  const int N = I * np;
  double m = HYG_NINF;
  int cnt = 0;
  if (np <= 64) {
    constexpr int NW = NT / 64;
    const int lane = lane_id(), wv = wave_id();
    TransRegs q;
    q.lPm0 = cl.lPm[0]; q.lPm1 = cl.lPm[1]; q.lPm2 = cl.lPm[2]; q.lPm3 = cl.lPm[3];
    q.lU1 = cl.lU1; q.lU2 = cl.lU2; q.u = cl.u;
    const double* __restrict__ lPc = cl.lPc;
    if (lane < np) {
      const uint64_t par = pst[lane];
      const double pa = pw[lane];
      const Hz4 h = phz[lane];
      const int am = hyg_st_m(par), adc = hyg_st_dc(par), arc = hyg_st_rc(par), adk = hyg_st_dk(par),
                ark = hyg_st_rk(par);
      // w = (base + lg) - sub reproduces the three branches of weight_one exactly
      double base = pa, sub = 0.0;
      if (mode == MODE_UNBIASED) base = -cl.log_M + lse;
      if (mode == MODE_OPTIMAL) {
        const double v = (double)log_c + (pa - lse);
        sub = v < 0.0 ? v : 0.0;
      }
      // tg_trans of every proposal slot with the child substituted
      // (case_control_proposal_mappings.py:11-134): the per-ancestor parts
      // once, per slot only what the slot changes. Same operands and the same
      // addition order as tg_trans, so the weights are bit-identical.
      const double NINF = HYG_NINF;
      const bool ok = (adk < adc ? adk : adc) >= q.u;
      const int j00 = am * 2;
      const double lPm_s = j00 == 0 ? q.lPm0 : q.lPm3;  // m' = m
      const double lm0 = ok ? (am ? q.lPm2 : q.lPm0) : (am == 0 ? 0.0 : NINF);
      const double lm1 = ok ? (am ? q.lPm3 : q.lPm1) : (am == 1 ? 0.0 : NINF);
      const double lmA = ok ? lPm_s : 0.0;
      const double* __restrict__ lPcr = lPc + arc * K;  // row r_c of log P_ctrl
      const double lcA = (adc + 1 == 1) ? (h.lrc + lPcr[arc]) : h.l1c;  // d_c' = d_c + 1, r_c' = r_c
      const double lkB = (adk == 0) ? NINF : h.l1k;
      const double lkA = am == 1 ? ((ark == arc && adk == adc) ? 0.0 : NINF) : (arc == ark ? NINF : lkB);
      const bool condC = (am == 1 && adc + 1 != 1) || (arc == ark && am == 0);
      const double lkC_cp = h.lrk + ((arc == ark) ? q.lU1 : q.lU2);
      const int dD = (am == 0) ? adc + 1 : 0;  // merge slot: both groups at d
      const double lcD = (dD == 1) ? (h.lrc + lPcr[arc]) : ((dD == adc + 1) ? h.l1c : NINF);
      const double Ec_rc = Et[arc], Ek_rk = Et[K + ark];
      auto put = [&](int s, double tr, double e) {
        double w = NINF;
        if (hyg_isfinite(tr)) w = (base + (tr + e)) - sub;
        W[s * np + lane] = w;
        m = dmax(m, w);
        cnt += (w > NINF) ? 1 : 0;
      };
      const int K2 = 2 * K;
      if constexpr (BATCH) {
        // The wave's slots in batches of BS. The compiler hoists no LDS load
        // over a wave-uniform branch, so a slot per basic block is one LDS
        // round trip and one dependent f64 chain after the other. A batch is
        // one basic block: every load of its slots first, then their weights
        // as independent chains, then the stores. A slot past the wave's last
        // one reads what the wave's first slot reads and stores nothing. Per
        // weight the operands and the order of the additions are put()'s.
        // (The one shape built this way, K = 6 at four waves, fills every
        // batch of three: 3 A-D and 9 two-change-point slots per wave, so the
        // clamps, the masks and the uneven trip count fold away there. They
        // are for other values of HYG_WGEN_BATCH and other compiled shapes.)
        constexpr int BS = HYG_WGEN_BATCH;
        auto put_if = [&](bool on, int s, double tr, double e) {
          const double v = (base + (tr + e)) - sub;
          const double w = hyg_isfinite(tr) ? v : NINF;
          if (on) {  // wave-uniform
            W[s * np + lane] = w;
            m = dmax(m, w);
            cnt += (w > NINF) ? 1 : 0;
          }
        };
        // Slot types A-D, one select form: a slot loads at most one entry of Et
        // and one of lPcr (per-lane indices) and chooses its operands by its
        // type, a constant of the wave index wq: no select is left.
        auto ad_slots = [&](const int wq) {
          const int nAD = (wq < K2) ? (K2 - wq + NW - 1) / NW : 0;
#pragma unroll
          for (int k0 = 0; k0 < (K2 + NW - 1) / NW; k0 += BS) {
            if (k0 >= nAD) break;
            int sl[BS], rr[BS];
            bool on[BS];
            double et[BS], pc[BS];
#pragma unroll
            for (int b = 0; b < BS; ++b) {
              on[b] = k0 + b < nAD;
              const int s = wq + (on[b] ? k0 + b : 0) * NW;
              const bool tB = s >= 1 && s < K, tC = s >= K && s < K2 - 1;
              const int qq = s - K;
              // B: control change to r != r_k; C: case change to r != r_c
              const int r = tB ? ((s - 1 < ark) ? s - 1 : s) : (tC ? ((qq < arc) ? qq : qq + 1) : arc);
              sl[b] = s;
              rr[b] = r;
              et[b] = Et[tB ? r : K + r];  // (D: Et[K + r_c]; A: not used)
              pc[b] = lPcr[r];             // (B only)
            }
#pragma unroll
            for (int b = 0; b < BS; ++b) {
              const int s = sl[b];
              const bool tA = s == 0, tB = s >= 1 && s < K, tD = s == K2 - 1;
              const double lkC = condC ? q.lU1 : ((rr[b] != ark) ? lkC_cp : NINF);
              const double lm = tA ? lmA : (tD ? lm1 : lm0);
              const double lc = tB ? (h.lrc + pc[b]) : (tD ? lcD : lcA);
              const double lk = tA ? lkA : (tB ? lkB : (tD ? 0.0 : lkC));
              put_if(on[b], s, (lm + lc) + lk, (tB ? et[b] : Ec_rc) + ((tA || tB) ? Ek_rk : et[b]));
            }
          }
        };
#pragma unroll
        for (int w = 0; w < NW; ++w)
          if (wv == w) ad_slots(w);
        // two change points (i, j): x = (i == j, 1, i, 1, j), from the wave's
        // first slot >= 2K; the trip count once (every wave's is the same
        // where NW divides 2K and K^2, as at the compiled shape)
        const int s0 = wv + NW * ((K2 - wv + NW - 1) / NW);
        const bool even = K2 % NW == 0 && (I - K2) % NW == 0;
        const int nE = even ? (I - K2) / NW : ((s0 < I) ? (I - s0 + NW - 1) / NW : 0);
#pragma unroll
        for (int k0 = 0; k0 < (I - K2 + NW - 1) / NW; k0 += BS) {
          if (k0 >= nE) break;
          int sl[BS], ii[BS], jj[BS];
          bool on[BS];
          double ei[BS], ej[BS], pc[BS];
#pragma unroll
          for (int b = 0; b < BS; ++b) {
            on[b] = k0 + b < nE;
            sl[b] = s0 + (on[b] ? k0 + b : 0) * NW;
            ii[b] = (sl[b] - K2) / K;
            jj[b] = (sl[b] - K2) - ii[b] * K;
            ei[b] = Et[ii[b]];
            ej[b] = Et[K + jj[b]];
            pc[b] = lPcr[ii[b]];
          }
#pragma unroll
          for (int b = 0; b < BS; ++b) {
            const int i = ii[b], j = jj[b];
            const double e = ei[b] + ej[b];
            const double lc = h.lrc + pc[b];
            double lk;
            if (i == j) lk = 0.0;
            else if (i == ark && am == 0) lk = q.lU1;
            else lk = (j != ark) ? (h.lrk + ((i == ark) ? q.lU1 : q.lU2)) : NINF;
            put_if(on[b], sl[b], (((i == j) ? lm1 : lm0) + lc) + lk, e);
          }
        }
        *m_out = m;
        *c_out = cnt;
        return;
      }
      // Slot by slot (every other build): loops with trip counts fixed by K
      // (compile-time in the shape-specialised kernels, so they unroll; each
      // slot stays a basic block of its own: load, wait, arithmetic, store);
      // s is wave-uniform.
#pragma unroll
      for (int k = 0; k < (K2 + NW - 1) / NW; ++k) {  // slot types A-D
        const int s = wv + k * NW;
        if (s >= K2) break;
        if (s == 0) {
          put(0, (lmA + lcA) + lkA, Ec_rc + Ek_rk);
        } else if (s < K) {  // control change to r != r_k
          const int r = (s - 1 < ark) ? s - 1 : s;
          put(s, (lm0 + (h.lrc + lPcr[r])) + lkB, Et[r] + Ek_rk);
        } else if (s < K2 - 1) {  // case change to r != r_c
          const int qq = s - K;
          const int r = (qq < arc) ? qq : qq + 1;
          const double lk = condC ? q.lU1 : ((r != ark) ? lkC_cp : NINF);
          put(s, (lm0 + lcA) + lk, Ec_rc + Et[K + r]);
        } else {  // merge
          put(s, (lm1 + lcD) + 0.0, Ec_rc + Et[K + arc]);
        }
      }
      // two change points (i, j): x = (i == j, 1, i, 1, j), from the wave's
      // first slot >= 2K
      const int s0 = wv + NW * ((K2 - wv + NW - 1) / NW);
#pragma unroll
      for (int k = 0; k < (I - K2 + NW - 1) / NW; ++k) {
        const int s = s0 + k * NW;
        if (s >= I) break;
        const int ii = (s - K2) / K, jj = (s - K2) - ii * K;
        const double e = Et[ii] + Et[K + jj];
        const double lc = h.lrc + lPcr[ii];
        double lk;
        if (ii == jj) lk = 0.0;
        else if (ii == ark && am == 0) lk = q.lU1;
        else lk = (jj != ark) ? (h.lrk + ((ii == ark) ? q.lU1 : q.lU2)) : NINF;
        put(s, (((ii == jj) ? lm1 : lm0) + lc) + lk, e);
      }
    }
    *m_out = m;
    *c_out = cnt;
    return;
  }
  for (int n = threadIdx.x; n < N; n += NT) {
    const double w = weight_one(cl, K, n, np, mode, log_c, lse, pst, pw, phz, Et);
    W[n] = w;
    m = dmax(m, w);
    cnt += (w > HYG_NINF) ? 1 : 0;
  }
  *m_out = m;
  *c_out = cnt;
}
template <int NT>
__device__ __forceinline__ void gen_weights_init(const ConstLds& cl, int K, int r_ph, const double* Et, double* W,
                                                 double* m_out, int* c_out) {
  double m = HYG_NINF;
  int cnt = 0;
  for (int n = threadIdx.x; n < K * K; n += NT) {
    const int i = n / K, j = n - (n / K) * K;
    const double obs = Et[i] + Et[K + j];
    const double tr = (i == j) ? cl.lPc[r_ph * K + i] : HYG_NINF;
    const double w = obs + tr;
    W[n] = w;
    m = dmax(m, w);
    cnt += (w > HYG_NINF) ? 1 : 0;
  }
  *m_out = m;
  *c_out = cnt;
}

// log of the exact F=100 mass sum of exp(W - mx) over W[0..N).
template <int NT>
__device__ __forceinline__ double log_mass_sum(const double* W, int N, double mx, unsigned char* red) {
  hyg_u128 s = hyg_u128_zero();
#pragma unroll 4
  for (int n = threadIdx.x; n < N; n += NT) {
    const double x = W[n] - mx;
    s = hyg_u128_add(s, hyg_exp_fix100(x));  // exp(x < -70) < 2^-100 -> 0
  }
  const hyg_u128 S = block_sum128<NT>(s, red);
  return hyg_log(hyg_u128_to_f64(S, 100));
}

}  // namespace hyg
