// sg_sample_kernels.hip -- backward simulation of the single-group model from
// the history of a forward-only launch (sg_chain_kernel's HST builds): joint
// draws of the whole segmentation, B trajectories per chain.
//
//   sg_sample_kernel  one wave per (chain, trajectory b), four waves per
//                     workgroup; the waves share nothing and meet at no barrier.
//
// A particle is (d, r) and the predecessor of (d > 1, r) can only be
// (d - 1, r), so a backward draw is needed at segment starts only: the
// trajectory jumps from segment start to segment start and is a fill between
// them, O(segments * N_max + T) per trajectory.
//
// A draw from the set of site s with logits l_n, n < N_s:
// m = max l_n, i_n = hyg_exp_fix100(l_n - m), C_n the inclusive sums in n
// order, S = C_{N-1}, uu = (hyg_rand64(seed, chain_id, 6, s, b) >> 11) 2^-53,
// thr = max(1, ceil(uu S)), n* = the smallest n with C_n >= thr. Only integers
// are compared, so the result does not depend on the reduction order. Lane l
// holds the particles l + 64 j, j < 4.
#include <hip/hip_runtime.h>

#include "../../include/hyg_arith.h"
#include "hyg_dev.h"
#include "sg_common.h"
#include "sg_dev.h"

namespace hyg {

constexpr int kSgSampleWaves = 4;               // trajectories per workgroup
constexpr int kSgSampleSlots = kSgThreads / 64;  // particles per lane

// (d mod 2^16, r) as the two int16 of a path row, one 32-bit store
__device__ __forceinline__ uint32_t sg_path_word(int d, int r) {
  return ((uint32_t)d & 0xffffu) | (((uint32_t)r & 0xffffu) << 16);
}

// rows of sites [0, t] of trajectory b: -1 (the rest of a trajectory that cannot go on)
__device__ __forceinline__ void sg_sample_fill_bad(uint32_t* __restrict__ pw, int64_t out_begin, int B, int b, int t,
                                                   int lane) {
  for (int s = t - lane; s >= 0; s -= 64) pw[((size_t)out_begin + (size_t)s) * (size_t)B + b] = 0xffffffffu;
}

__global__ void __launch_bounds__(64 * kSgSampleWaves)
sg_sample_kernel(SgMultiDev mm, const SgChainDev* __restrict__ chains, int n_chains, SgHistDev hs,
                 const int32_t* __restrict__ fwd_status, int B, int groups, uint32_t* __restrict__ pw,
                 int32_t* __restrict__ sample_status) {
  const int chain = (int)(blockIdx.x / (unsigned)groups);
  const int b = (int)(blockIdx.x % (unsigned)groups) * kSgSampleWaves + wave_id();
  const int lane = lane_id();
  if (chain >= n_chains || b >= B) return;  // wave-uniform: no barrier follows
  const SgChainDev ch = chains[chain];
  const SgModelDev md = mm.models[mm.chain_model[chain]];
  const hyg_sg_consts& c = *md.consts;
  const int K = c.K, u = c.u, Nmax = c.Nmax;
  int t = ch.T - 1;
  const int fst = fwd_status ? fwd_status[chain] : HYG_OK;
  if (fst != HYG_OK) {
    sg_sample_fill_bad(pw, ch.out_begin, B, b, t, lane);
    if (sample_status && b == 0 && lane == 0) sample_status[chain] = fst;
    return;
  }
  int r_to = -1;  // the regime entered at the segment start above the draw; -1: the draw of the last site
  // every round moves t down by d >= 1: at most T rounds
  while (t >= 0) {
    const size_t row = (size_t)ch.out_begin + (size_t)t;
    int N = hs.n_part[row];
    N = N < 0 ? 0 : (N > Nmax ? Nmax : N);
    const int nj = (N + 63) >> 6;  // (<= kSgSampleSlots: Nmax <= 256)
    double lg[kSgSampleSlots];
    double mx = HYG_NINF;
#pragma unroll
    for (int j = 0; j < kSgSampleSlots; ++j) {
      const int n = lane + 64 * j;
      double l = HYG_NINF;
      if (j < nj && n < N) {
        const double lw = hs.lw[row * (size_t)Nmax + n];
        if (r_to < 0) {
          l = lw;
        } else {
          const uint32_t st = hs.st[row * (size_t)Nmax + n];
          if (sg_d(st) >= 1 && sg_r(st) < K) {
            double base, cont;
            sg_trans_parts(md, u, st, base, cont);
            l = (lw + base) + c.logP[sg_r(st) * K + r_to];  // the forward's a_n first
          }
        }
        if (!(l == l)) l = HYG_NINF;
      }
      lg[j] = l;
      mx = dmax(mx, l);
    }
    mx = wave_max(mx);
    bool ok = mx > HYG_NINF && mx < HYG_INF;
    int nstar = -1;
    if (ok) {
      hyg_u128 im[kSgSampleSlots], tot[kSgSampleSlots];
      hyg_u128 S = hyg_u128_zero();
#pragma unroll
      for (int j = 0; j < kSgSampleSlots; ++j) {
        im[j] = hyg_u128_zero();
        tot[j] = hyg_u128_zero();
        if (j < nj) {
          im[j] = hyg_exp_fix100(lg[j] - mx);
          tot[j] = wave_sum128(im[j]);
          S = hyg_u128_add(S, tot[j]);
        }
      }
      const double uu =
          (double)(hyg_rand64(ch.seed, ch.chain_id, kSgRngSample, (uint64_t)t, (uint64_t)b) >> 11) *
          1.1102230246251565404e-16;
      hyg_u128 thr = sg_ceil_mul_f64(uu, S);
      if (hyg_u128_is_zero(thr)) thr.lo = 1;
      hyg_u128 off = hyg_u128_zero();
#pragma unroll
      for (int j = 0; j < kSgSampleSlots; ++j) {
        if (j < nj && nstar < 0) {
          const hyg_u128 end = hyg_u128_add(off, tot[j]);
          if (!hyg_u128_lt(end, thr)) {  // the threshold falls among the particles 64 j .. 64 j + 63
            const hyg_u128 cn = hyg_u128_add(off, wave_incl128(im[j]));
            const uint64_t hit = wave_ballot(!hyg_u128_lt(cn, thr));
            if (hit) nstar = 64 * j + __builtin_ctzll(hit);
          }
          off = end;
        }
      }
      ok = nstar >= 0 && nstar < N;
    }
    int d = 0, r = 0;
    if (ok) {
      const uint32_t st = hs.st[row * (size_t)Nmax + nstar];
      d = sg_d(st);
      r = sg_r(st);
      ok = d >= 1 && d <= t + 1 && r < K;
    }
    if (!ok) {  // no finite logit, a sojourn longer than the chain so far, a regime >= K: not on a forward's history
      sg_sample_fill_bad(pw, ch.out_begin, B, b, t, lane);
      if (sample_status && lane == 0) sample_status[chain] = HYG_ENUMERIC;
      return;
    }
    // the segment: sites t - d + 1 .. t hold (d - (t - site), r)
    for (int k = lane; k < d; k += 64)
      pw[((size_t)ch.out_begin + (size_t)(t - k)) * (size_t)B + b] = sg_path_word(d - k, r);
    r_to = r;
    t -= d;
  }
}

int sg_launch_sample(const SgMultiDev& mm, const hyg_sg_consts& c, const SgChainDev* chains_dev, int n_chains,
                     const SgHistDev& hist, const int32_t* fwd_status, int B, int16_t* paths, int32_t* sample_status,
                     void* stream) {
  if (n_chains <= 0) return HYG_OK;
  if (c.Nmax > kSgThreads || c.K < 2 || c.K > HYG_KMAX) return HYG_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (sample_status && hipMemsetAsync(sample_status, 0, sizeof(int32_t) * (size_t)n_chains, s) != hipSuccess)
    return HYG_EDEVICE;
  const int groups = (B + kSgSampleWaves - 1) / kSgSampleWaves;
  hipLaunchKernelGGL(sg_sample_kernel, dim3((unsigned)n_chains * (unsigned)groups), dim3(64 * kSgSampleWaves), 0, s,
                     mm, chains_dev, n_chains, hist, fwd_status, B, groups, (uint32_t*)paths, sample_status);
  return hipGetLastError() == hipSuccess ? HYG_OK : HYG_EDEVICE;
}

}  // namespace hyg
