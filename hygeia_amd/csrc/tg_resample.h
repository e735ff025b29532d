// tg_resample.h -- resampling in the two-group chain kernels: categorical
// draws over a workgroup (categorical_block), optimal finite-state resampling
// through the counting sort (optimal_resample) and through the top-set path
// (top_set_resample: the bitonic and rank sorts, sys_count, the two finishes).
#pragma once

#include "tg_weights.h"

namespace hyg {

// Categorical draws (tfd.Categorical(logits).sample with TF's multinomial CDF
// semantics): for each active draw q with random bits rnd(q), the first n with
// cdf_n > floor(u * total). logit(n) is recomputed on demand.
// GW: cp is in global memory (the forward's key area of a global-weights shape).
template <int NT, bool GW = false, typename LogitFn, typename ActiveFn, typename RandFn, typename OutFn>
__device__ __forceinline__ void categorical_block(int N, double lmax, LogitFn logit, int n_draw, ActiveFn active,
                                                  RandFn rnd, OutFn out, hyg_u128* cp, unsigned char* red) {
  const int cs = (N + NT - 1) / NT;
  const int p0 = threadIdx.x * cs, p1 = (p0 + cs < N) ? p0 + cs : N;
  hyg_u128 loc = hyg_u128_zero();
  for (int n = p0; n < p1; ++n) {
    const double x = logit(n) - lmax;
    loc = hyg_u128_add(loc, hyg_exp_fix100(x));
  }
  block_scan128<NT>(loc, cp, red);
  part_barrier<GW>();
  const hyg_u128 total = cp[NT];
  for (int q = threadIdx.x; q < n_draw; q += NT) {
    if (!active(q)) continue;
    const hyg_u128 target = hyg_scale_target(rnd(q), total);
    int lo = 0, hi = NT - 1;  // last chunk with cp[ch] <= target
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (hyg_u128_lt(target, cp[mid])) hi = mid - 1; else lo = mid;
    }
    int sel = -1;
    for (int ch = lo; ch < NT && sel < 0; ++ch) {
      hyg_u128 cdf = cp[ch];
      const int a0 = ch * cs, a1 = (a0 + cs < N) ? a0 + cs : N;
      for (int n = a0; n < a1; ++n) {
        const double x = logit(n) - lmax;
        cdf = hyg_u128_add(cdf, hyg_exp_fix100(x));
        if (hyg_u128_lt(target, cdf)) { sel = n; break; }
      }
    }
    out(q, sel < 0 ? N - 1 : sel);
  }
}

// ------------------------------------------------------ optimal resampling
// OptimalFiniteState (resampling_functions.py:7-52) on the significant
// log-weights (weights below sig_thresh have zero f32 mass and can
// never be counted by the K search):
//  1. counting sort: buckets by a monotone map of the f32 value, then each key
//     is ranked inside its bucket; the sorted order is unique (value desc,
//     index asc), so the bucket map only affects speed;
//  2. exact 192-bit mass prefix sums of the sorted masses;
//  3. the K / log c loop (:12-23): log c(a) and the prefix count P(c(a)) are
//     evaluated for every a < M at once (one lane per a), then the loop's
//     iterates a' = max(a, P(c(a))) are followed;
//  4. the systematic residual draw (:32-40, :56-69): target j lands on the
//     first residual position with C >= ceil(T_j R) (exact), found by the
//     thread whose chunk of sorted positions contains it.
// Writes parents[0..M) and sh.Kk / sh.log_c (log_c not finite -> caller
// runs the unbiased fallback). Returns n_sig via sh.n_sig.
template <int NT, bool GW = false>
__device__ __forceinline__ void optimal_resample(const double* W, uint64_t* sorted, int N, double mx, double logS, float thr,
                                 uint64_t* keys, int* bcnt, int* bpos, hyg_u192* pre64, hyg_u192* tau, int* parents,
                                 Shared& sh,
                                 const ConstLds& cl, unsigned char* red, int M, int cnt_fin, uint64_t seed,
                                 uint64_t chain_id, int t, float Usys, unsigned long long* ph, bool timed) {
  const int tid = threadIdx.x;
#define SPH(k)                                                     \
  if (timed && tid == 0) {                                         \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
    ph[k] += now_ - ph[kPh - 1];                                        \
    ph[kPh - 1] = now_;                                                 \
  }
  // any monotone map works (the order inside a bucket is resolved exactly);
  // sqrt spacing puts narrow buckets where the weights crowd, near the top
  const float scale = 1.0f / (-thr);
  auto bucket_of = [&](float lw) -> int {
    const int q = (int)(__builtin_sqrtf((-lw) * scale) * (float)kBuckets);
    return q < kBuckets - 1 ? q : kBuckets - 1;
  };
  // ---- 1a. bucket histogram
  for (int i = tid; i < kBuckets; i += NT) bcnt[i] = 0;
  part_barrier<GW>();
  #pragma unroll 4
  for (int n = tid; n < N; n += NT) {
    const double w = W[n];
    if (w > HYG_NINF) {
      const float lw = (float)((w - mx) - logS);
      if (lw >= thr) atomicAdd(&bcnt[bucket_of(lw)], 1);
    }
  }
  part_barrier<GW>();
  SPH(17);
  // ---- 1b. bucket starts (exclusive scan), kBuckets / NT buckets per thread
  {
    constexpr int PB = (kBuckets + NT - 1) / NT;
    int loc = 0;
    for (int i = 0; i < PB; ++i) {
      const int q = tid * PB + i;
      if (q < kBuckets) loc += bcnt[q];
    }
    int tot;
    int run = block_excl_int<NT>(loc, red, &tot);
    for (int i = 0; i < PB; ++i) {
      const int q = tid * PB + i;
      if (q < kBuckets) { bpos[q] = run; run += bcnt[q]; }
    }
    if (tid == 0) sh.n_sig = tot;
  }
  part_barrier<GW>();
  SPH(18);
  const int n_sig = sh.n_sig;
  // ---- 1c. scatter into buckets (arbitrary order inside a bucket)
  #pragma unroll 4
  for (int n = tid; n < N; n += NT) {
    const double w = W[n];
    if (w > HYG_NINF) {
      const float lw = (float)((w - mx) - logS);
      if (lw >= thr) keys[atomicAdd(&bpos[bucket_of(lw)], 1)] = sort_key(lw, n);
    }
  }
  part_barrier<GW>();
  SPH(19);
  // ---- 1d. rank every key inside its bucket and place it in `sorted` (the
  //          W area: every read of W is done); bpos now holds the bucket ends
  for (int p = tid; p < n_sig; p += NT) {
    const uint64_t k = keys[p];
    const int q = bucket_of(key_value(k));
    const int end = bpos[q], beg = end - bcnt[q];
    int rank = 0;
#pragma unroll 4
    for (int i = beg; i < end; ++i) rank += (keys[i] < k) ? 1 : 0;
    sorted[beg + rank] = k;
  }
  part_barrier<GW>();
  SPH(13);
  // ---- 2. masses and exact prefix sums over contiguous chunks of sorted positions
  const int cs = (n_sig + NT - 1) / NT;
  const int p0 = tid * cs;
  const int p1 = (p0 + cs < n_sig) ? p0 + cs : n_sig;
  hyg_u192 loc = hyg_u192_zero();
  // the f32 masses of this thread's chunk stay in registers for the prefix,
  // the K search and the systematic walk (chunks longer than kMR recompute)
  constexpr int kMR = 8;
  float mreg[kMR];
  const bool inreg = cs <= kMR;
  if (inreg) {
#pragma unroll
    for (int i = 0; i < kMR; ++i) {
      const int p = p0 + i;
      mreg[i] = 0.0f;
      if (p < p1) mreg[i] = hyg_expf(key_value(sorted[p]));
    }
#pragma unroll
    for (int i = 0; i < kMR; ++i) loc = hyg_u192_add(loc, hyg_fix149f(mreg[i]));
  } else {
    for (int p = p0; p < p1; ++p) loc = hyg_u192_add(loc, hyg_fix149f(hyg_expf(key_value(sorted[p]))));
  }
  auto mass_at = [&](int p) -> float {  // mass of sorted position p of this thread's chunk
    if (inreg) {
      float v = 0.0f;
#pragma unroll
      for (int i = 0; i < kMR; ++i) v = (p - p0 == i) ? mreg[i] : v;
      return v;
    }
    return hyg_expf(key_value(sorted[p]));
  };
  hyg_u192 total;
  const hyg_u192 myex = block_excl192<NT>(loc, red, &total);
  const int npre = M < 64 ? M : 64;  // pre64 holds min(M, 64) entries (make_layout)
  if (p0 < npre) {  // inclusive prefix of the first npre sorted positions
    hyg_u192 run = myex;
    for (int p = p0; p < p1 && p < npre; ++p) {
      run = hyg_u192_add(run, hyg_fix149f(mass_at(p)));
      pre64[p] = run;
    }
  }
  part_barrier<GW>();
  SPH(14);
  // ---- 3. K / log c (loop-variable semantics of :12-31)
  if (wave_id() == 0) {
    const int lane = lane_id();
    if (M <= 64) {
      // lane a: c(a) and the prefix count P(c(a)) = #{p : fl(c(a) + x_p) > 0}
      int Pa = 0;
      float ca = 0.0f;
      hyg_u192 rva = hyg_u192_zero();
      const int a = lane;
      if (a < M && a < N) {
        if (a < n_sig) rva = hyg_u192_sub(total, a == 0 ? hyg_u192_zero() : pre64[a - 1]);
        const double rvd = hyg_u192_to_f64(rva);
        const float l2 = (rvd == 0.0) ? HYG_NINFF : (float)hyg_log(rvd);
        ca = cl.logMa[a] - l2;
        if (hyg_isfinitef(ca)) {
          int lo = 0, hi = n_sig;  // first p with the predicate false
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((float)(ca + key_value(sorted[mid])) > 0.0f) lo = mid + 1; else hi = mid;
          }
          Pa = lo;
        } else if (ca > 0.0f) {
          Pa = cnt_fin;  // +inf: every finite particle
        } else {
          Pa = 0;
        }
      }
      // follow a <- max(a, P(c(a))) from a = 0 (the body runs at least once)
      int aa = 0, bb = -1;
      while (aa != bb && aa < N && aa < M) {
        const int nxt = __builtin_amdgcn_readlane(Pa, aa);
        bb = aa;
        aa = nxt > aa ? nxt : aa;
      }
      const float lc = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ca), bb));
      hyg_u192 R;
      R.w0 = rdlane64(rva.w0, bb);
      R.w1 = rdlane64(rva.w1, bb);
      R.w2 = rdlane64(rva.w2, bb);
      if (lane == 0) {
        sh.Kk = bb;
        sh.log_c = lc;
        sh.R = R;
        sh.preK = hyg_u192_sub(total, R);
      }
    } else {
      // general M: the loop as written, one iteration at a time
      int a = 0, b = -1;
      float lc = -1.0f;
      hyg_u192 rv_last = hyg_u192_zero();
      while (a != b && a < N && a < M) {
        hyg_u192 rv = hyg_u192_zero();
        if (a < n_sig) {
          hyg_u192 pre = hyg_u192_zero();
          if (a > 0 && a <= 64) pre = pre64[a - 1];
          else if (a > 64) {
            pre = pre64[63];
            for (int p = 64; p < a; ++p) pre = hyg_u192_add(pre, hyg_fix149f(hyg_expf(key_value(sorted[p]))));
          }
          rv = hyg_u192_sub(total, pre);
        }
        const double rvd = hyg_u192_to_f64(rv);
        const float l1 = hyg_logf((float)(M - a));
        const float l2 = (rvd == 0.0) ? HYG_NINFF : (float)hyg_log(rvd);
        const float cn = l1 - l2;
        int cnt = 0;
        if (hyg_isfinitef(cn)) {
          int lo = 0, hi = n_sig;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((float)(cn + key_value(sorted[mid])) > 0.0f) lo = mid + 1; else hi = mid;
          }
          cnt = (lo - a) > 0 ? lo - a : 0;
        } else if (cn > 0.0f) {
          cnt = (cnt_fin - a) > 0 ? cnt_fin - a : 0;
        }
        b = a;
        a = a + cnt;
        lc = cn;
        rv_last = rv;
      }
      if (lane == 0) {
        sh.Kk = b;
        sh.log_c = lc;
        sh.R = rv_last;
        sh.preK = hyg_u192_sub(total, rv_last);
      }
    }
  }
  part_barrier<GW>();
  SPH(15);
  int Kk = sh.Kk;
  const float log_c = sh.log_c;
  if (Kk >= N || !hyg_isfinitef(log_c)) return;  // caller runs the unbiased fallback
  // ---- 4. deterministic top-K, systematic residual with exact thresholds
  const int L = M - Kk;
  const float U = Usys;  // hyg_u01f(hyg_rand64(seed, chain_id, HYG_RNG_SYSTEMATIC, t, 0)), drawn ahead
  const float Lf = (float)L;
  const hyg_u192 R = sh.R, preK = sh.preK;
  for (int j = tid; j < L; j += NT) {
    tau[j] = hyg_u192_add(preK, hyg_ceil_mul_f32_bf(((float)j + U) / Lf, R));
    parents[Kk + j] = key_index(sorted[Kk]);  // unfilled -> residual index 0
  }
  for (int p = tid; p < Kk; p += NT) parents[p] = key_index(sorted[p]);
  part_barrier<GW>();
  if (p0 < n_sig && p0 + cs > Kk && L > 0) {
    // first target not reached before this chunk: #{j : tau_j <= C(p0 - 1)}
    int j = 0;
    if (p0 > Kk) {
      int lo = 0, hi = L;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (hyg_u192_ge(myex, tau[mid])) lo = mid + 1; else hi = mid;
      }
      j = lo;
    }
    hyg_u192 C = myex;
    for (int p = p0; p < p1 && j < L; ++p) {
      C = hyg_u192_add(C, hyg_fix149f(mass_at(p)));
      if (p >= Kk) {
        while (j < L && hyg_u192_ge(C, tau[j])) {
          parents[Kk + j] = key_index(sorted[p]);
          ++j;
        }
      }
    }
  }
  SPH(16);
#undef SPH
}

// ------------------------------------------- resampling: the top-set path
// OptimalFiniteState touches the order of the largest log-weights only: the
// K / log c search reads the prefix masses of the first a < M sorted weights
// and counts #{p : fl(c + x_p) > 0}, and the systematic targets land where
// the cumulative residual mass crosses them (at C3 the deepest draw sits near
// sorted rank 300 of ~900 significant weights). This path sorts exactly only
// the top set A = {lw >= cut} for the most inclusive of kNCut cutoffs whose
// set fits one block bitonic sort (<= 128 keys per wave), takes the total
// mass of every significant weight from an order-free exact sum, and then
// checks with exact quantities that each index decision falls inside A:
//   - every K-loop probe the loop visits has its prefix and its count in A;
//   - the last systematic target lies at or below the mass of A.
// If a check fails the caller runs the full counting-sort path
// (optimal_resample), so the parents are those of the full sort either way.
enum { FAST_DONE = 0, FAST_FALLBACK = 1, FAST_FALLBACK_REGEN = 2 };
#define TPH(k)                                                     \
  if (timed && threadIdx.x == 0) {                                 \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
    ph[k] += now_ - ph[kPh - 1];                                   \
    ph[kPh - 1] = now_;                                            \
  }

// cutoffs of the top set in W - mx (nats below the largest weight); the last
// set (k = kNCut - 1) is the whole candidate list (W - mx >= sig_thresh)
__host__ __device__ constexpr double cut_below_top(int k) {
  // selects, not a table: a runtime index into a local array is a memory load
  return k < 4 ? (k < 2 ? (k == 0 ? 14.0 : 17.0) : (k == 2 ? 20.0 : 23.0))
               : (k < 6 ? (k == 4 ? 26.0 : 30.0) : 36.0);
}

// The narrow (u128) images of the top set's outside masses: from cutoff
// kNarrowCut on, every outside mass is below e^-cut, and a lane sums at most
// kNarrowPerLane of them; their images m 2^149 must sum below 2^128, i.e.
// cut > ln(kNarrowPerLane 2^21) = 19.41 nats for 128 entries per lane.
constexpr int kNarrowCut = 2;
constexpr int kNarrowPerLane = 128;
static_assert(kNarrowPerLane <= 128 && cut_below_top(kNarrowCut) >= 19.5,
              "u128 outside-mass images: 128 masses below e^-19.5 sum below 2^128 at scale 2^149");

// Lanes l of a wave whose key keeps the minimum at stage (KK, J) of the
// bitonic sort below, for J in [R, 64R) and the wave bit of i clear
template <int R, int J, int KK>
constexpr uint64_t keep_min_pattern() {
  uint64_t m = 0;
  for (int l = 0; l < 64; ++l) {
    const bool a = (l & (J / R)) == 0;
    const bool b = (KK < 64 * R) ? ((l & (KK / R)) == 0) : true;
    if (a == b) m |= 1ull << l;
  }
  return m;
}

// One compare-exchange stage (k, j) of a bitonic sort of 64*NW*R keys held
// R per lane, key index i = wave*64R + lane*R + r (ascending result).
// j < R: inside the lane; j < 64R: lane xor shuffles; else: LDS + barrier.
template <int NT, int R, int KK, int J>
__device__ __forceinline__ void bitonic_stage(uint64_t (&e)[R], uint64_t* buf, int& ib) {
  constexpr int n = 64 * (NT / 64) * R;
  const int base = (int)(threadIdx.x >> 6) * 64 * R + lane_id() * R;
  if constexpr (J < R) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int pr = r ^ J;
      if (pr > r) {
        const bool up = ((base + r) & KK) == 0;
        const uint64_t a = e[r], b = e[pr];
        const bool sw = up ? (a > b) : (a < b);
        e[r] = sw ? b : a;
        e[pr] = sw ? a : b;
      }
    }
  } else if constexpr (J < 64 * R) {
    // keep_min = ((i & J) == 0) == ((i & KK) == 0) for i = wave 64R + lane R + r
    // is a constant lane pattern (J, and KK < 64R, select lane bits; KK >= 64R a
    // wave bit): the exchange is the compare's lane mask xnor that pattern
    constexpr uint64_t pat = keep_min_pattern<R, J, KK>();
    const bool wflip = (KK >= 64 * R) && (((wave_id() * 64 * R) & KK) != 0);  // wave-uniform
    const uint64_t keep = wflip ? ~pat : pat;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint64_t o = xshfl64<J / R>(e[r]);
      const uint64_t lt = wave_ballot(o < e[r]);
      e[r] = lane_select64(~(keep ^ lt), e[r], o);
    }
  } else {
    uint64_t* b = buf + (ib & 1) * n;  // alternate buffers: one barrier per stage
    ++ib;
#pragma unroll
    for (int r = 0; r < R; ++r) b[base + r] = e[r];
    lds_barrier();
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = base + r;
      const uint64_t o = b[i ^ J];
      const bool keep_min = ((i & J) == 0) == ((i & KK) == 0);
      const bool lt = o < e[r];
      e[r] = (keep_min == lt) ? o : e[r];
    }
  }
}
template <int NT, int R, int KK, int J>
struct Bitonic {
  __device__ static __forceinline__ void run(uint64_t (&e)[R], uint64_t* buf, int& ib) {
    bitonic_stage<NT, R, KK, J>(e, buf, ib);
    if constexpr (J > 1) Bitonic<NT, R, KK, J / 2>::run(e, buf, ib);
    else if constexpr (KK < 64 * (NT / 64) * R) Bitonic<NT, R, 2 * KK, KK>::run(e, buf, ib);
  }
};
// The order of Bitonic<64 NSW, 1, 2, 1> (ascending) of distinct keys, one per
// lane of the first NSW waves, by ranks: each wave sorts its 64 keys ascending
// (the network's stages KK <= 64, every wave in the final direction), the
// runs meet in buf[0, 64 NSW), and each key's position is its rank, the sum
// over the runs of the keys below it (its lane in its own run; a 7-probe
// binary search in the others, interleaved); buf[64 NSW, 128 NSW) receives the
// sorted keys. Two barriers and 21 in-wave stages in place
// of the network's three cross-wave stages and 33 in-wave stages. The other
// waves of the workgroup pass the same barriers and run `idle` between them.
template <int J, int KK>
__device__ __forceinline__ void rank_sort_stage(uint64_t& e) {
  constexpr uint64_t pat = keep_min_pattern<1, J, KK>();  // KK = 64: every wave as wave 0 (ascending)
  const uint64_t o = xshfl64<J>(e);
  const uint64_t lt = wave_ballot(o < e);
  e = lane_select64(~(pat ^ lt), e, o);
}
template <int J, int KK>
struct RankRuns {
  __device__ static __forceinline__ void run(uint64_t& e) {
    rank_sort_stage<J, KK>(e);
    if constexpr (J > 1) RankRuns<J / 2, KK>::run(e);
    else if constexpr (KK < 64) RankRuns<KK, 2 * KK>::run(e);
  }
};
template <int NSW, class Idle>
__device__ __forceinline__ uint64_t rank_sort_asc(uint64_t e, uint64_t* buf, bool sorter, Idle idle) {
  const int base = (int)(threadIdx.x >> 6) * 64 + lane_id();
  if (sorter) {
    RankRuns<1, 2>::run(e);
    buf[base] = e;
  }
  lds_barrier();
  if (!sorter) {
    idle();
  } else {
    int pos[NSW];
#pragma unroll
    for (int r = 0; r < NSW; ++r) pos[r] = 0;
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
#pragma unroll
      for (int r = 0; r < NSW; ++r) pos[r] += (buf[64 * r + pos[r] + step - 1] < e) ? step : 0;
    }
    int rank = 0;
#pragma unroll
    for (int r = 0; r < NSW; ++r) rank += pos[r] + ((buf[64 * r + pos[r]] < e) ? 1 : 0);
    buf[64 * NSW + rank] = e;
  }
  lds_barrier();
  return sorter ? buf[64 * NSW + base] : e;
}

// workgroup barriers of a bitonic sort of n keys held R per lane (one per
// cross-wave stage): the waves of a larger workgroup that take no part in the
// sort pass the same number of barriers
constexpr int bitonic_lds_stages(int n, int R) {
  int c = 0;
  for (int kk = 2; kk <= n; kk *= 2)
    for (int j = kk / 2; j >= 1; j /= 2) c += (j >= 64 * R) ? 1 : 0;
  return c;
}

// Sort A (nA keys in srt[]), exact prefix masses, the K / log c loop and the
// systematic draws. scr: the W + key areas (W is overwritten). The sort runs on
// the first NSW waves (64 NSW R keys); the other waves of the workgroup only
// pass its barriers.
template <int NT, int NSW, int R>
__device__ __forceinline__ int top_set_finish(uint64_t* srt, int nA, bool hasB, int N, int M, int cnt_fin, const hyg_u192& massB,
                              unsigned char* scr, int* parents, Shared& sh, const ConstLds& cl, unsigned char* red,
                              float Usys, unsigned long long* ph, bool timed, int pb) {
  static_assert(NSW <= NT / 64, "sorting waves");
  const int lane = lane_id();
  const bool sorter = (NSW == NT / 64) || wave_id() < NSW;  // wave-uniform
  const int base = (int)(threadIdx.x >> 6) * 64 * R + lane * R;
  uint64_t e[R];
  hyg_u192 f[R];
  hyg_u192 loc = hyg_u192_zero();
  if (sorter) {
#pragma unroll
    for (int r = 0; r < R; ++r) e[r] = (base + r < nA) ? srt[base + r] : ~0ull;
    int ib = 0;
    Bitonic<64 * NSW, R, 2, 1>::run(e, (uint64_t*)scr, ib);
    TPH(27);
    // (every wave loaded its keys before the first cross-wave barrier)
#pragma unroll
    for (int r = 0; r < R; ++r) srt[base + r] = e[r];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float m = hyg_expf(key_value(e[r]));
      f[r] = hyg_fix149f((base + r < nA) ? m : 0.0f);
      loc = hyg_u192_add(loc, f[r]);
    }
  } else {
    constexpr int nb = bitonic_lds_stages(64 * NSW * R, R);
#pragma unroll
    for (int i = 0; i < nb; ++i) lds_barrier();
#pragma unroll
    for (int r = 0; r < R; ++r) {
      e[r] = ~0ull;
      f[r] = hyg_u192_zero();
    }
  }
  hyg_u192 massA;
  // red's last readers (the previous step's block max) are behind this step's
  // barriers; its publishing barrier ends every sort-buffer read
  const hyg_u192 ex = block_excl192<NT, false>(loc, red, &massA);
  hyg_u192* pre = (hyg_u192*)scr;                           // inclusive prefix of sorted position p
  const hyg_u192 total = hyg_u192_add(massA, massB);         // every significant weight's mass
  hyg_u192 run = ex;
  if (sorter) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      run = hyg_u192_add(run, f[r]);
      if (base + r < nA) pre[base + r] = run;
    }
  }
  lds_barrier();
  TPH(28);
  if (wave_id() == 0) {
    serial_begin(pb);
    // lane a: c(a) (loop-variable semantics of :12-31); the loop's counts
    // P(c(a)) = #{p : fl(c(a) + x_p) > 0} are taken only at the iterates it
    // visits, by a ballot over the sorted keys x_p of positions p < min(nA, M)
    // (one per lane; M <= 64 on this path): the predicate is monotone in p,
    // so the count of true lanes is the first false position.
    const int a = lane;
    const int cap = nA < M ? nA : M;
    float xk;
    if constexpr (R == 1) xk = key_value(e[0]);  // wave 0 lane p holds sorted position p
    else xk = key_value(srt[lane < nA ? lane : 0]);
    const uint64_t capmask = (cap >= 64) ? ~0ull : ((1ull << cap) - 1ull);
    int flag = 0;
    float ca = 0.0f;
    hyg_u192 rva = hyg_u192_zero();
    if (a < M && a < N) {
      // (positions past the significant weights have zero mass, so R(a) = 0
      // there; outside the list nothing is significant)
      if (a <= nA) rva = hyg_u192_sub(total, a == 0 ? hyg_u192_zero() : pre[a - 1]);
      else if (hasB) flag = 1;  // prefix outside A
      const double rvd = hyg_u192_to_f64(rva);
      const float l2 = (rvd == 0.0) ? HYG_NINFF : (float)hyg_log(rvd);
      ca = cl.logMa[a] - l2;
    }
    TPH(30);
    int aa = 0, bb = -1, ovf = 0;
    while (aa != bb && aa < N && aa < M) {
      const float c = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ca), aa));
      int nxt = 0;
      if (hyg_isfinitef(c)) {  // uniform
        // (no weight below sig_thresh satisfies the predicate: c < log M + 103.3 there)
        nxt = (int)__builtin_popcountll(wave_ballot((float)(c + xk) > 0.0f) & capmask);
        if (nxt == nA && nA < M && hasB) ovf = 1;  // the count may continue below A
      } else if (c > 0.0f) {
        nxt = cnt_fin;  // +inf: every finite particle
      }
      ovf |= __builtin_amdgcn_readlane(flag, aa);
      bb = aa;
      aa = nxt > aa ? nxt : aa;
    }
    TPH(32);
    const float lc = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ca), bb));
    const hyg_u192 Rr = rdlane192(rva, bb);
    int status = FAST_DONE;
    if (ovf) {
      status = FAST_FALLBACK_REGEN;
    } else if (bb < N && hyg_isfinitef(lc)) {
      // systematic residual (:32-40, :56-69): target j lands on the first
      // sorted position p >= K with C(p) >= preK + ceil(T_j R)
      const int L = M - bb;
      const hyg_u192 preK = hyg_u192_sub(total, Rr);
      hyg_u192 tau = hyg_u192_zero();
      if (lane < L) tau = hyg_u192_add(preK, hyg_ceil_mul_f32_bf(((float)lane + Usys) / (float)L, Rr));
      const hyg_u192 tlast = rdlane192(tau, L > 0 ? L - 1 : 0);
      TPH(31);
      if (L > 0 && hasB && !hyg_u192_ge(massA, tlast)) {
        status = FAST_FALLBACK_REGEN;
      } else {
        if (lane < bb) parents[lane] = key_index(srt[lane]);
        if (lane < L) {
          int lo = bb, hi = nA - 1;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (hyg_u192_ge(pre[mid], tau)) hi = mid; else lo = mid + 1;
          }
          parents[bb + lane] = key_index(srt[lo]);
        }
        TPH(34);
      }
    }
    if (lane == 0) {
      sh.Kk = bb;
      sh.log_c = lc;
      sh.fast = status;
    }
    TPH(33);
    serial_end(pb);
  }
  lds_barrier();
  TPH(29);
  return sh.fast;
}

// u192 -> f64 to within a few ulp (a search estimate only: every decision it
// guides is checked exactly); the scale 2^-149 cancels in the ratios it forms
__device__ __forceinline__ double u192_approx(const hyg_u192& a) {
  auto w = [](uint64_t x) { return fma((double)(uint32_t)(x >> 32), 0x1p32, (double)(uint32_t)x); };
  return fma(w(a.w2), 0x1p128, fma(w(a.w1), 0x1p64, w(a.w0)));
}

// #{j in [0, L) : ceil(T_j R) <= v} for the systematic targets
// T_j = ((float)j + U) / (float)L (f32, as resampling_functions.py:58-67 forms
// them; Ttab[j] holds T_j): T_j R <= v is T_j <= v / R. The estimate
// j ~ (v / R) L - U is within 1e-5 of the exact threshold (T_j carries two f32
// roundings, v / R here a relative error below 2^-49), so every j < j0 counts
// and no j >= j0 + 2 does (j0 = floor of the estimate); the two candidates in
// between are compared in f64 with a 2^-46 guard band and, inside it, exactly
// in integers.
__device__ __forceinline__ int sys_count(const hyg_u192& v, const hyg_u192& R, double invR, int L, float U,
                                         const float* Ttab) {
  const double y = u192_approx(v) * invR;
  double jf = y * (double)L - (double)U;
  jf = jf < -1.0 ? -1.0 : (jf > (double)L ? (double)L : jf);
  const int j0 = (int)floor(jf);
  const double ylo = y * (1.0 - 0x1p-46), yhi = y * (1.0 + 0x1p-46);
  float T[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {  // loads first (one LDS round trip)
    const int j = j0 + k;
    T[k] = Ttab[j < 0 ? 0 : (j >= L ? L - 1 : j)];
  }
  int c = j0 > 0 ? j0 : 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int j = j0 + k;
    const double t = (double)T[k];
    bool le = t < ylo;
    if (!le && !(t > yhi) && j >= 0 && j < L) le = hyg_u192_ge(v, hyg_ceil_mul_f32_bf(T[k], R));  // exact
    c += (le && j >= 0 && j < L) ? 1 : 0;
  }
  return c;
}

// The value of the lane below (lane 0: `first`), DPP wave_shr:1.
__device__ __forceinline__ int wave_shr1(int v, int first) {
  return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false);
}

// LDS bytes of top_set_finish1's scratch: the sort's two exchange buffers,
// then the sorted masses' in-wave inclusive prefixes, then the targets T_j
template <int NSW>
constexpr size_t tsf1_bytes() { return 2 * 64 * NSW * sizeof(uint64_t) + 64 * NSW * sizeof(hyg_u192) + 64 * sizeof(float); }

// top_set_finish for one key per lane (sorter wave w, lane l: sorted position
// 64 w + l), shaped for latency: after the sort each sorting wave scans its
// own masses and publishes its total (one barrier, no block scan); wave 0 then
// runs the K loop on its own prefixes and finds the systematic targets by
// counting them per sorted position (sys_count), 64 positions per pass, from
// the first kept position on, instead of a binary search per target. Same
// parents, Kk, log c and fallback decisions as top_set_finish.
// The outside masses of the lists, for top_set_finish1<.., SPLIT = true>:
// the lists hold the outside log-weights (f32 bits, -inf inside A).
struct ListsB {
  const int* lst;        // wave w's list at lst[w * stride], part_cnt[w * kNCut + kNCut - 1] entries
  int stride;
  const int* part_cnt;
  hyg_u192* part_tot;    // one partial per non-sorting wave
  bool narrow;           // every outside mass below e^-20, <= kNarrowPerLane images per lane: u128 sums
                         // (a lane sums up to 2 ceil(N / NT) images: two lists)
};
// Exact image sum of the f32 masses exp(lw) of list w (lane-strided, two
// entries per lane in flight).
__device__ __forceinline__ void list_mass(const ListsB& lb, int w, hyg_u128& n128, hyg_u192& m192) {
  const int cnt = lb.part_cnt[w * kNCut + kNCut - 1];
  const int* L = lb.lst + w * lb.stride;
  const int lane = lane_id();
  for (int b = 0; b < cnt; b += 128) {  // cnt is wave-uniform
    const int i0 = b + lane, i1 = b + 64 + lane;
    const float x0 = __builtin_bit_cast(float, L[i0 < cnt ? i0 : b]);
    const float x1 = __builtin_bit_cast(float, L[i1 < cnt ? i1 : b]);
    const float m0 = (i0 < cnt) ? hyg_expf(x0) : 0.0f, m1 = (i1 < cnt) ? hyg_expf(x1) : 0.0f;
    if (lb.narrow) {
      n128 = hyg_u128_add(n128, hyg_u128_add(hyg_fix149f_low128(m0), hyg_fix149f_low128(m1)));
    } else {
      m192 = hyg_u192_add(m192, hyg_u192_add(hyg_fix149f(m0), hyg_fix149f(m1)));
    }
  }
}

// The ancestors gathered ahead by sorted position. While wave 0 runs the
// serial section of top_set_finish1 (c(a), the K loop, the systematic search),
// the other waves compute, for the sorted positions [0, n), exactly what the
// forward's gather computes for a parent at that position (state, weight, own
// hazards) and park it by position; wave 0 publishes each parent's sorted
// position beside its index, and the gather copies the parked entry of a
// position below n. pos[] is the sort's first exchange buffer (dead behind the
// sort's second barrier); the parked entries follow top_set_finish1's scratch,
// in bytes of the W / key areas that are dead there: the weights are
// overwritten by the sort already (every fallback behind that point
// regenerates them before it reads them or uses the key area), and the
// candidate lists were last read before the barrier that starts the section.
struct Ahead {
  int* pos;      // [M]: the sorted position of parent a
  uint64_t* st;  // [n], by sorted position: the ancestor's state,
  double* w;     // its weight
  Hz4* hz;       // and its own hazards
  int n;         // positions gathered ahead (0: none)
};
template <int NT, int NSW>
__device__ __forceinline__ Ahead ahead_area(unsigned char* scr, size_t scr_bytes, int window) {
  constexpr size_t used = (tsf1_bytes<NSW>() + 15) / 16 * 16;
  constexpr size_t per = sizeof(uint64_t) + sizeof(double) + sizeof(Hz4);
  int n = scr_bytes > used ? (int)((scr_bytes - used) / per) : 0;
  n = n < window ? n : window;
  n = n < 64 * (NT / 64 - 1) ? n : 64 * (NT / 64 - 1);  // one position per lane of the waves behind wave 0
  Ahead a;
  a.pos = (int*)scr;
  a.st = (uint64_t*)(scr + used);
  a.w = (double*)(scr + used + sizeof(uint64_t) * n);
  a.hz = (Hz4*)(scr + used + (sizeof(uint64_t) + sizeof(double)) * n);
  a.n = n > 0 ? n : 0;
  return a;
}

enum { FAST_DONE_AHEAD = 3 };  // FAST_DONE with the parents' sorted positions published (Ahead)

template <int NT, int NSW, bool SPLIT, class Anc>
__device__ __forceinline__ int top_set_finish1(uint64_t* srt, int nA, bool hasB, int N, int M, int cnt_fin,
                                               const hyg_u192& massB_in, unsigned char* scr, int* parents,
                                               Shared& sh, const ConstLds& cl, unsigned char* red, float Usys,
                                               const ListsB& lb, const Ahead& ah, Anc ancestor_of,
                                               unsigned long long* ph, bool timed, int pb) {
  static_assert(NSW <= NT / 64 && NSW <= 4, "sorting waves");
  constexpr int NW = NT / 64, NNS = NW - NSW;
  static_assert(!SPLIT || NNS >= NSW, "the outside masses need idle waves");
  const int lane = lane_id();
  const bool sorter = (NSW == NT / 64) || wave_id() < NSW;  // wave-uniform
  const int base = (int)(threadIdx.x >> 6) * 64 + lane;
  hyg_u192* preL = (hyg_u192*)(scr + 2 * 64 * NSW * sizeof(uint64_t));  // past the sort buffers
  hyg_u192* wtot = (hyg_u192*)red;  // red's last readers are behind this step's barriers
  uint64_t e[1];
  hyg_u192 f = hyg_u192_zero(), inc = hyg_u192_zero();
  if (sorter) {
    // (distinct pads above every key past nA: the rank sort needs distinct keys)
    e[0] = (base < nA) ? srt[base] : ~0ull - (uint64_t)base;
    e[0] = rank_sort_asc<NSW>(e[0], (uint64_t*)scr, true, []() {});
    TPH(27);
    // (every wave loaded its keys before the sort's first barrier)
    srt[base] = e[0];
    const float m = hyg_expf(key_value(e[0]));
    f = hyg_fix149f((base < nA) ? m : 0.0f);
    inc = wave_incl192(f);
    preL[base] = inc;
    if (lane == 63) wtot[wave_id()] = inc;
  } else {
    // SPLIT: the waves that do not sort sum the outside masses meanwhile,
    // wave NSW + v the lists v and v + NNS (NW <= 2 NNS): the first while the
    // sorting waves sort their runs, the second while they search the ranks
    // (between the sort's two barriers)
    static_assert(!SPLIT || NW <= 2 * NNS, "two lists per idle wave");
    hyg_u128 n128 = hyg_u128_zero();
    hyg_u192 m192 = hyg_u192_zero();
    const int v = wave_id() - NSW;
    if (SPLIT && hasB) list_mass(lb, v, n128, m192);  // uniform
    (void)rank_sort_asc<NSW>(0, (uint64_t*)scr, false, [&]() {
      if (SPLIT && hasB && v + NNS < NW) list_mass(lb, v + NNS, n128, m192);
    });
    if (SPLIT && hasB) {
      if (lb.narrow) { m192.w0 = n128.lo; m192.w1 = n128.hi; m192.w2 = 0; }
      const hyg_u192 ws = wave_sum192(m192);
      if (lane == 0) lb.part_tot[v] = ws;
    }
    e[0] = ~0ull;
  }
  lds_barrier();
  TPH(28);
  if (wave_id() == 0) {
    serial_begin(pb);
    hyg_u192 massA = hyg_u192_zero();
#pragma unroll
    for (int w = 0; w < NSW; ++w) massA = hyg_u192_add(massA, wtot[w]);
    hyg_u192 massB = massB_in;
    if (SPLIT && hasB) {
#pragma unroll
      for (int w = 0; w < NNS; ++w) massB = hyg_u192_add(massB, lb.part_tot[w]);
    }
    const hyg_u192 total = hyg_u192_add(massA, massB);  // every significant weight's mass
    // lane a: c(a) (loop-variable semantics of :12-31) from the suffix mass
    // total - C(a - 1), C(a - 1) = this lane's exclusive prefix
    const int a = lane;
    const float xk = key_value(e[0]);
    const int cap = nA < M ? nA : M;
    const uint64_t capmask = (cap >= 64) ? ~0ull : ((1ull << cap) - 1ull);
    int flag = 0;
    float ca = 0.0f;
    hyg_u192 rva = hyg_u192_zero();
    if (a < M && a < N) {
      if (a <= nA) rva = hyg_u192_sub(total, hyg_u192_sub(inc, f));
      else if (hasB) flag = 1;  // prefix outside A
      const double rvd = hyg_u192_to_f64(rva);
      const float l2 = (rvd == 0.0) ? HYG_NINFF : (float)hyg_log(rvd);
      ca = cl.logMa[a] - l2;
    }
    TPH(30);
    int aa = 0, bb = -1, ovf = 0;
    while (aa != bb && aa < N && aa < M) {
      const float c = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ca), aa));
      int nxt = 0;
      if (hyg_isfinitef(c)) {  // uniform
        nxt = (int)__builtin_popcountll(wave_ballot((float)(c + xk) > 0.0f) & capmask);
        if (nxt == nA && nA < M && hasB) ovf = 1;  // the count may continue below A
      } else if (c > 0.0f) {
        nxt = cnt_fin;  // +inf: every finite particle
      }
      ovf |= __builtin_amdgcn_readlane(flag, aa);
      bb = aa;
      aa = nxt > aa ? nxt : aa;
    }
    TPH(32);
    const float lc = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ca), bb));
    int status = FAST_DONE;
    if (ovf) {
      status = FAST_FALLBACK_REGEN;
    } else if (bb < N && hyg_isfinitef(lc)) {
      // (bb < nA here: bb > nA sets ovf, and bb = nA leaves a zero residual
      // mass when nothing lies outside A, so log c is infinite)
      if (lane < bb) parents[lane] = key_index(e[0]);
      if (ah.n > 0 && lane < bb) ah.pos[lane] = lane;  // (uniform) a kept parent sits at its own position
      const int L = M - bb;
      TPH(31);
      if (L > 0) {
        // systematic residual (:32-40, :56-69): target j lands on the first
        // sorted position p >= K with C(p) >= preK + ceil(T_j R); position p
        // takes the targets j in [count(C(p - 1)), count(C(p)))
        const hyg_u192 Rr = rdlane192(rva, bb);
        const double invR = 1.0 / u192_approx(Rr);
        const hyg_u192 preK = hyg_u192_sub(total, Rr);
        float* Ttab = (float*)(scr + tsf1_bytes<NSW>() - 64 * sizeof(float));
        if (lane < L) Ttab[lane] = ((float)lane + Usys) / (float)L;
        wave_lds_sync();
        // C at the start of each sorting wave's positions
        hyg_u192 wb[NSW];
        wb[0] = hyg_u192_zero();
#pragma unroll
        for (int w = 1; w < NSW; ++w) wb[w] = hyg_u192_add(wb[w - 1], wtot[w - 1]);
        int cprev = 0;
        // 64 positions per pass from the first kept one on (the deepest
        // target sits about 60 positions past it at C3: mostly one pass)
#pragma unroll
        for (int i = 0; i < NSW; ++i) {
          const int p0 = bb + 64 * i;
          if (p0 >= nA || cprev >= L) break;  // uniform
          const int p = p0 + lane;
          const int pc = p < nA ? p : nA - 1;  // past A: the count of its last position
          const int wp = pc >> 6;
          hyg_u192 C = preL[pc];
#pragma unroll
          for (int w = 1; w < NSW; ++w)
            if (wp == w) C = hyg_u192_add(C, wb[w]);
          const uint64_t key = srt[pc];
          const int cnt = sys_count(hyg_u192_sub(C, preK), Rr, invR, L, Usys, Ttab);
          const int cex = wave_shr1(cnt, cprev);
          for (int j = cex; j < cnt; ++j) parents[bb + j] = key_index(key);
          if (ah.n > 0)
            for (int j = cex; j < cnt; ++j) ah.pos[bb + j] = pc;
          cprev = __builtin_amdgcn_readlane(cnt, 63);
        }
        // targets past A: only when weights lie outside it
        if (cprev < L) status = FAST_FALLBACK_REGEN;
      }
      TPH(34);
    }
    if (lane == 0) {
      sh.Kk = bb;
      sh.log_c = lc;
      sh.fast = (status == FAST_DONE && ah.n > 0) ? FAST_DONE_AHEAD : status;
    }
    TPH(33);
    serial_end(pb);
  } else if (ah.n > 0) {  // uniform
    // the ancestors of the sorted positions [0, ah.n), one per lane of the
    // waves behind wave 0 (see Ahead); a step that falls back, or draws its
    // parents otherwise, leaves them unread
    const int p = (wave_id() - 1) * 64 + lane;
    if (p < ah.n && p < nA) {
      uint64_t s;
      double w;
      Hz4 h;
      ancestor_of(key_index(srt[p]), s, w, h);
      ah.st[p] = s;
      ah.w[p] = w;
      ah.hz[p] = h;
    }
  }
  lds_barrier();
  TPH(29);
  return sh.fast;
}

// Top-set path of OptimalFiniteState; returns FAST_DONE (parents / Kk /
// log_c written; log_c infinite -> the caller's unbiased fallback),
// FAST_FALLBACK (W intact) or FAST_FALLBACK_REGEN (W overwritten). The
// counts of the cutoff sets per wave (part_cnt) were published with the
// candidate lists before the log-sum-exp reduction.
// FINE (kFineLists) and `fine`: the list is walked per 64 entries (list_walk).
template <int NT, int NSW, bool FINE, class Anc>
__device__ __forceinline__ int top_set_resample(const double* W, int N, double mx, double logS, int* lst, int lb, int cw,
                                bool fine,
                                unsigned char* scr, size_t scr_bytes, uint64_t* srt, size_t srt_bytes,
                                const int* part_cnt, hyg_u192* part_tot, int* parents, Shared& sh,
                                const ConstLds& cl, unsigned char* red, int M, int cnt_fin, float Usys,
                                int rmax, const Ahead& ah, Anc ancestor_of, unsigned long long* ph, bool timed, int pb) {
  constexpr int NW = NT / 64;
  const int wv = wave_id(), lane = lane_id();
  // ---- 1. the most inclusive cutoff whose set A fits the sort
  // one LDS read per lane per 8 waves (lane w * kNCut + k holds wave w's count
  // at cutoff k, waves 8-15 in a second register), the per-cutoff totals by
  // xor shuffles (every lane l gets cutoff l % 8)
  static_assert(kNCut == 8 && NW * kNCut <= 128, "cutoff counts: one or two per lane");
  const int pc = (lane < NW * kNCut) ? part_cnt[lane] : 0;
  const int pc2 = (NW * kNCut > 64 && lane + 64 < NW * kNCut) ? part_cnt[lane + 64] : 0;
  int c = pc + pc2;
  c += (int)xshfl32<8>((uint32_t)c);
  c += (int)xshfl32<16>((uint32_t)c);
  c += (int)xshfl32<32>((uint32_t)c);
  const int np = (c <= 64 * NSW) ? 64 * NSW : 128 * NSW;
  const bool fits = lane < kNCut && c <= 64 * NSW * rmax && (size_t)np * sizeof(hyg_u192) <= scr_bytes &&
                    (size_t)np * 8 <= srt_bytes;
  const uint64_t fm = wave_ballot(fits);
  const int nL = __builtin_amdgcn_readlane(c, kNCut - 1);
  if (threadIdx.x == 0) sh.n_sig = nL;
  if (fm == 0) return FAST_FALLBACK;  // uniform
  const int ks = 63 - __builtin_clzll(fm);  // the most inclusive cutoff that fits
  const int nA = __builtin_amdgcn_readlane(c, ks);
  const bool hasB = nA < nL;         // list weights outside A (their masses enter the total)
  const double cutx = (ks == kNCut - 1) ? HYG_NINF : -cut_below_top(ks);
  int off = 0;
  for (int w = 0; w < wv; ++w)
    off += __builtin_amdgcn_readlane(w < 8 ? pc : pc2, (w & 7) * kNCut + ks);
  // ---- 2. gather A's keys; exact mass of the list weights outside A. From the
  // third cutoff on (X >= 20 nats below the top: every outside mass is below
  // e^-20 < 2^-28.8, its image m 2^149 below 2^120.2, and a lane sums at most
  // ceil(N / NT) <= 128 of them, below 2^127.2) a lane's images are formed and
  // summed as u128.
  const bool narrow = ks >= kNarrowCut && (N + NT - 1) / NT <= kNarrowPerLane;
  // SPLIT (workgroups with at least as many idle waves as sorting ones): the
  // lists take the outside log-weights back and the idle waves sum their
  // masses during the sort (top_set_finish1)
  constexpr int NNS = NW - NSW;
  constexpr bool kSplitB = NSW <= 4 && NNS >= NSW;
  const bool split = kSplitB && nA <= 64 * NSW && scr_bytes >= tsf1_bytes<NSW>();
  hyg_u192 mb = hyg_u192_zero(), mb2 = hyg_u192_zero();
  hyg_u128 nb = hyg_u128_zero(), nb2 = hyg_u128_zero();
  constexpr int kLR = kLRof<NT>;
  // (kFineLists builds; the others run the written-out copy in the else branch below: change the two together)
  [[maybe_unused]] auto gather = [&](auto rc, int b) {  // R entries per lane from entry b on, loads first (see the lse loop)
    constexpr int R = decltype(rc)::value;
    int nn[R];
    float lw[R];
    bool inA[R], outA[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = b + r * 64 + lane;
      nn[r] = lst[lb + (i < cw ? i : b)];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const bool v = b + r * 64 + lane < cw;
      const double x = W[nn[r]] - mx;
      lw[r] = (float)(x - logS);
      inA[r] = v && x >= cutx;
      outA[r] = v && !inA[r];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint64_t bal = wave_ballot(inA[r]);
      if (inA[r]) srt[off + lanes_below(bal)] = sort_key(lw[r], nn[r]);
      off += (int)__builtin_popcountll(bal);
    }
    if (split) {
      if (hasB) {
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (b + r * 64 + lane < cw) lst[lb + b + r * 64 + lane] = __builtin_bit_cast(int, outA[r] ? lw[r] : HYG_NINFF);
      }
    } else if (hasB && narrow) {  // uniform; expf(lw) is 0 below sig_thresh
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float m = hyg_expf(lw[r]);
        const hyg_u128 f = hyg_fix149f_low128(outA[r] ? m : 0.0f);
        if (r & 1) nb2 = hyg_u128_add(nb2, f); else nb = hyg_u128_add(nb, f);
      }
    } else if (hasB) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float m = hyg_expf(lw[r]);
        const hyg_u192 f = hyg_fix149f(outA[r] ? m : 0.0f);
        if (r & 1) mb2 = hyg_u192_add(mb2, f); else mb = hyg_u192_add(mb, f);
      }
    }
  };
  if constexpr (FINE) {
    list_walk<kLR>(cw, fine, gather);
  } else {
    // (the other builds keep the loop written out: their code is what it was, register for
    // register; called through the lambda their spills move. This is `gather` above at R = kLR,
    // statement for statement: change the two together)
    for (int b = 0; b < cw; b += 64 * kLR) {  // kLR entries per lane, loads first (see the lse loop)
      int nn[kLR];
      float lw[kLR];
      bool inA[kLR], outA[kLR];
#pragma unroll
      for (int r = 0; r < kLR; ++r) {
        const int i = b + r * 64 + lane;
        nn[r] = lst[lb + (i < cw ? i : b)];
      }
#pragma unroll
      for (int r = 0; r < kLR; ++r) {
        const bool v = b + r * 64 + lane < cw;
        const double x = W[nn[r]] - mx;
        lw[r] = (float)(x - logS);
        inA[r] = v && x >= cutx;
        outA[r] = v && !inA[r];
      }
#pragma unroll
      for (int r = 0; r < kLR; ++r) {
        const uint64_t bal = wave_ballot(inA[r]);
        if (inA[r]) srt[off + lanes_below(bal)] = sort_key(lw[r], nn[r]);
        off += (int)__builtin_popcountll(bal);
      }
      if (split) {
        if (hasB) {
#pragma unroll
          for (int r = 0; r < kLR; ++r)
            if (b + r * 64 + lane < cw) lst[lb + b + r * 64 + lane] = __builtin_bit_cast(int, outA[r] ? lw[r] : HYG_NINFF);
        }
      } else if (hasB && narrow) {  // uniform; expf(lw) is 0 below sig_thresh
#pragma unroll
        for (int r = 0; r < kLR; ++r) {
          const float m = hyg_expf(lw[r]);
          const hyg_u128 f = hyg_fix149f_low128(outA[r] ? m : 0.0f);
          if (r & 1) nb2 = hyg_u128_add(nb2, f); else nb = hyg_u128_add(nb, f);
        }
      } else if (hasB) {
#pragma unroll
        for (int r = 0; r < kLR; ++r) {
          const float m = hyg_expf(lw[r]);
          const hyg_u192 f = hyg_fix149f(outA[r] ? m : 0.0f);
          if (r & 1) mb2 = hyg_u192_add(mb2, f); else mb = hyg_u192_add(mb, f);
        }
      }
    }
  }
  if constexpr (kSplitB) {
    if (split) {
      lds_barrier();  // the keys of A and the lists' log-weights
      TPH(26);
      ListsB lbs;
      lbs.lst = lst;
      lbs.stride = ((N + NT - 1) / NT) * 64;
      lbs.part_cnt = part_cnt;
      lbs.part_tot = part_tot;
      lbs.narrow = ks >= kNarrowCut && 2 * ((N + NT - 1) / NT) <= kNarrowPerLane;
      return top_set_finish1<NT, NSW, kSplitB>(srt, nA, hasB, N, M, cnt_fin, hyg_u192_zero(), scr, parents, sh, cl,
                                               red, Usys, lbs, ah, ancestor_of, ph, timed, pb);
    }
  }
  if (hasB) {
    if (narrow) {
      const hyg_u128 t = hyg_u128_add(nb, nb2);
      mb.w0 = t.lo; mb.w1 = t.hi; mb.w2 = 0;
    } else {
      mb = hyg_u192_add(mb, mb2);
    }
    const hyg_u192 ws = wave_sum192(mb);
    if (lane == 0) part_tot[wv] = ws;
  }
  lds_barrier();
  hyg_u192 massB = hyg_u192_zero();
  if (hasB) massB = sum_waves192<NW>(part_tot);
  TPH(26);
  if (nA <= 64 * NSW) {
    if constexpr (NSW <= 4)
      if (scr_bytes >= tsf1_bytes<NSW>())
        return top_set_finish1<NT, NSW, false>(srt, nA, hasB, N, M, cnt_fin, massB, scr, parents, sh, cl, red, Usys,
                                               ListsB{}, ah, ancestor_of, ph, timed, pb);
    return top_set_finish<NT, NSW, 1>(srt, nA, hasB, N, M, cnt_fin, massB, scr, parents, sh, cl, red, Usys, ph, timed, pb);
  }
  return top_set_finish<NT, NSW, 2>(srt, nA, hasB, N, M, cnt_fin, massB, scr, parents, sh, cl, red, Usys, ph, timed, pb);
}
#undef TPH

}  // namespace hyg
