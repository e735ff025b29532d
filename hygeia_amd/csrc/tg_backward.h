// tg_backward.h -- tg_backward_kernel, the backward simulation of the
// two-group chain kernels, with the children of an ancestor (Child,
// trans_possible) and the random bits of its draws (backward_bits).
#pragma once

#include "tg_forward.h"

namespace hyg {

// ------------------------------------------------- backward-kernel rows
// Child of an ancestor (registers) in proposal slot s (wave-uniform), with the
// child's own hazard rows, exactly as tg_xi + child_hz produce them.
struct Child {
  int m, dc, rc, dk, rk;
  Hz4 h;
};
__device__ __forceinline__ Child child_of(const ConstLds& cl, int K, int am, int adc, int arc, int adk, int ark,
                                          const Pf3& p, int s) {
  Child x;
  // c_cont / k_cont: the child's duration continues on the ancestor's
  // prefetched row; merge (m = 0): case continues on the control row; every
  // other row is the d = 1 row of the child's own regime
  bool c_cont, k_cont, merge = false;
  if (s == 0) {
    x.m = am; x.dc = adc + 1; x.rc = arc; x.dk = adk + 1; x.rk = ark;
    c_cont = true; k_cont = true;
  } else if (s < K) {
    const int r = (s - 1 < ark) ? s - 1 : s;
    x.m = 0; x.dc = 1; x.rc = r; x.dk = adk + 1; x.rk = ark;
    c_cont = false; k_cont = true;
  } else if (s < 2 * K - 1) {
    const int qq = s - K;
    const int r = (qq < arc) ? qq : qq + 1;
    x.m = 0; x.dc = adc + 1; x.rc = arc; x.dk = 1; x.rk = r;
    c_cont = true; k_cont = false;
  } else if (s == 2 * K - 1) {
    const int d = (am == 0) ? adc + 1 : 0;
    x.m = 1; x.dc = d; x.rc = arc; x.dk = d; x.rk = arc;
    merge = am == 0;
    c_cont = merge; k_cont = false;
  } else {
    const int j = s - 2 * K, i = j / K, jj = j - i * K;
    x.m = (i == jj); x.dc = 1; x.rc = i; x.dk = 1; x.rk = jj;
    c_cont = false; k_cont = false;
  }
  // value selects (a select of addresses would put p in scratch memory)
  const double2 h1c = cl.hz1[0][x.rc], h1k = cl.hz1[1][x.rk];
  x.h.lrc = c_cont ? p.c1.x : h1c.x;
  x.h.l1c = c_cont ? p.c1.y : h1c.y;
  x.h.lrk = merge ? p.kc.x : (k_cont ? p.k1.x : h1k.x);
  x.h.l1k = merge ? p.kc.y : (k_cont ? p.k1.y : h1k.y);
  return x;
}
// false when tg_trans(x -> next) selects a constant -inf branch whatever the
// table values (the selected value is then -inf; true leaves it to the values)
__device__ __forceinline__ bool trans_possible(int u, const Child& x, int mn, int dcn, int rcn, int dkn, int rkn) {
  const bool lm = ((x.dk < x.dc ? x.dk : x.dc) >= u) || (mn == x.m);
  const bool lc = (dcn == 1) || (dcn == x.dc + 1 && rcn == x.rc);
  bool lk;
  if (mn == 1) lk = (rkn == rcn && dkn == dcn);
  else if (x.m == 1 && dcn != 1) lk = (dkn == 1 && rkn != rcn);
  else if (rcn == x.rk && x.m == 0) lk = (dkn == 1 && rkn != rcn);
  else lk = (dkn == 1) ? (rkn != rcn && rkn != x.rk) : (dkn == x.dk + 1 && rkn == x.rk);
  return lm && lc && lk;
}

// The random bits of step t's B backward draws, hyg_rand64(seed, chain,
// BACKWARD, t, b) for b < B (Philox blocks of 4, one lane per block), into
// rb[0..B); run by one otherwise idle wave one step ahead of their use.
__device__ __forceinline__ void backward_bits(uint64_t* rb, int B, int t, uint64_t seed, uint64_t chain_id) {
  const int q = lane_id();
  if (4 * q < B) {
    const hyg_ph4 r = hyg_philox4x64((uint64_t)HYG_RNG_BACKWARD, (uint64_t)t, (uint64_t)q, 0, seed, chain_id);
    rb[4 * q + 0] = r.v[0]; rb[4 * q + 1] = r.v[1]; rb[4 * q + 2] = r.v[2]; rb[4 * q + 3] = r.v[3];
  }
}

// GW: the full-N weights (the final step's draw and the general path) live in
// the chain's global scratch (ChainDev::wg_offset of `wscr`, the same workspace
// as `ws`, disjoint bytes) instead of LDS, whose W area then holds the lists
// alone (make_layout gw): several chains per CU at the C5 shape. Global W is
// handed between threads behind __syncthreads (its vmcnt(0) release), only on
// the steps that build it.
// MM: the chain's model from the launch's table (see tg_forward_kernel).
template <int NT, int KC = 0, int MC = 0, int BC = 0, bool PHS = false, bool GW = false,  // KC > 0: one model shape (see tg_forward_kernel)
          bool MM = false>
__global__ void __launch_bounds__(NT, (NT == 512 ? 1 : 3))
tg_backward_kernel(ModelArg<MM> md_arg, const ChainDev* __restrict__ chains, const double* __restrict__ E,
                   const uint8_t* __restrict__ ws, const int32_t* status_in, int16_t* __restrict__ o_merged,
                   int16_t* __restrict__ o_control, int16_t* __restrict__ o_case, float* __restrict__ o_split,
                   float* __restrict__ o_regime, int32_t* status_out, Lay lay_arg,
                   unsigned long long* __restrict__ dbg_arg, uint8_t* __restrict__ wscr) {
  unsigned long long* __restrict__ const dbg = PHS ? dbg_arg : nullptr;  // (see tg_forward_kernel)
  const ModelDev md = model_of(md_arg, chains, blockIdx.x);
  const hyg_tg_consts* __restrict__ c = md.consts;
  const int K = KC ? KC : c->K, M = KC ? MC : c->M, B = KC ? BC : c->B, I = KC ? 2 * KC + KC * KC : c->I,
            K2 = 2 * K, tid = threadIdx.x;
  const Lay lay = KC ? make_layout(KC, MC, BC, MC * (2 * KC + KC * KC), NT, true, GW) : lay_arg;
  const int Lcap = lay.lcap;  // doubles of the list area (Nmax without GW)
  const ChainDev ch = chains[blockIdx.x];
  const int T = ch.T;
  if (status_in[blockIdx.x] != HYG_OK) return;  // uniform
  extern __shared__ __align__(16) unsigned char smem[];
  double* W;
  if constexpr (GW) W = (double*)(wscr + ch.wg_offset);
  else W = (double*)(smem + lay.W);
  // a barrier behind which every thread's W writes are visible (LDS: the
  // LDS-only barrier; global W: a workgroup release of the stores)
  auto w_barrier = [&]() {
    if constexpr (GW) __syncthreads();
    else lds_barrier();
  };
  double* Lg = (double*)(smem + lay.L);
  uint64_t* pst = (uint64_t*)(smem + lay.pst);
  double* pw = (double*)(smem + lay.pw);
  Hz4* phz = (Hz4*)(smem + lay.phz);
  Pf3* pf = (Pf3*)(smem + lay.pf);
  double* ering = (double*)(smem + lay.ering);
  ConstLds& cl = *(ConstLds*)(smem + lay.cl);
  hyg_u128* cp128 = (hyg_u128*)(smem + lay.cp);
  int* idx = (int*)(smem + lay.parents);
  uint64_t* X = (uint64_t*)(smem + lay.X);
  int* grp = (int*)(smem + lay.grp);
  uint64_t* gst = (uint64_t*)(smem + lay.gst);
  uint64_t* rb = (uint64_t*)(smem + lay.rb);
  uint64_t* xo = (uint64_t*)(smem + lay.xo);
  unsigned char* red = smem + lay.red;
  Shared& sh = *(Shared*)(smem + lay.sh);
  // Trajectories and test-function means of time tt
  // (run_inference_two_groups.py:233-240, 294-314) from the states wave 0
  // sampled (xo[tt & 1]), one wave, trajectory b on lane b (B <= 64). From 128
  // threads on they are written by wave 1 during the next step's draw, off
  // wave 0's serial path (deferred by one step; the state buffer is double).
  constexpr int kOutWave = NT >= 128 ? 1 : 0;
  auto write_outputs = [&](int tt) {
    const int lane = lane_id();
    const bool v = lane < B;
    uint64_t x = 0;
    if (v) {
      x = xo[(tt & 1) * B + lane];
      const size_t o = (size_t)(ch.out_begin + tt) * B + lane;
      o_merged[o] = (int16_t)hyg_st_m(x);
      o_control[2 * o + 0] = (int16_t)hyg_st_dc(x);
      o_control[2 * o + 1] = (int16_t)hyg_st_rc(x);
      o_case[2 * o + 0] = (int16_t)hyg_st_dk(x);
      o_case[2 * o + 1] = (int16_t)hyg_st_rk(x);
    }
    int myc = __builtin_popcountll(__ballot(v && hyg_st_m(x) == 0));
    for (int r = 0; r < K; ++r) {
      const int cc = __builtin_popcountll(__ballot(v && hyg_st_rc(x) == r));
      const int ck = __builtin_popcountll(__ballot(v && hyg_st_rk(x) == r));
      myc = (lane == 1 + r) ? cc : ((lane == 1 + K + r) ? ck : myc);
    }
    if (lane < 2 * K + 1) {
      const float vv = (float)myc / (float)B;
      if (lane == 0) o_split[ch.out_begin + tt] = vv;
      else o_regime[(size_t)(ch.out_begin + tt) * K2 + (lane - 1)] = vv;
    }
  };
  int pend = -1;  // the time whose outputs are still to be written (B <= 64)

  const uint8_t* rec0 = ws + ch.ws_offset;
  const size_t rstride = record_bytes(M);
  const double* Ech = E + ch.site_begin * K2;
  load_consts(cl, c, md);
  if (tid == 0) sh.status = HYG_OK;
  unsigned long long* ph_acc = sh.ph;
  if (tid < kPh) ph_acc[tid] = 0;
#define BPH(k)                                                     \
  if (dbg && tid == 0) {                                           \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
    ph_acc[k] += now_ - ph_acc[kPh - 1];                                \
    ph_acc[kPh - 1] = now_;                                             \
  }
  // Records are read ahead in two stages: step t consumes record t from LDS,
  // stores record t-1 (read during step t+1) with its hazard rows (issued at
  // the top of step t), and issues the read of record t-2.
  auto rec_ptr = [&](int tt) { return rec0 + (size_t)tt * rstride; };
  StepScalars s = *(const StepScalars*)rec_ptr(T - 1);
  if (tid < s.n_par) {
    const int o0 = ((T - 1) & 1) * M + tid;  // record t lives in LDS buffer t & 1
    const uint64_t* rst = (const uint64_t*)(rec_ptr(T - 1) + sizeof(StepScalars));
    const uint64_t st = rst[tid];
    pst[o0] = st;
    pw[o0] = ((const double*)(rst + M))[tid];
    const double2 hc = hz_at(md, K, 0, hyg_st_rc(st), hyg_st_dc(st));
    const double2 hk = hz_at(md, K, 1, hyg_st_rk(st), hyg_st_dk(st));
    Hz4 h;
    h.lrc = hc.x; h.l1c = hc.y; h.lrk = hk.x; h.l1k = hk.y;
    phz[o0] = h;
    pf[o0] = prefetch_rows(md, K, st);
  }
  // The record pipeline of the steps below (the reads of records t-1 / t-2,
  // the hazard rows of record t-1's ancestors and its LDS store) is the last
  // wave's work when M <= 64, ancestor a on its lane a: that wave has no slot
  // of its own in the list phase at 8 waves (d_c >= 3: K + 1 slots), so the
  // loads leave the waves whose list work the draw waits for. Otherwise thread
  // a holds ancestor a.
  const int ra = (M <= 64 && NT >= 128) ? ((wave_id() == NT / 64 - 1) ? lane_id() : M) : tid;
  // stage-1 registers: record t-1
  StepScalars s1{};
  uint64_t st1 = 0;
  double w1 = 0.0;
  if (T >= 2) {
    s1 = *(const StepScalars*)rec_ptr(T - 2);
    if (ra < M) {
      const uint64_t* rst = (const uint64_t*)(rec_ptr(T - 2) + sizeof(StepScalars));
      st1 = rst[ra];
      w1 = ((const double*)(rst + M))[ra];
    }
  }
  {
    const int bi = (T - 1) / kEBlock;
    load_eblock(ering, Ech, bi, T, K2, NT);
    if (bi > 0) load_eblock(ering, Ech, bi - 1, T, K2, NT);
  }
  lds_barrier();
  if (dbg && tid == 0) ph_acc[kPh - 1] = __builtin_amdgcn_s_memtime();

  for (int t = T - 1; t >= 0; --t) {
    // ---- regenerate the particles of step t from its record (LDS buffer t & 1;
    //      record t-1 is stored into the other buffer during this step)
    const int bt = t & 1;
    const double* Et = erow(ering, t, K2);
    const int np = s.n_par;
    const uint64_t* P = pst + bt * M;
    const double* PW = pw + bt * M;
    const Hz4* PHZ = phz + bt * M;
    const Pf3* PF = pf + bt * M;
    const float rnp = (np > 0) ? 1.0f / (float)np : 0.0f;
    const int N = (s.mode == MODE_INIT) ? K * K : I * np;
    double mloc = HYG_NINF;
    int cloc = 0;
    // The rows of the backward kernel need the weights of the few candidates
    // that can reach a trajectory's next state only (the list path); all N
    // weights are built for the final step's draw and for the general path.
    const bool fast = (s.mode != MODE_INIT) && np <= 64 && B <= 64 && Lcap >= 192 && t != T - 1;
    bool w_ready = false;
    auto make_W = [&]() {
      if (s.mode == MODE_INIT) gen_weights_init<NT>(cl, K, s.r_ph, Et, W, &mloc, &cloc);
      else gen_weights<NT>(cl, K, I, np, s.mode, s.log_c, s.lse, P, PW, PHZ, Et, W, &mloc, &cloc);
      w_ready = true;
    };
    if (!fast) make_W();
    BPH(0);
    // ---- hazard rows of record t-1's ancestors (arrived: read during step t+1)
    double2 h1c = make_double2(0.0, 0.0), h1k = make_double2(0.0, 0.0);
    Pf3 pf1;
    const bool have1 = (t > 0) && (ra < s1.n_par);
    if (have1) {
      h1c = hz_at(md, K, 0, hyg_st_rc(st1), hyg_st_dc(st1));
      h1k = hz_at(md, K, 1, hyg_st_rk(st1), hyg_st_dk(st1));
      pf1 = prefetch_rows(md, K, st1);
    }
    // ---- issue the read of record t-2. Its scalars come in as a vector load
    //      (lane i < 8: dword i) and are unpacked at the end of the step: a
    //      scalar load shares lgkmcnt with LDS, so the step's first LDS wait
    //      (or the spill of its SGPRs) waited out its trip to L2 on every wave.
    uint32_t sv2 = 0;
    uint64_t st2 = 0;
    double w2 = 0.0;
    if (t >= 2) {
      const uint8_t* rn = rec_ptr(t - 2);
      if (lane_id() < 8) sv2 = ((const uint32_t*)rn)[lane_id()];
      if (ra < M) {
        const uint64_t* rst = (const uint64_t*)(rn + sizeof(StepScalars));
        st2 = rst[ra];
        w2 = ((const double*)(rst + M))[ra];
      }
    }
    // ---- emission block t/EB - 2 into the half freed after this step's rows
    const bool eload = (t % kEBlock) == 0 && t >= 2 * kEBlock;
    constexpr int EQ = (kEBlock * 2 * HYG_KMAX + NT - 1) / NT;  // rows of one block per thread
    double ebuf[EQ];
    const int e_tot = eload ? kEBlock * K2 : 0;
    if (eload) {
      const int t0 = (t / kEBlock - 2) * kEBlock;
#pragma unroll
      for (int q = 0; q < EQ; ++q) {
        const int i = tid + q * NT;
        ebuf[q] = (i < e_tot) ? Ech[(size_t)t0 * K2 + i] : 0.0;
      }
    }
    if (!fast) w_barrier();  // W written by every thread (the list path reads only LDS written behind barriers)
    BPH(1);
    auto state_of = [&](int n) -> uint64_t {
      if (s.mode == MODE_INIT) return init_state(K, n);
      const int sl = fdiv(n, np, rnp);
      return tg_xi(K, P[n - sl * np], sl);
    };
    auto hz_of_n = [&](int n) -> Hz4 {
      if (s.mode == MODE_INIT) {
        const int i = n / K, j = n - (n / K) * K;
        Hz4 h;
        h.lrc = cl.hz1[0][i].x; h.l1c = cl.hz1[0][i].y; h.lrk = cl.hz1[1][j].x; h.l1k = cl.hz1[1][j].y;
        return h;
      }
      const int sl = fdiv(n, np, rnp), a = n - sl * np;
      return child_hz(cl, K, P[a], sl, PF[a], md);
    };
    const int rbs = ((B + 3) / 4) * 4;  // stride of the two draw-bit buffers
    const bool pre_bits = B <= 64 && NT >= 128;
    if (pre_bits && t == T - 1 && t >= 1 && wave_id() == NT / 64 - 1)
      backward_bits(rb + ((t - 1) & 1) * rbs, B, t - 1, ch.seed, ch.chain_id);
    auto rnd = [&](int b) -> uint64_t {
      return hyg_rand64(ch.seed, ch.chain_id, HYG_RNG_BACKWARD, (uint64_t)t, (uint64_t)b);
    };
    bool fail = false;
    if (t == T - 1) {
      // ---- B draws from the final weights (:383-385)
      const double lmax = block_max<NT>(mloc, red);
      if (!(lmax > HYG_NINF)) { if (tid == 0) sh.status = HYG_ENUMERIC; lds_barrier(); break; }
      auto logit = [&](int n) -> double { return W[n]; };
      auto out = [&](int q, int n) { idx[q] = n; };
      auto all = [](int) { return true; };
      lds_barrier();
      categorical_block<NT>(N, lmax, logit, B, all, rnd, out, cp128, red);
      lds_barrier();  // idx for the trajectory tail
    } else {
      // ---- backward-kernel rows (:400-435), one per distinct next state.
      // B <= 64: the groups (distinct next states, in order of first
      // occurrence) were formed by wave 0 at the end of step t+1.
      if (B > 64) {
        if (tid == 0) {
          int ng = 0;
          for (int b = 0; b < B; ++b) {
            int g = 0;
            while (g < ng && gst[g] != X[b]) ++g;
            if (g == ng) gst[ng++] = X[b];
            grp[b] = g;
          }
          sh.ng = ng;
        }
        lds_barrier();
      }
      const int ng = sh.ng;
      if (dbg && tid == 0) ph_acc[10] += ng;
      BPH(2);
      for (int g = 0; g < ng; ++g) {
        const uint64_t xn = gst[g];
        const int mn = hyg_st_m(xn), dcn = hyg_st_dc(xn), rcn = hyg_st_rc(xn), dkn = hyg_st_dk(xn),
                  rkn = hyg_st_rk(xn);
        bool one_wave = false;
        int L = 0, seg_incl = 0, nseg = 0;
        constexpr int kSeg = 16;
        bool segp = false;
        int* lst_n = (int*)cp128;  // list indices (cp area, NT+1 u128 = 4(NT+1) ints)
        double* lst_l = Lg;        // list logits (the W area: W is not built on the list path)
        if (fast) {
          // ---- finite logits l_n = log f(xn | x_n) + W_n, gathered into a short
          //      list (n, l_n): only a few dozen of the N candidates can reach xn.
          // Only slots whose child can have d_c = dcn - 1 (or a control change
          // point when dcn = 1) can reach xn: lc of tg_trans is a constant -inf
          // otherwise (ancestors always have d_c >= 1).
          int r0a, r0b, r1a, r1b;
          if (dcn >= 3) {  // A, C, D; the case side of trans_possible leaves fewer:
            r0a = 0; r0b = 1; r1a = K; r1b = 2 * K;
            if (mn == 1 && cl.u > 1) {
              r1a = 2 * K - 1;  // D: a C child (m = 0, d_k = 1 < u) cannot merge
            } else if (mn == 0 && dkn >= 2) {
              // unmerged xn continuing its case segment: x.m = 0 (no D), x.d_k =
              // d_k' - 1 and x.r_k = r_k' (a C child has d_k = 1, r_k = its slot's
              // regime; candidates have r_c = r_c' as lc requires)
              if (dkn == 2 && rkn != rcn) {
                r1a = K + (rkn < rcn ? rkn : rkn - 1);
                r1b = r1a + 1;
              } else {
                r1a = r1b = 2 * K;
              }
            }
          }
          else if (dcn == 2) { r0a = 1; r0b = K; r1a = 2 * K + rcn * K; r1b = r1a + K; }   // B, E(i = rcn)
          else { r0a = 0; r0b = I; r1a = I; r1b = I; }
          const int nseg0 = r0b - r0a;
          nseg = nseg0 + (r1b - r1a);
          // Segment list (at most kSeg reachable slots): slot v's finite logits
          // at [64 v, 64 v + c_v) in lane order, so the list is in n order by
          // construction: no shared counter, no atomics, no rank sort
          segp = nseg <= kSeg && Lcap >= 64 * kSeg + 160 && 4 * (NT + 1) >= 64 * kSeg;
          if (!segp) {
            if (tid == 0) sh.cnt = 0;
            lds_barrier();  // (the segment path: every reader of the areas is behind the last group's barrier)
          }
          const int cap = (4 * (NT + 1) < Lcap) ? 4 * (NT + 1) : Lcap;
          constexpr int NW = NT / 64;
          const int lane = lane_id(), wv = wave_id();
          const bool act = lane < np;
          const uint64_t par = act ? P[lane] : 0;
          const int am = hyg_st_m(par), adc = hyg_st_dc(par), arc = hyg_st_rc(par), adk = hyg_st_dk(par),
                    ark = hyg_st_rk(par);
          Pf3 pa{};
          Hz4 hanc{};
          double pwa = 0.0;
          if (act) {  // the ancestor's rows, once per group (not per slot)
            pa = PF[lane];
            hanc = PHZ[lane];
            pwa = PW[lane];
          }
          // the reachable slots, both ranges, round-robin over the waves (one
          // slot per wave from 8 waves on at d_c >= 3)
          {
            for (int sgv = wv; sgv < nseg; sgv += NW) {  // sgv: segment of slot sl
              const int sl = (sgv < nseg0) ? r0a + sgv : r1a + (sgv - nseg0);
              const Child x = child_of(cl, K, am, adc, arc, adk, ark, pa, sl);
              const bool poss = act && trans_possible(cl.u, x, mn, dcn, rcn, dkn, rkn);
              if (__ballot(poss) == 0) {  // nothing in this slot reaches xn
                if (segp && lane == 0) sh.segc[sgv] = 0;
                continue;
              }
              double l = HYG_NINF;
              if (poss) {
                // weight_at with the ancestor in registers and the child from
                // child_of (the same state as tg_xi): same operands, same order
                const uint64_t xs = hyg_st_pack(x.m, x.dc, x.rc, x.dk, x.rk);
                const double tr = tg_trans_sel(cl.lPm[am * 2 + x.m], cl.lPc[arc * K + x.rc], cl.lU1, cl.lU2, cl.u,
                                               am, adc, arc, adk, ark, xs, hanc);
                double w = HYG_NINF;
                if (hyg_isfinite(tr)) {
                  const double lg = tr + (Et[x.rc] + Et[K + x.rk]);
                  if (s.mode == MODE_KEEP) w = pwa + lg;
                  else if (s.mode == MODE_UNBIASED) w = (-cl.log_M + s.lse) + lg;
                  else {
                    const double vv = (double)s.log_c + (pwa - s.lse);
                    w = (pwa + lg) - (vv < 0.0 ? vv : 0.0);
                  }
                }
                if (w > HYG_NINF) {
                  const double f = tg_trans_sel(cl.lPm[x.m * 2 + mn], cl.lPc[x.rc * K + rcn], cl.lU1, cl.lU2,
                                                cl.u, x.m, x.dc, x.rc, x.dk, x.rk, xn, x.h);
                  if (hyg_isfinite(f)) l = f + w;
                }
              }
              const unsigned long long mask = __ballot(l > HYG_NINF);
              if (segp) {
                if (lane == 0) sh.segc[sgv] = (int)__popcll(mask);
                if (l > HYG_NINF) {
                  const int pos = 64 * sgv + lanes_below(mask);
                  lst_n[pos] = sl * np + lane;
                  lst_l[pos] = l;
                }
              } else if (mask) {
                int base = 0;
                if (lane == 0) base = atomicAdd(&sh.cnt, __popcll(mask));
                base = __builtin_amdgcn_readfirstlane(base);
                if (l > HYG_NINF) {
                  const int pos = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                  if (pos < cap) { lst_n[pos] = sl * np + lane; lst_l[pos] = l; }
                }
              }
            }
          }
          lds_barrier();
          BPH(3);
          // segment path: inclusive prefix of the segment counts in every wave
          seg_incl = segp ? wave_incl_int(lane_id() < nseg ? sh.segc[lane_id()] : 0) : 0;
          L = segp ? __builtin_amdgcn_readlane(seg_incl, 63) : sh.cnt;
          if (dbg && tid == 0) ph_acc[11] += L;
          if (L == 0) { fail = true; break; }  // uniform: every logit -inf
          one_wave = L <= 64 && Lcap >= 192;
        }
        if (pre_bits && g == 0 && t >= 1 && wave_id() == NT / 64 - 1)  // next step's bits, while wave 0 draws
          backward_bits(rb + ((t - 1) & 1) * rbs, B, t - 1, ch.seed, ch.chain_id);
        if (one_wave) {
          // ---- one wave: order the list by n, exact masses, scan, draws
          if (wave_id() == 0) {
            serial_begin();
            const int lane = lane_id();
            const bool v = lane < L;
            double sv;
            hyg_u128* cdfa;
            int* cn;
            if (segp) {
              // list position `lane` lies in the segment whose inclusive end
              // is the first one above it (lanes q >= nseg hold the total L:
              // every valid lane is below it, so all kSeg ends are read, each
              // from a constant lane)
              int seg = 0, base = 0;
#pragma unroll
              for (int q = 0; q < kSeg; ++q) {
                const int iv = __builtin_amdgcn_readlane(seg_incl, q);
                seg += (iv <= lane) ? 1 : 0;
                base = (iv <= lane) ? iv : base;
              }
              const int at = 64 * seg + (lane - base);
              const int myn = v ? lst_n[at] : 0;
              sv = v ? lst_l[at] : HYG_NINF;
              cdfa = (hyg_u128*)(Lg + 64 * kSeg);       // behind the segments
              cn = (int*)(Lg + 64 * kSeg + 128);        // the list's indices in n order
              if (v) cn[lane] = myn;
            } else {
              const int myn = v ? lst_n[lane] : 0x7fffffff;
              const double myl = v ? lst_l[lane] : HYG_NINF;
              int rank = 0;
#pragma unroll 4
              for (int j = 0; j < L; ++j) rank += (lst_n[j] < myn) ? 1 : 0;  // broadcast reads
              __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront", "local");
              if (v) { lst_n[rank] = myn; lst_l[rank] = myl; }
              __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront", "local");
              sv = v ? lst_l[lane] : HYG_NINF;
              cdfa = (hyg_u128*)(Lg + 64);  // behind the 64 list logits
              cn = lst_n;
            }
            BPH(12);
            const double lmax = wave_max(sv);
            BPH(13);
            hyg_u128 ms = hyg_u128_zero();
            if (v) ms = hyg_exp_fix100(sv - lmax);
            BPH(14);
            const hyg_u128 cdf = wave_incl128(ms);
            BPH(15);
            hyg_u128 total;
            total.lo = rdlane64(cdf.lo, L - 1);
            total.hi = rdlane64(cdf.hi, L - 1);
            if (v) cdfa[lane] = cdf;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront", "local");
            BPH(16);
            // lane b draws for trajectory b: first list entry with cdf > target
            if (lane < B && grp[lane] == g) {
              const uint64_t bits = pre_bits ? rb[(t & 1) * rbs + lane] : rnd(lane);  // = hyg_rand64(.., t, lane)
              const hyg_u128 tb = hyg_scale_target(bits, total);
              int lo = 0, hi = L - 1;
              while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (hyg_u128_lt(tb, cdfa[mid])) hi = mid; else lo = mid + 1;
              }
              idx[lane] = cn[lo];
            }
            serial_end();
          } else if (kOutWave > 0 && g == 0 && pend >= 0 && wave_id() == kOutWave) {
            write_outputs(pend);
          }
          if (kOutWave > 0 && g == 0) pend = -1;
          BPH(4);
          if (g + 1 < ng) lds_barrier();  // the next group's list reuses the areas wave 0 read
        } else {
          // ---- general case: logits of all N in index order (built in place of
          //      the weights), block categorical
          if (kOutWave > 0 && g == 0 && pend >= 0) {
            if (wave_id() == kOutWave) write_outputs(pend);
            pend = -1;
          }
          if (!w_ready) {
            w_barrier();  // the list areas (= the W area) are reused below
            make_W();
            w_barrier();
          }
          double m = HYG_NINF;
          for (int n = tid; n < N; n += NT) {
            const double w = W[n];
            double l = HYG_NINF;
            if (w > HYG_NINF) {
              const double f = tg_trans(cl, K, state_of(n), xn, hz_of_n(n));
              if (hyg_isfinite(f)) l = f + w;
            }
            W[n] = l;  // each n read and rewritten by one thread
            m = dmax(m, l);
          }
          if constexpr (GW) __syncthreads();  // the categorical reads other threads' logits
          w_ready = false;  // W holds this group's logits now
          const double lmax = block_max<NT>(m, red);
          if (!(lmax > HYG_NINF)) { fail = true; break; }  // uniform: every logit -inf
          auto logit = [&](int n) -> double { return W[n]; };
          auto in_g = [&](int b) { return grp[b] == g; };
          auto out = [&](int b, int n) { idx[b] = n; };
          categorical_block<NT>(N, lmax, logit, B, in_g, rnd, out, cp128, red);
          lds_barrier();
        }
        BPH(5);
      }
      if (fail) { if (tid == 0) sh.status = HYG_ENUMERIC; lds_barrier(); break; }
    }
    // ---- trajectories and test-function means at t (run_inference_two_groups.py:233-240, 294-314)
    if (B <= 64) {
      // wave 0 alone: trajectory b on lane b (idx written by this wave's draws,
      // or behind a barrier), then the groups of step t-1's next states
      if (wave_id() == 0) {
        serial_begin();
        wave_lds_sync();
        const int lane = lane_id();
        const bool v = lane < B;
        uint64_t x = 0;
        if (v) {
          x = state_of(idx[lane]);
          xo[(t & 1) * B + lane] = x;
        }
        if constexpr (kOutWave == 0) {
          wave_lds_sync();
          write_outputs(t);
        }
        BPH(6);
        if (t > 0) {
          // distinct states in order of first occurrence, by ballots: one
          // iteration per group (about one per step)
          uint64_t rem = __ballot(v);
          int gi = 0, mg = 0;
          while (rem) {  // uniform
            const int ld = (int)__builtin_ctzll(rem);
            const uint64_t xv = rdlane64(x, ld);
            const uint64_t eq = __ballot(v && x == xv);
            if (lane == 0) gst[gi] = xv;
            mg = ((eq >> lane) & 1) ? gi : mg;
            rem &= ~eq;
            ++gi;
          }
          if (v) grp[lane] = mg;
          if (lane == 0) sh.ng = gi;
        }
        serial_end();
      }
    } else {
      for (int b = tid; b < B; b += NT) {
        const uint64_t x = state_of(idx[b]);
        X[b] = x;
        const size_t o = (size_t)(ch.out_begin + t) * B + b;
        o_merged[o] = (int16_t)hyg_st_m(x);
        o_control[2 * o + 0] = (int16_t)hyg_st_dc(x);
        o_control[2 * o + 1] = (int16_t)hyg_st_rc(x);
        o_case[2 * o + 0] = (int16_t)hyg_st_dk(x);
        o_case[2 * o + 1] = (int16_t)hyg_st_rk(x);
      }
      lds_barrier();
      if (tid < 2 * K + 1) {
        int cntv = 0;
        for (int b = 0; b < B; ++b) {
          const uint64_t x = X[b];
          if (tid == 0) cntv += (hyg_st_m(x) == 0);
          else if (tid <= K) cntv += (hyg_st_rc(x) == tid - 1);
          else cntv += (hyg_st_rk(x) == tid - 1 - K);
        }
        const float v = (float)cntv / (float)B;
        if (tid == 0) o_split[ch.out_begin + t] = v;
        else o_regime[(size_t)(ch.out_begin + t) * K2 + (tid - 1)] = v;
      }
    }
    // ---- record t-1 (+ hazard rows) into the other buffer: its last readers
    //      (step t+1) are behind this step's barriers; the emission block into
    //      the ring half whose rows this step no longer reads
    if (have1) {
      const int o = (bt ^ 1) * M + ra;
      pst[o] = st1;
      pw[o] = w1;
      Hz4 h;
      h.lrc = h1c.x; h.l1c = h1c.y; h.lrk = h1k.x; h.l1k = h1k.y;
      phz[o] = h;
      pf[o] = pf1;
    }
    if (eload) {
      double* dst = ering + (size_t)((t / kEBlock - 2) & 1) * kEBlock * K2;
#pragma unroll
      for (int q = 0; q < EQ; ++q) {
        const int i = tid + q * NT;
        if (i < e_tot) dst[i] = ebuf[q];
      }
    }
    lds_barrier();
    if (kOutWave > 0 && B <= 64) pend = t;
    s = s1;
    st1 = st2;
    w1 = w2;
    {
      // (StepScalars: mode, n_par, log_c, r_ph, lse; zero before record 0)
      s1.mode = __builtin_amdgcn_readlane((int)sv2, 0);
      s1.n_par = __builtin_amdgcn_readlane((int)sv2, 1);
      s1.log_c = __builtin_bit_cast(float, __builtin_amdgcn_readlane((int)sv2, 2));
      s1.r_ph = __builtin_amdgcn_readlane((int)sv2, 3);
      s1.lse = d_of(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)sv2, 5) << 32) |
                    (uint32_t)__builtin_amdgcn_readlane((int)sv2, 4));
      s1.pad = 0.0;
    }
  }
  lds_barrier();
  if (kOutWave > 0 && B <= 64 && pend >= 0 && wave_id() == kOutWave) write_outputs(pend);
  if (tid == 0 && status_out) status_out[blockIdx.x] = sh.status;
  if (dbg && tid == 0) {
    for (int k = 0; k < kPh - 1; ++k) dbg[(size_t)blockIdx.x * kPh + k] = ph_acc[k];
    dbg[(size_t)blockIdx.x * kPh + kPh - 1] = (unsigned long long)T;
  }
#undef BPH
}

}  // namespace hyg
