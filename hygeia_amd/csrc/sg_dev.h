// sg_dev.h -- device helpers shared by the single-group kernels
// (sg_kernels.hip, sg_sample_kernels.hip): the packed particle state, the
// transition parts of a particle and the exact ceil(T * R).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/hyg_arith.h"
#include "sg_common.h"

namespace hyg {

__device__ __forceinline__ uint32_t sg_pack(int d, int r) { return (uint32_t)d | ((uint32_t)r << 24); }
__device__ __forceinline__ int sg_d(uint32_t s) { return (int)(s & 0xffffffu); }
__device__ __forceinline__ int sg_r(uint32_t s) { return (int)(s >> 24); }

// Model::evaluateLogTransitionDensity (singleGroup.h:569-608) split per
// previous particle (d, r): the density of a fresh particle (1, q) is
// base + log P[r][q] with base = log rho(d, r) (0 after the hazard's exit, -inf
// for d < u), and of the continuing particle (d + 1, r) it is cont =
// log(1 - rho(d, r)). Both equal the oracle's sg_trans bit for bit (the
// diagonal log P[r][r] = -inf covers q == r).
// the hazard row and exit flag of state s (sg_trans_parts in two halves: the
// loads, and the parts formed from them where they are used)
__device__ __forceinline__ void sg_trans_load(const SgModelDev& md, uint32_t s, double2& h, uint8_t& ex) {
  const int d = sg_d(s), r = sg_r(s);
  int di = d - 1;
  if (di >= md.dcap) di = md.dcap - 1;
  h = *(const double2*)(md.hz + ((size_t)r * md.dcap + di) * 2);
  ex = md.ex[(size_t)r * md.dcap + di];
}
__device__ __forceinline__ void sg_trans_form(int u, uint32_t s, const double2& h, uint8_t ex, double& base,
                                              double& cont) {
  base = (sg_d(s) >= u) ? (ex ? 0.0 : h.x) : HYG_NINF;
  cont = h.y;
}
__device__ __forceinline__ void sg_trans_parts(const SgModelDev& md, int u, uint32_t s, double& base,
                                               double& cont) {
  double2 h;
  uint8_t ex;
  sg_trans_load(md, s, h, ex);
  sg_trans_form(u, s, h, ex, base, cont);
}

// ceil(T * R) for a double T in [0, 1] and R < 2^127 (oracle/sg_oracle.c:ceil_mul_f64)
__device__ __forceinline__ hyg_u128 sg_ceil_mul_f64(double T, hyg_u128 R) {
  hyg_u128 z = hyg_u128_zero();
  if (!(T > 0.0)) return z;
  const uint64_t b = hyg_f64_bits(T);
  const int E = (int)((b >> 52) & 0x7ff);
  const uint64_t m = (E == 0) ? (b & 0x000fffffffffffffull) : ((b & 0x000fffffffffffffull) | 0x0010000000000000ull);
  const int s = (E == 0) ? 1074 : 1075 - E;
  const uint64_t l0 = m * R.lo, h0 = hyg_mulhi64(m, R.lo);
  const uint64_t l1 = m * R.hi, h1 = hyg_mulhi64(m, R.hi);
  uint64_t w0 = l0, w1 = h0 + l1, w2 = h1 + (w1 < h0 ? 1u : 0u);
  if (s >= 192) { hyg_u128 o; o.lo = (w0 | w1 | w2) ? 1u : 0u; o.hi = 0; return o; }
  uint64_t b0 = 0, b1 = 0, b2 = 0;
  if (s < 64) b0 = (1ull << s) - 1;
  else if (s < 128) { b0 = ~0ull; b1 = (s == 64) ? 0 : (1ull << (s - 64)) - 1; }
  else { b0 = ~0ull; b1 = ~0ull; b2 = (s == 128) ? 0 : (1ull << (s - 128)) - 1; }
  const uint64_t q0 = w0 + b0, c0 = q0 < w0;
  const uint64_t t1 = w1 + b1, c1a = t1 < w1;
  const uint64_t q1 = t1 + c0, c1b = q1 < t1;
  const uint64_t q2 = w2 + b2 + c1a + c1b;
  hyg_u128 r;
  if (s < 64) { r.lo = (q0 >> s) | (s ? q1 << (64 - s) : 0); r.hi = (q1 >> s) | (s ? q2 << (64 - s) : 0); }
  else if (s == 64) { r.lo = q1; r.hi = q2; }
  else if (s < 128) { r.lo = (q1 >> (s - 64)) | (q2 << (128 - s)); r.hi = q2 >> (s - 64); }
  else if (s == 128) { r.lo = q2; r.hi = 0; }
  else { r.lo = q2 >> (s - 128); r.hi = 0; }
  return r;
}

}  // namespace hyg
