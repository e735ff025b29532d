// Internal types of the single-group path shared by capi.cpp and
// sg_kernels.hip (not part of the public ABI).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/hyg_sg_model.h"
#include "../../include/hyg_sg_pe.h"

namespace hyg {

constexpr int kSgThreads = 256;         // one particle per thread: N_max <= 256
constexpr int kSgPsiCapDefault = 4096;  // pending smoothing times per chain
constexpr int kSgRngSystematic = 5;     // Philox stream of the systematic uniform

struct SgModelDev {
  const hyg_sg_consts* consts;  // device copy
  const double* hz;             // [K][dcap][2]: log rho, log(1 - rho) | -inf
  const uint8_t* ex;            // [K][dcap] exit status
  int32_t dcap;
  int32_t nmax_reads;
  const double* lf;             // BB tables as hyg_sg_bb_tables
  const double* lg;
  const double* cst;
  uint64_t key_keep;            // the packed log-weight sort's key bits (~0xff; hyg_sg_force_key_drop)
};

struct SgChainDev {
  int64_t site_begin;
  int64_t out_begin;
  int64_t psi_offset;  // byte offset of the chain's smoothing slots in the workspace
  int64_t ring_offset; // byte offset of the chain's step-record ring (SMC workgroup -> smoothing workgroup)
  int64_t ctl_offset;  // byte offset of the chain's ring control words (zeroed before each launch)
  uint64_t seed;
  uint64_t chain_id;
  int32_t T;
  int32_t rcap;        // parameter estimation: hazard rows per regime
  int64_t pe_offset;   // parameter estimation: byte offset of the chain's region
  int64_t theta_row;   // parameter estimation: first output row of theta
};

// Online parameter estimation (include/hyg_sg_pe.h), model-level inputs
struct SgPeDev {
  hyg_sgpe_consts c;
  const double* theta0;        // [dim] initial theta
  const hyg_sgpe_step* steps;  // [n] step sizes / bias corrections per update
  const double* lgk;           // [K][lgk_stride] theta-free part of the NegBin log-pmf
  const double* dgk;           // [K][lgk_stride] psi(x + kappa) - psi(kappa) (kappa estimated), else null
  int32_t lgk_stride;
  int32_t pad;
  double* theta_out;           // [rows][c.dim]
};

// Per-chain region of the estimation path: phi [2][256][K^2] (the kappa
// coordinates' score is identically 0, include/hyg_sg_pe.h), theta, ADAM
// moments, previous / current score [K (K + 1)] each, hazard rows [K][rcap],
// and the rebuild scratch h, g, gk, bigH[d-1], gradBigH[d-1] [K][rcap] f64 +
// exit [K][rcap] u8.
__host__ __device__ inline size_t sg_pe_region_bytes(int K, int rcap) {
  const size_t dim = (size_t)K * K, dth = (size_t)K * (K + 1);
  const size_t b = 8 * (2 * (size_t)kSgThreads * dim + 5 * dth) + 32 * (size_t)K * rcap + 40 * (size_t)K * rcap +
                   (size_t)K * rcap;
  return (b + 255) / 256 * 256;
}

// The SMC of a chain runs in one workgroup and its online marginal smoothing
// in a second one (sg_kernels.hip): per step the SMC workgroup publishes a
// record {N, N_prev, M, t | ancestor + regime [256] u64 | weights [256] f64 |
// backward kernels [K][256] f64} into a ring of kSgRing slots in the
// workspace, the smoothing workgroup consumes it.
constexpr int kSgRing = 32;
__host__ __device__ inline size_t sg_rec_bytes(int K) {
  return (16 + 8 * 2 * (size_t)kSgThreads + 8 * (size_t)K * kSgThreads + 255) / 256 * 256;
}
constexpr size_t kSgCtlBytes = 16;  // per chain: head (records published), tail (consumed), abort code, and
                                    // (first chain of a launch) the launch's dispatch-ticket counter

// Per-chain workspace: cap psi slots [K][256] f64, then the pending-time lists
// slot[2][cap] / time[2][cap] (double-buffered), keep[cap], free[cap] (int32),
// then the step-record ring.
__host__ __device__ inline size_t sg_psi_region_bytes(int K, int cap) {
  return ((sizeof(double) * (size_t)K * kSgThreads * (size_t)cap) + 255) / 256 * 256;
}
__host__ __device__ inline size_t sg_lists_bytes(int cap) {
  return ((sizeof(int32_t) * 6 * (size_t)cap) + 255) / 256 * 256;
}
__host__ __device__ inline size_t sg_chain_ws_bytes(int K, int cap) {
  return sg_psi_region_bytes(K, cap) + sg_lists_bytes(cap) + (size_t)kSgRing * sg_rec_bytes(K);
}

// A multi-model launch (hyg_sg_run_chains_multi): chain i of the launch runs
// under models[chain_model[i]]. All three are device arrays in the workspace
// header; the descriptors stay SgChainDev, so the single-model builds see the
// same ones. With estimation pe_models[m] replaces SgPeDev's theta0 / lgk / dgk
// (models of one kappa vector, bit for bit, point at one lgk / dgk table).
struct SgPeModelDev {
  const double* theta0;  // [dim]
  const double* lgk;     // [K][lgk_stride]
  const double* dgk;     // [K][lgk_stride] (kappa estimated), else null
};
struct SgMultiDev {
  const SgModelDev* models;        // [n_models], key_keep filled in (sg_key_keep)
  const int32_t* chain_model;      // [n_chains]
  const SgPeModelDev* pe_models;   // [n_models] with estimation, else null
};

// The outputs of a forward-only launch (sg_chain_kernel's FO builds), device
// pointers indexed by the chain of the launch; only log_z is required. The
// three trace arrays (TRC builds; at least one non-null) are indexed by output
// row, SgChainDev::out_begin + t. trs: LDS offset of the trace's class sums.
struct SgFoDev {
  double* log_z;          // [n_chains]
  double* final_lw;       // [n_chains][Nmax], -inf beyond N
  int32_t* final_st;      // [n_chains][Nmax][2] (d, r), -1 beyond N
  int32_t* n_part;        // [n_chains]
  double* log_z_t;        // [rows]
  double* regime_probs;   // [rows][K]
  double* cp_probs;       // [rows]
  uint32_t trs;
  uint32_t pad;
};

// The history of a forward-only launch (sg_chain_kernel's HST builds): the
// particle set of every site, indexed by output row, SgChainDev::out_begin + t.
// 12 Nmax + 4 bytes per site. Entries n >= n_part[row] are not written; after
// HYG_ENUMERIC the rows from the failing site on have n_part = 0.
struct SgHistDev {
  double* lw;        // [rows][Nmax] unnormalised log-weights of step t
  uint32_t* st;      // [rows][Nmax] d | r << 24
  int32_t* n_part;   // [rows] N_t
};
struct SgFoHistDev {
  SgFoDev fo;
  SgHistDev hist;
};

// The history builds' translation unit (sg_kernels_fohst.hip): multi-model,
// untraced; every other output is the untraced forward-only launch's.
int sg_launch_history_multi(const SgMultiDev& mm, const hyg_sg_consts& c, const SgChainDev* chains_dev, int n_chains,
                            const double* E, uint8_t* ws, const SgFoDev& out, const SgHistDev& hist, int32_t* status,
                            void* stream);

// Backward simulation from a history (sg_sample_kernels.hip): one wave per
// (chain, trajectory), B trajectories per chain, paths int16 [rows][B][2] =
// (d mod 2^16, r) at row out_begin + t. fwd_status / sample_status may be null.
constexpr int kSgRngSample = 6;  // Philox stream of the backward draws
int sg_launch_sample(const SgMultiDev& mm, const hyg_sg_consts& c, const SgChainDev* chains_dev, int n_chains,
                     const SgHistDev& hist, const int32_t* fwd_status, int B, int16_t* paths, int32_t* sample_status,
                     void* stream);

// A forward-only launch (sg_kernels_fo.hip, sg_kernels_fomm.hip): one workgroup
// per chain, nothing but the descriptors in the workspace; trace: the TRC
// builds. mm non-null: the multi-model builds (md is then unused).
int sg_launch_filter(const SgModelDev& md, const hyg_sg_consts& c, const SgChainDev* chains_dev, int n_chains,
                     const double* E, uint8_t* ws, const SgFoDev& out, bool trace, int32_t* status, void* stream,
                     const SgMultiDev* mm = nullptr);
int sg_launch_filter_multi(const SgMultiDev& mm, const hyg_sg_consts& c, const SgChainDev* chains_dev, int n_chains,
                           const double* E, uint8_t* ws, const SgFoDev& out, bool trace, int32_t* status,
                           void* stream);
// the instantiation such a launch runs (no device needed); HYG_EUNSUPPORTED for a shape it cannot run
int sg_filter_kernel_name(const hyg_sg_consts& c, bool multi, bool trace, const char** name);
size_t sg_filter_lds_bytes(const hyg_sg_consts& c, bool trace);

int sg_launch_emission(const SgModelDev& md, const hyg_sg_consts& c, const uint16_t* meth, const uint16_t* tot,
                       int S, int64_t n_sites, double* E, void* stream);
// ctl: the chains' ring control words (kSgCtlBytes each, contiguous), zeroed here before the launches
int sg_force_key_drop(int bits);  // test override of the packed sort's dropped key bits (0 = 8)
uint64_t sg_key_keep();           // SgModelDev::key_keep of the next launch
// mm: the multi-model form (md is then unused; c is the shape the models share).
// The LDS layout and the batching are planned from the shape as without it.
int sg_launch_chains(const SgModelDev& md, const hyg_sg_consts& c, const SgChainDev* chains_dev, int n_chains,
                     const double* E, uint8_t* ws, int psi_cap, double* probs, int32_t* status, void* ctl,
                     void* stream, const SgPeDev* pe = nullptr, const SgMultiDev* mm = nullptr);
// the multi-model builds' translation unit (sg_kernels_mm.hip); called by sg_launch_chains
int sg_launch_chains_multi(const SgMultiDev& mm, const hyg_sg_consts& c, const SgChainDev* chains_dev, int n_chains,
                           const double* E, uint8_t* ws, int psi_cap, double* probs, int32_t* status, void* stream,
                           const SgPeDev* pe);
size_t sg_lds_bytes(const hyg_sg_consts& c, int psi_cap, bool pe = false);

}  // namespace hyg
