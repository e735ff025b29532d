// Internal types shared by the host library (capi.cpp) and the kernels
// (tg_kernels.hip). Not part of the public ABI.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/hyg_model.h"

namespace hyg {

constexpr int kDefaultThreads = 256;     // forward workgroup size
constexpr int kDefaultThreadsBwd = 256;  // backward workgroup size (HYG_THREADS[_FWD/_BWD] override)
// forward / backward workgroup size when a launch has at most one chain per CU
// (tg_kernels.hip pick_threads; HYG_LOWOCC_THREADS overrides both): the
// backward's list phase keeps 12 waves busy (768: 546 vs 558 ms at 145 chains,
// r03x), the forward is faster at 512 (1327 vs 1377 ms)
constexpr int kLowOccThreads = 512;
constexpr int kLowOccThreadsBwd = 768;
constexpr int kEBlock = 8;     // emission rows staged in LDS per block of steps

// Device-side chain descriptor (lives in the workspace header).
struct ChainDev {
  int64_t site_begin;
  int64_t out_begin;
  int64_t ws_offset;  // byte offset of the chain's history records
  uint64_t seed;
  uint64_t chain_id;
  int32_t T;
  int32_t pad;  // index of the chain's model in the table of a multi-model launch (launch_chains_multi), else 0
  // byte offset of the chain's global particle scratch (chain_scratch_bytes):
  // the backward's full-N weights (Nmax f64; backward_global_w), and for a
  // shape whose particle arrays exceed LDS (forward_global_w) the forward's
  // weights and sort keys, whose weight part the backward reuses
  int64_t wg_offset;
};

// Per-step history record: scalars, then M packed parent states, then M
// parent weights. Written by the forward kernel, read by the backward kernel.
struct StepScalars {
  int32_t mode;   // 0 keep, 1 optimal, 2 unbiased, 3 init
  int32_t n_par;
  float log_c;
  int32_t r_ph;
  double lse;
  double pad;
};
static_assert(sizeof(StepScalars) == 32, "record scalars");
// (the backward kernel reads them as dwords: mode 0, n_par 1, log_c 2, r_ph 3, lse 4-5)
static_assert(offsetof(StepScalars, n_par) == 4 && offsetof(StepScalars, log_c) == 8 &&
                  offsetof(StepScalars, r_ph) == 12 && offsetof(StepScalars, lse) == 16,
              "record scalar dwords");

#if defined(__HIPCC__)
__host__ __device__
#endif
inline size_t record_bytes(int M) { return sizeof(StepScalars) + (size_t)M * 16; }

struct ModelDev {
  const hyg_tg_consts* consts;  // device copy
  const double* hz;             // [2][K][dcap][2]
  int32_t dcap;
  int32_t nmax_reads;
  const double* lf;   // [nmax+1]
  const double* lg;   // [K][3][nmax+1]
  const double* cst;  // [K]
  const double* bbt;  // per-(n, y) terms [(nmax+1)(nmax+2)/2][K] (hyg_bb_term_table), or null when too large
};

// Launchers (tg_kernels.hip)
int launch_emission(const ModelDev& md, const hyg_tg_consts& c, const uint16_t* meth_c, const uint16_t* tot_c,
                    int s_c, const uint16_t* meth_k, const uint16_t* tot_k, int s_k, int64_t n_sites,
                    double* E, void* stream);
// chains_host: the same descriptors on the host (their lengths decide whether
// the forward runs in rounds, tg_kernels.hip forward_schedule); null: one launch.
int launch_chains(const ModelDev& md, const hyg_tg_consts& c, const ChainDev* chains_dev, int n_chains,
                  const double* E, uint8_t* ws, const hyg_tg_outputs& out, void* stream,
                  const ChainDev* chains_host = nullptr);
// A launch whose chains each name their model: models_dev is a device table of
// the launch's models (same shape c, one emission table), ChainDev::pad of a
// chain its index into the table. Planned as launch_chains of n_chains chains.
int launch_chains_multi(const ModelDev* models_dev, const hyg_tg_consts& c, const ChainDev* chains_dev, int n_chains,
                        const double* E, uint8_t* ws, const hyg_tg_outputs& out, void* stream,
                        const ChainDev* chains_host = nullptr);
// A forward-only launch: the forward of every chain in a build that records no
// history (tg_forward_kernel's REC = false), planned as the forward of
// launch_chains of n_chains chains. Writes out.log_z, out.status and, where
// given, out.final_log_weights; ws holds the header and, for a forward_global_w
// shape, the chains' scratch. The timing events stand around the forward.
int launch_filter(const ModelDev& md, const hyg_tg_consts& c, const ChainDev* chains_dev, int n_chains,
                  const double* E, uint8_t* ws, const hyg_tg_outputs& out, void* stream);
int launch_filter_multi(const ModelDev* models_dev, const hyg_tg_consts& c, const ChainDev* chains_dev, int n_chains,
                        const double* E, uint8_t* ws, const hyg_tg_outputs& out, void* stream);
// A traced forward-only launch: launch_filter[_multi] in the TRC build of the
// forward kernel, which also writes row ChainDev::out_begin + t of the trace
// arrays (device pointers, at least one non-null) for every site t of a chain.
int launch_trace(const ModelDev& md, const hyg_tg_consts& c, const ChainDev* chains_dev, int n_chains, const double* E,
                 uint8_t* ws, const hyg_tg_outputs& out, const hyg_tg_trace& trace, void* stream);
int launch_trace_multi(const ModelDev* models_dev, const hyg_tg_consts& c, const ChainDev* chains_dev, int n_chains,
                       const double* E, uint8_t* ws, const hyg_tg_outputs& out, const hyg_tg_trace& trace,
                       void* stream);
void set_kernel_timing(bool on);
int last_kernel_ms(float* out3);
// Diagnostics of a launch of n_chains chains, read from its kernel plan
// (tg_kernels.hip: plan, the one place that decides which kernel runs).
int tg_threads_per_chain(const hyg_tg_consts& c, int n_chains);  // forward workgroup size of a launch
int tg_threads_per_chain_bwd(const hyg_tg_consts& c, int n_chains);  // backward workgroup size of a launch
// the instantiation a launch runs, as tools/resource_notes.py spells it; returns the plan's status
// (multi: of a multi-model launch, whose names carry a seventh argument, true)
int tg_kernel_name(const hyg_tg_consts& c, int n_chains, bool backward, const char** name, bool multi = false);
// the same of a forward-only launch: all eight template arguments, the last one false
int tg_filter_kernel_name(const hyg_tg_consts& c, int n_chains, const char** name, bool multi = false);
// the same of a traced launch: nine arguments, "...,false,true>"
int tg_trace_kernel_name(const hyg_tg_consts& c, int n_chains, const char** name, bool multi = false);
size_t tg_trace_lds_bytes(const hyg_tg_consts& c, int n_chains);  // LDS of one chain of a traced launch
int tg_force_threads(int fwd, int bwd);                           // test override (0 = automatic)
int tg_resident_per_cu(const hyg_tg_consts& c, int n_chains);     // forward workgroups per CU
void tg_set_tail_overlap(bool on);                                // hyg_tg_set_tail_overlap
int tg_set_gather_window(int positions);                          // hyg_tg_set_gather_window
void tg_set_priority_rotation(bool on);                           // hyg_tg_set_priority_rotation
void tg_set_fine_list_walk(bool on);                              // hyg_tg_set_fine_list_walk
int tg_fine_list_walk();                                          // hyg_tg_fine_list_walk
int tg_priority_base(unsigned long long ticks, int slot);         // hyg_tg_priority_base
int tg_set_forward_rounds(int mode);                              // hyg_tg_set_forward_rounds
// hyg_tg_forward_schedule (tg_kernels.hip): rounds, grids, block orders and step ranges of a launch
int tg_forward_schedule(const hyg_tg_consts& c, const int* T, int n, bool multi, bool forward_only, int cus, int resident,
                        int max_rounds, int* blocks, int* order, int* begin, int* end);
int tg_priority_epoch_ticks();                                    // clock ticks (10 ns) of one order of priorities
int tg_device_cus(int dev);                                       // CUs of a device as the launcher sees them
int tg_set_device_cus(int dev, int cus);                          // test override (0 = query the device)
size_t tg_layout_bytes(const hyg_tg_consts& c, int threads, bool backward);  // LDS of one chain (0: bad width)
// Whether a model's backward keeps its full-N weights (the general path and the
// final step's draw) in a per-chain global scratch of Nmax f64 instead of LDS,
// so that its LDS holds several chains per CU (the C5 shape); the workspace
// then carries n_chains * chain_scratch_bytes(c) more bytes.
bool backward_global_w(const hyg_tg_consts& c);
// Whether a model's particle arrays (the forward's full-N weights and sort
// keys) exceed the 160 KiB LDS of a CU at the default width. Such a shape runs
// both kernels at 256 threads, whatever width is forced, with those arrays in
// the chain's global scratch; it implies backward_global_w.
bool forward_global_w(const hyg_tg_consts& c);
// Global scratch of one chain (a multiple of 256 bytes; 0 for a shape that
// keeps everything in LDS): Nmax f64 for the backward alone, the forward's
// weights and keys for a forward_global_w shape.
size_t chain_scratch_bytes(const hyg_tg_consts& c);

}  // namespace hyg
