// tg_rows.h -- the row tables of the two-group chain kernels: what a
// translation unit says about each instantiation it holds (KernelRow), how a
// row is written (TG_ROW) and how its kernel is launched (ChainLaunch, the
// row's thunk). tg_kernels.hip holds the rows of the full builds.
#pragma once

#include "tg_forward.h"

namespace hyg {

// The model argument of a launch: one model, or (table != nullptr) the device
// table of a multi-model launch, whose plans hold multi-model rows.
struct ModelRef {
  ModelDev md;
  const ModelDev* table;
};
// One launch of a chain kernel, forward or backward, as a row's thunk takes it.
struct ChainLaunch {
  unsigned grid;  // workgroups: one per chain (the threads are the row's nt)
  size_t lds;     // dynamic LDS
  hipStream_t stream;
  ModelRef m;
  const ChainDev* chains;
  const double* E;
  uint8_t* ws;  // (the kernels' ws and wscr)
  hyg_tg_outputs out;
  Lay lay;
  unsigned long long* dbg;      // phase-timer builds: the counters (phase_buffer); else null
  const TraceArg<true>* trace;  // traced builds: the trace arrays; else null
  const ResArg<true>* res;      // resuming builds: the grid's entries; else null
};

// The instantiations. A compile-time shape has its own builds: the pipeline's
// (C3 / C4: K = 6, M = 50, B = 25) at 256, 512 and 768 threads, the stress
// shape's (C5: K = 12, M = 50, B = 25) at 512 and 768 and, for the GW backward,
// at 256. HYG_NO_SHAPE=1 (tuning build) takes the generic ones.
enum Shape { kGeneric = 0, kC3 = 6, kC5 = 12 };  // (the value is the build's KC)
struct KernelRow {
  int nt;
  Shape shape;
  bool phases, gw;         // phase-timer build; GW build
  bool mm, rec, trc, res;  // multi-model, recording, traced, resuming build
  const void* fn;          // the kernel (hipFuncSetAttribute, the occupancy query)
  const char* name;        // as tools/resource_notes.py prints it
  void (*launch)(const ChainLaunch&);  // hipLaunchKernelGGL of exactly this instantiation
};
// The forward-only rows (REC = false) and their kernels live in tg_kernels_fo.hip, the
// traced ones (TRC) in tg_kernels_trc.hip, the resuming ones (RES) in tg_kernels_res.hip.
const KernelRow* fo_rows(bool mm, size_t* n);
const KernelRow* trc_rows(bool mm, size_t* n);
const KernelRow* res_rows(bool mm, size_t* n);
template <size_t A, size_t B>  // the single-model or the multi-model table of a pair
const KernelRow* pick_rows(const KernelRow (&one)[A], const KernelRow (&multi)[B], bool mm, size_t* n) {
  *n = mm ? B : A;
  return mm ? multi : one;
}

// A chain kernel's model argument and its optional ones (TraceArg, ResArg) from a launch's.
template <bool MM>
ModelArg<MM> model_arg(const ModelRef& m) {
  if constexpr (MM) return m.table;
  else return m.md;
}
template <bool ON, template <bool> class Arg>
Arg<ON> optional_arg(const Arg<true>* a) {
  if constexpr (ON) return *a;
  else return {};
}
// The launch thunk of a forward row, over tg_forward_kernel's template
// arguments (the backward's stands with its rows in tg_kernels.hip).
template <int NT, int KC, int MC, int BC, bool PHS, bool GW, bool MM = false, bool REC = true, bool TRC = false,
          bool RES = false>
void forward_thunk(const ChainLaunch& a) {
  hipLaunchKernelGGL((tg_forward_kernel<NT, KC, MC, BC, PHS, GW, MM, REC, TRC, RES>), dim3(a.grid), dim3(NT), a.lds,
                     a.stream, model_arg<MM>(a.m), a.chains, a.E, a.ws, a.out.status, a.out.log_z,
                     a.out.final_log_weights, a.lay, a.dbg, a.ws, optional_arg<TRC, TraceArg>(a.trace),
                     optional_arg<RES, ResArg>(a.res));
}

// A row's flags from the template arguments behind PHS that the row spells out.
template <bool GW, bool MM = false, bool REC = true, bool TRC = false, bool RES = false>
struct RowFlags { static constexpr bool gw = GW, mm = MM, rec = REC, trc = TRC, res = RES; };
// TG_ROW(forward | backward, NT, KC, MC, BC, PHS, GW[,MM[,REC[,TRC[,RES]]]]): a
// row from its kernel's template arguments: threads, K, M, B (0: any shape),
// phase timers, GW, then the later ones up to the last not at its default. The
// name is the list as written, so those behind GW are written without blanks.
// The row mentions its kernel itself, ahead of the thunk: the kernels stand in
// the code object in the order of first mention.
#define TG_ROW(DIR, NT, KC, MC, BC, PHS, ...)                                                             \
  {NT, Shape(KC), PHS, RowFlags<__VA_ARGS__>::gw, RowFlags<__VA_ARGS__>::mm, RowFlags<__VA_ARGS__>::rec,  \
   RowFlags<__VA_ARGS__>::trc, RowFlags<__VA_ARGS__>::res,                                                \
   (const void*)&tg_##DIR##_kernel<NT, KC, MC, BC, PHS, __VA_ARGS__>,                                     \
   "tg_" #DIR "_kernel<" #NT "," #KC "," #MC "," #BC "," #PHS "," #__VA_ARGS__ ">",                       \
   &DIR##_thunk<NT, KC, MC, BC, PHS, __VA_ARGS__>}
// The builds of every table but the full single-model ones, X(NT, KC, MC, BC,
// GW): every width's generic build, the generic GW one at 256 and the two
// compiled shapes at their widths. No phase-timer builds (see find_row).
#define TG_PLAIN_BUILDS(X)                                                                                  \
  X(64, 0, 0, 0, false)     X(128, 0, 0, 0, false)    X(256, 0, 0, 0, true)     X(256, 6, 50, 25, false)  \
  X(256, 0, 0, 0, false)    X(768, 6, 50, 25, false)  X(768, 12, 50, 25, false) X(768, 0, 0, 0, false)    \
  X(512, 6, 50, 25, false)  X(512, 12, 50, 25, false) X(512, 0, 0, 0, false)

}  // namespace hyg
