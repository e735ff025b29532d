// tg_kernels_trc.hip -- the traced forward-only builds of tg_forward_kernel
// (template flags REC = false, TRC = true, tg_forward.h) and their row table,
// trc_rows, in a translation unit of their own, as tg_kernels_fo.hip holds the
// plain forward-only ones: the 22 instantiations (11 single-model, 11
// multi-model) compile beside the chain kernels of tg_kernels.hip instead of
// behind them.
#include "tg_rows.h"

namespace hyg {

// The plain builds of tg_rows.h, as the forward-only ones, with TRC: their names carry all nine arguments.
#define TR(NT, KC, MC, BC, GW) TG_ROW(forward, NT, KC, MC, BC, false, GW,false,false,true),
#define TR_MM(NT, KC, MC, BC, GW) TG_ROW(forward, NT, KC, MC, BC, false, GW,true,false,true),
static const KernelRow kTrcRows[] = {TG_PLAIN_BUILDS(TR)};
static const KernelRow kTrcRowsMm[] = {TG_PLAIN_BUILDS(TR_MM)};
const KernelRow* trc_rows(bool mm, size_t* n) { return pick_rows(kTrcRows, kTrcRowsMm, mm, n); }

}  // namespace hyg
