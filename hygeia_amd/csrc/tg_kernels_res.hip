// tg_kernels_res.hip -- the resuming builds of tg_forward_kernel (template flag
// RES = true, tg_forward.h) and their row table, res_rows, in a translation
// unit of their own, as tg_kernels_fo.hip / tg_kernels_trc.hip hold the
// forward-only ones: the 4 instantiations (the pipeline's compiled shape and
// the generic build at 256 threads, single-model and multi-model) compile
// beside the chain kernels of tg_kernels.hip instead of behind them.
#include "tg_rows.h"

namespace hyg {

// RES builds (their names carry all ten arguments) at 256 threads, the one
// width whose launches are cut in time (forward_schedule).
#define RS(NT, KC, MC, BC) TG_ROW(forward, NT, KC, MC, BC, false, false,false,true,false,true)
#define RS_MM(NT, KC, MC, BC) TG_ROW(forward, NT, KC, MC, BC, false, false,true,true,false,true)
static const KernelRow kResRows[] = {RS(256, 6, 50, 25), RS(256, 0, 0, 0)};
static const KernelRow kResRowsMm[] = {RS_MM(256, 6, 50, 25), RS_MM(256, 0, 0, 0)};
const KernelRow* res_rows(bool mm, size_t* n) { return pick_rows(kResRows, kResRowsMm, mm, n); }

}  // namespace hyg
