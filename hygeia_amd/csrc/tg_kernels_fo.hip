// tg_kernels_fo.hip -- the forward-only builds of tg_forward_kernel (template
// flag REC = false, tg_forward.h) and their row table, fo_rows, in a
// translation unit of their own: the 22 instantiations (11 single-model, 11
// multi-model) compile beside the 60 chain kernels of tg_kernels.hip instead
// of behind them.
#include "tg_rows.h"

namespace hyg {

// The plain builds of tg_rows.h with REC = false: their names carry all eight arguments.
#define FO(NT, KC, MC, BC, GW) TG_ROW(forward, NT, KC, MC, BC, false, GW,false,false),
#define FO_MM(NT, KC, MC, BC, GW) TG_ROW(forward, NT, KC, MC, BC, false, GW,true,false),
static const KernelRow kFoRows[] = {TG_PLAIN_BUILDS(FO)};
static const KernelRow kFoRowsMm[] = {TG_PLAIN_BUILDS(FO_MM)};
const KernelRow* fo_rows(bool mm, size_t* n) { return pick_rows(kFoRows, kFoRowsMm, mm, n); }

}  // namespace hyg
