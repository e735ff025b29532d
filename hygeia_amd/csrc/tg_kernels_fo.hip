// tg_kernels_fo.hip -- the forward-only builds of tg_forward_kernel (template
// flag REC = false, tg_kernels.hip) and their row table, fo_rows, in a
// translation unit of their own: the 22 instantiations (11 single-model, 11
// multi-model) compile beside the 60 chain kernels of tg_kernels.hip instead
// of behind them.
#define HYG_TG_FO_TU 1
#include "tg_kernels.hip"
