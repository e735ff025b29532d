// tg_kernels_trc.hip -- the traced forward-only builds of tg_forward_kernel
// (template flags REC = false, TRC = true, tg_kernels.hip) and their row table,
// trc_rows, in a translation unit of their own, as tg_kernels_fo.hip holds the
// plain forward-only ones: the 22 instantiations (11 single-model, 11
// multi-model) compile beside the chain kernels of tg_kernels.hip instead of
// behind them.
#define HYG_TG_FO_TU 1
#define HYG_TG_TRC_TU 1
#include "tg_kernels.hip"
