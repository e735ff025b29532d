// tg_kernels_res.hip -- the resuming builds of tg_forward_kernel (template flag
// RES = true, tg_kernels.hip) and their row table, res_rows, in a translation
// unit of their own, as tg_kernels_fo.hip / tg_kernels_trc.hip hold the
// forward-only ones: the 4 instantiations (the pipeline's compiled shape and
// the generic build at 256 threads, single-model and multi-model) compile
// beside the chain kernels of tg_kernels.hip instead of behind them.
#define HYG_TG_FO_TU 1
#define HYG_TG_RES_TU 1
#include "tg_kernels.hip"
