// sg_kernels_mm.hip -- the multi-model builds of sg_chain_kernel (template flag
// MM, sg_kernels.hip) and their launch, sg_launch_chains_multi, in a
// translation unit of their own: the 30 instantiations (K = 2 .. 16, with and
// without parameter estimation) compile beside the 32 single-model ones
// instead of behind them.
#define HYG_SG_MM_TU 1
#include "sg_kernels.hip"
