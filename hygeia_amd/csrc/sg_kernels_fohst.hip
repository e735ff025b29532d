// sg_kernels_fohst.hip -- the history builds of sg_chain_kernel (template flags
// MM, FO and HST, sg_kernels.hip) and their launch, sg_launch_history_multi:
// 15 instantiations (K = 2 .. 16), multi-model and untraced only.
#define HYG_SG_FO_TU 3
#include "sg_kernels.hip"
