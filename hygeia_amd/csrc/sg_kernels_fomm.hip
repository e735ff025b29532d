// sg_kernels_fomm.hip -- the multi-model forward-only builds of sg_chain_kernel
// (template flags MM, FO and TRC, sg_kernels.hip) and their launch,
// sg_launch_filter_multi: 30 instantiations (K = 2 .. 16, untraced and traced).
#define HYG_SG_FO_TU 2
#include "sg_kernels.hip"
