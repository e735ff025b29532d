// sg_kernels_fo.hip -- the forward-only builds of sg_chain_kernel (template
// flags FO and TRC, sg_kernels.hip) for single-model launches and their launch,
// sg_launch_filter, in a translation unit of their own: 30 instantiations
// (K = 2 .. 16, untraced and traced) that compile beside the full builds. The
// multi-model ones are in sg_kernels_fomm.hip.
#define HYG_SG_FO_TU 1
#include "sg_kernels.hip"
