// k_warp_bf16.hip -- the fast warp's bf16 (CV_16BF) store instantiations: k_warp.hip compiled with CVGS_WARP_BF16_TU, which keeps its
// templates and replaces the launch entry points by warp_fast_launch_bf16 (the fp16 kernels' twins with OT = __bf16).
#define CVGS_WARP_BF16_TU 1
#include "k_warp.hip"
