// k_pointwise_bf16.hip -- the thread-fused pointwise kernel's bf16 (CV_16BF) store instantiations: k_pointwise.hip compiled with
// CVGS_PW_BF16_TU, which keeps its templates and replaces the launch entry points by pw_launch_bf16 (the fp16 kernels' twins, OT = __bf16).
#define CVGS_PW_BF16_TU 1
#include "k_pointwise.hip"
