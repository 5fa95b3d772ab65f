// k_nv12_bf16.hip -- K4's bf16 (CV_16BF) store instantiations: k_nv12.hip compiled with CVGS_K4_BF16_TU, which keeps its templates and
// replaces launch_nv12 by k4_launch_bf16 (the fp16 kernels' twins with OT = __bf16).
#define CVGS_K4_BF16_TU 1
#include "k_nv12.hip"
