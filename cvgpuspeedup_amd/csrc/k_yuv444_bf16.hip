// k_yuv444_bf16.hip -- the planar 4:4:4 resize kernels' bf16 (CV_16BF) store instantiations: k_yuv444.hip compiled with CVGS_Y444_BF16_TU,
// which keeps its templates and replaces launch_yuv444 by y444_launch_bf16 (the fp16 kernels' twins with OT = __bf16).
#define CVGS_Y444_BF16_TU 1
#include "k_yuv444.hip"
