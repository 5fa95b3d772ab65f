// k_yuv422_bf16.hip -- the packed 4:2:2 resize kernels' bf16 (CV_16BF) store instantiations: k_yuv422.hip compiled with CVGS_Y422_BF16_TU,
// which keeps its templates and replaces launch_yuv422 by y422_launch_bf16 (the fp16 kernels' twins with OT = __bf16).
#define CVGS_Y422_BF16_TU 1
#include "k_yuv422.hip"
