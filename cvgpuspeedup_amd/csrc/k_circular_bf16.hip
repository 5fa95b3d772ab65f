// k_circular_bf16.hip -- the single-launch CircularTensor update's bf16 (CV_16BF) store instantiations: k_circular.hip compiled with
// CVGS_CIRC_BF16_TU, which keeps its templates and replaces the launch entry points by circ_push_launch_bf16 (OT = __bf16).
#define CVGS_CIRC_BF16_TU 1
#include "k_circular.hip"
