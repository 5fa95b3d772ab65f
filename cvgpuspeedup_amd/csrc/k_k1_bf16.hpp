// k_k1_bf16.hpp -- K1's bf16 (CV_16BF) store instantiations: the fp16 twins' kernels (k_k1.hip, k_k1_c3.hip, k_k1_c4.hip) with
// OT = __bf16, so every store converts with v_cvt_pk_bf16_f32.  Instantiated per channel count in k_k1_bf16_c3.hip / k_k1_bf16_c4.hip
// (parallel compilation); launch_k1 (k_k1.hip) picks the mode.
#pragma once
#include "k_k1_impl.hpp"

namespace cvgs {

enum K1Bf16Mode { K1_BF16_PLANAR = 0, K1_BF16_PACKED = 1, K1_BF16_MIRRORED = 2 };

// PLANAR: planar tensor (NCHW / CNHW; single chains, cvgs_execute_many ticks, host or device tables), prog_id = the planar program;
// PACKED: packed pixels (canon: the chain was rewritten into the canonical pipeline); MIRRORED: planar tensor + cvgs_write_desc.mirrors,
// planes in the kernel arguments, prog_id = k1_classify_program's answer
template <int CN>
static hipError_t k1_launch_bf16(int mode, int prog_id, bool canon, bool table, int rows, const ChainArgs& c, const PlaneParams* ip, int ni, int out_cn,
                                 LaunchCtx& s) {
    if (mode == K1_BF16_PACKED) return launch_other_np<CN, __bf16, WM_PACKED>(false, table, rows, c, ip, ni, s, canon);
    if (mode == K1_BF16_MIRRORED) {
        auto mir = [&](auto prog_tag) {
            using Pg = decltype(prog_tag);
            if (ni > CVGS_KERNARG_PLANES) return launch_t<CN, kKernargPlanesBig, 1, Pg, SRC_U8, __bf16, WM_PLANAR, true>(c, ip, ni, out_cn, s);
            return launch_t<CN, CVGS_KERNARG_PLANES, 1, Pg, SRC_U8, __bf16, WM_PLANAR, true>(c, ip, ni, out_cn, s);
        };
        return prog_id == 0 ? mir(ProgSwapMulSubDiv{}) : (prog_id == 1 ? mir(ProgMulSubDiv{}) : mir(InterpProg{}));
    }
    return launch_prog<CN, SRC_U8, __bf16>(prog_id, table, rows, c, ip, ni, out_cn, s);
}

} // namespace cvgs
