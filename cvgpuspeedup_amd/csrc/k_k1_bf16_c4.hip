// k_k1_bf16_c4.hip -- K1's bf16 store instantiations for 4-channel sources (see k_k1_bf16.hpp).
#include "k_k1_bf16.hpp"

namespace cvgs {

hipError_t k1_launch_bf16_c4(int mode, int prog_id, bool canon, bool table, int rows, const ChainArgs& c, const PlaneParams* ip, int ni, int out_cn,
                              LaunchCtx& s) {
    return k1_launch_bf16<4>(mode, prog_id, canon, table, rows, c, ip, ni, out_cn, s);
}

} // namespace cvgs
