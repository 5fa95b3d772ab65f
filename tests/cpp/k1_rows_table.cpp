// k1_rows_table.cpp -- k1_rows_instantiated (cvgpuspeedup_amd/csrc/k_k1_impl.hpp), the one mapping from the rows per wave a K1 launch
// asks for to the rows per wave of the kernel that exists, held to a table written out line by line for EVERY combination of its
// arguments.  Host only: the header's first section is plain C++ (CVGS_K1_ROWS_ONLY keeps the kernels out), nothing here touches the HIP
// runtime.  tests/test_k1_rows_cases.py builds and runs it; tests/test_gpu_k1_rows.py holds the launches themselves to the same table
// through the "@rN" suffix of cvgs_kernel_name.
//
// The table by launcher (requested 1 / 2 / 4 -> instantiated):
//   mirrored launches 1 / 1 / 1;  launch_other (packed pixels, separate planes) 1 / 1 / 4;  interpreted programs into a planar tensor
//   1 / 1 / 1;  launch_few_planar (1 / 2 channels, compile-time programs) 1 / 1 / 4;  launch_rpw, 16-bit / fp32 sources 1 / 4 / 4;
//   launch_rpw, u8 sources 1 / 2 / 4.
// Where two lines of it claim one combination, which one wins is a DECISION, taken from what launch_k1 did before the mapping was gathered
// into one function, and stated here so that a change of it is a change of this file:
//   * mirrored wins over everything (a mirrored launch is planar, u8, 3 / 4 channels: one row whatever its program);
//   * a packed / separate-plane write wins over "interpreted": launch_other has the 4-row form of InterpProg too;
//   * "interpreted" wins over "few": the interpreted 1- / 2-channel planar kernel exists with one row only.
// The 48 lines below hold every combination, those launch_k1 never forms included (mirrored with a packed write, 1 / 2 channels with a
// mirrored write ...): the function is total, and its answer there is the line's, by the same precedence.
#define CVGS_K1_ROWS_ONLY
#include "../../cvgpuspeedup_amd/csrc/k_k1_impl.hpp"

#include <cstdio>

namespace {

struct Line {
    int mirrored, wm, interpreted, few, src_u8;
    int want[3]; // asked for 1 / 2 / 4
};
const Line kTable[] = {
    // mirrored, write mode, interpreted, few, u8 source -> rows
    {0, cvgs::WM_PLANAR , 0, 0, 0, {1, 4, 4}},
    {0, cvgs::WM_PLANAR , 0, 0, 1, {1, 2, 4}},
    {0, cvgs::WM_PLANAR , 0, 1, 0, {1, 1, 4}},
    {0, cvgs::WM_PLANAR , 0, 1, 1, {1, 1, 4}},
    {0, cvgs::WM_PLANAR , 1, 0, 0, {1, 1, 1}},
    {0, cvgs::WM_PLANAR , 1, 0, 1, {1, 1, 1}},
    {0, cvgs::WM_PLANAR , 1, 1, 0, {1, 1, 1}},
    {0, cvgs::WM_PLANAR , 1, 1, 1, {1, 1, 1}},
    {0, cvgs::WM_PACKED , 0, 0, 0, {1, 1, 4}},
    {0, cvgs::WM_PACKED , 0, 0, 1, {1, 1, 4}},
    {0, cvgs::WM_PACKED , 0, 1, 0, {1, 1, 4}},
    {0, cvgs::WM_PACKED , 0, 1, 1, {1, 1, 4}},
    {0, cvgs::WM_PACKED , 1, 0, 0, {1, 1, 4}},
    {0, cvgs::WM_PACKED , 1, 0, 1, {1, 1, 4}},
    {0, cvgs::WM_PACKED , 1, 1, 0, {1, 1, 4}},
    {0, cvgs::WM_PACKED , 1, 1, 1, {1, 1, 4}},
    {0, cvgs::WM_SPLIT2D, 0, 0, 0, {1, 1, 4}},
    {0, cvgs::WM_SPLIT2D, 0, 0, 1, {1, 1, 4}},
    {0, cvgs::WM_SPLIT2D, 0, 1, 0, {1, 1, 4}},
    {0, cvgs::WM_SPLIT2D, 0, 1, 1, {1, 1, 4}},
    {0, cvgs::WM_SPLIT2D, 1, 0, 0, {1, 1, 4}},
    {0, cvgs::WM_SPLIT2D, 1, 0, 1, {1, 1, 4}},
    {0, cvgs::WM_SPLIT2D, 1, 1, 0, {1, 1, 4}},
    {0, cvgs::WM_SPLIT2D, 1, 1, 1, {1, 1, 4}},
    {1, cvgs::WM_PLANAR , 0, 0, 0, {1, 1, 1}},
    {1, cvgs::WM_PLANAR , 0, 0, 1, {1, 1, 1}},
    {1, cvgs::WM_PLANAR , 0, 1, 0, {1, 1, 1}},
    {1, cvgs::WM_PLANAR , 0, 1, 1, {1, 1, 1}},
    {1, cvgs::WM_PLANAR , 1, 0, 0, {1, 1, 1}},
    {1, cvgs::WM_PLANAR , 1, 0, 1, {1, 1, 1}},
    {1, cvgs::WM_PLANAR , 1, 1, 0, {1, 1, 1}},
    {1, cvgs::WM_PLANAR , 1, 1, 1, {1, 1, 1}},
    {1, cvgs::WM_PACKED , 0, 0, 0, {1, 1, 1}},
    {1, cvgs::WM_PACKED , 0, 0, 1, {1, 1, 1}},
    {1, cvgs::WM_PACKED , 0, 1, 0, {1, 1, 1}},
    {1, cvgs::WM_PACKED , 0, 1, 1, {1, 1, 1}},
    {1, cvgs::WM_PACKED , 1, 0, 0, {1, 1, 1}},
    {1, cvgs::WM_PACKED , 1, 0, 1, {1, 1, 1}},
    {1, cvgs::WM_PACKED , 1, 1, 0, {1, 1, 1}},
    {1, cvgs::WM_PACKED , 1, 1, 1, {1, 1, 1}},
    {1, cvgs::WM_SPLIT2D, 0, 0, 0, {1, 1, 1}},
    {1, cvgs::WM_SPLIT2D, 0, 0, 1, {1, 1, 1}},
    {1, cvgs::WM_SPLIT2D, 0, 1, 0, {1, 1, 1}},
    {1, cvgs::WM_SPLIT2D, 0, 1, 1, {1, 1, 1}},
    {1, cvgs::WM_SPLIT2D, 1, 0, 0, {1, 1, 1}},
    {1, cvgs::WM_SPLIT2D, 1, 0, 1, {1, 1, 1}},
    {1, cvgs::WM_SPLIT2D, 1, 1, 0, {1, 1, 1}},
    {1, cvgs::WM_SPLIT2D, 1, 1, 1, {1, 1, 1}},
};

} // namespace

int main() {
    int checked = 0, bad = 0;
    const int asked[3] = {1, 2, 4}, other[6] = {-1, 0, 3, 5, 8, 64};
    bool seen[2][3][2][2][2] = {};
    for (const Line& l : kTable) {
        if (seen[l.mirrored][l.wm][l.interpreted][l.few][l.src_u8]) {
            std::printf("FAILED: a combination is listed twice\n");
            ++bad;
        }
        seen[l.mirrored][l.wm][l.interpreted][l.few][l.src_u8] = true;
        for (int k = 0; k < 3; ++k, ++checked) {
            const int got = cvgs::k1_rows_instantiated(l.interpreted, l.src_u8, l.wm, l.few, l.mirrored, asked[k]);
            if (got != l.want[k]) {
                std::printf("FAILED: mirrored %d wm %d interpreted %d few %d u8 %d asked %d -> %d, the table says %d\n", l.mirrored, l.wm, l.interpreted, l.few,
                            l.src_u8, asked[k], got, l.want[k]);
                ++bad;
            }
        }
        // anything but 1 / 2 / 4 is no request: 0, which every launcher refuses (hipErrorInvalidValue)
        for (int o : other)
            if (cvgs::k1_rows_instantiated(l.interpreted, l.src_u8, l.wm, l.few, l.mirrored, o) != 0) {
                std::printf("FAILED: asked %d must give 0\n", o);
                ++bad;
            }
    }
    std::printf("%d answers checked, %d wrong\n", checked, bad);
    if (bad || checked != 48 * 3) return 1;
    std::printf("k1_rows_table passed!!\n");
    return 0;
}
