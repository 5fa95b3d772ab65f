// The host file of cvgs_warp_tables_from_boxes (csrc/cvgs_boxwarp.cpp) as a stand-alone program for AddressSanitizer + UBSan: no HIP, no
// library (tests/test_box_warp_asan.py builds and runs it).  The file is compiled INTO this program; cvgs::fail / cvgs::hip_fail record code
// and text here and the launcher keeps the frames it is handed.  Hostile boxes -- NaN, +-inf, +-FLT_MAX, denormals, inverted, empty -- go
// through cvgs_warp_table_from_boxes_host over heap buffers of exactly the size the contract states, so that the sanitizer guards their
// ends; every count from -2 to max_items + 2.  The last line is the verdict: "N checks, 0 bad".
#include "../../cvgpuspeedup_amd/csrc/cvgs_boxwarp.cpp"

#include <cfloat>
#include <cstdio>
#include <memory>
#include <vector>

namespace {
int g_code = 0;
std::string g_text;
std::vector<BoxWarpFrame> g_frames;
} // namespace

namespace cvgs {
int fail(int code, const std::string& msg) { g_code = code; g_text = msg; return code; }
int hip_fail(int hip_error, const char* what) { return fail(CVGS_ERR_HIP, std::string(what) + ": hip error " + std::to_string(hip_error)); }
int launch_box_warps(const BoxWarpFrame* f, int n, void*) { g_frames.assign(f, f + n); return 0; }
} // namespace cvgs

namespace {
int checks = 0, bad = 0;
void expect(bool ok, const char* what, int line) {
    ++checks;
    if (!ok) { ++bad; std::printf("WRONG line %d: %s   (last text: %s)\n", line, what, g_text.c_str()); }
}
#define EXPECT(c) expect((c), #c, __LINE__)

cvgs_box_warp_desc desc(int max_items, int shape, int dw, int dh) {
    cvgs_box_warp_desc d{};
    d.struct_size = sizeof(d);
    d.frame = cvgs_image2d{(const void*)0x10000, 97, 61, 304, 0}; // a pretend device address: never dereferenced
    d.src_type = CVGS_MAKETYPE(CVGS_DEPTH_8U, 3);
    d.read_kind = CVGS_READ_WARP_AFFINE;
    d.dst_width = dw; d.dst_height = dh;
    d.shape = shape; d.max_items = max_items;
    d.scale[0] = 1.25f; d.scale[1] = 1.25f; d.pad[0] = 0.f; d.pad[1] = 3.5f;
    return d;
}
} // namespace

int main() {
    const float nan = std::nanf(""), inf = INFINITY, big = FLT_MAX, tiny = 1e-42f;
    const float values[] = {0.f, -0.f, 1.f, -7.5f, 40.f, 1e6f, nan, inf, -inf, big, -big, tiny, -tiny, 3e38f};
    const int nv = (int)(sizeof(values) / sizeof(values[0]));
    std::vector<float> hostile; // every pair of values on the x axis against a good y axis, and on the y axis against a good x axis
    for (int a = 0; a < nv; ++a)
        for (int b = 0; b < nv; ++b) {
            const float x[4] = {values[a], 5.f, values[b], 50.f}, y[4] = {10.f, values[a], 40.f, values[b]};
            hostile.insert(hostile.end(), x, x + 4);
            hostile.insert(hostile.end(), y, y + 4);
        }
    const int n = (int)hostile.size() / 4;
    const int targets[][2] = {{1, 1}, {8, 6}, {192, 256}, {1 << 24, 1}};
    for (int shape = 0; shape < 2; ++shape)
        for (const auto& t : targets)
            for (int count = -2; count <= n + 2; count += (count < 2 || count >= n - 2) ? 1 : n / 5) {
                // heap buffers of exactly the contract's size
                std::unique_ptr<float[]> boxes(new float[(size_t)n * 4]);
                std::memcpy(boxes.get(), hostile.data(), (size_t)n * 4 * sizeof(float));
                std::unique_ptr<int32_t> cnt(new int32_t(count));
                std::unique_ptr<uint8_t[]> table(new uint8_t[(size_t)n * 64]);
                std::unique_ptr<float[]> rect(new float[(size_t)n * 4]);
                std::unique_ptr<int32_t[]> valid(new int32_t[(size_t)n]);
                cvgs_box_warp_desc d = desc(n, shape, t[0], t[1]);
                d.boxes = boxes.get(); d.count = cnt.get();
                EXPECT(cvgs_warp_table_from_boxes_host(&d, table.get(), rect.get(), valid.get()) == CVGS_OK);
                const int live = count < 0 ? 0 : (count > n ? n : count);
                int n_valid = 0;
                bool ok = true;
                for (int i = 0; i < n; ++i) {
                    WarpPlane P;
                    std::memcpy(&P, table.get() + (size_t)i * 64, 64);
                    ok = ok && P.w == 97 && P.h == 61 && P.step == 304 && P.dw == t[0] && P.dh == t[1] && (valid[i] == 0 || valid[i] == 1);
                    for (int k = 0; k < 9; ++k) ok = ok && fit_finite((double)P.m[k]); // an entry never carries NaN or inf
                    if (!valid[i]) ok = ok && P.m[2] == -1.f && P.m[5] == -1.f && P.m[0] == 0.f && rect[(size_t)i * 4] == 0.f && rect[(size_t)i * 4 + 3] == 0.f;
                    if (i >= live) ok = ok && !valid[i];
                    n_valid += valid[i];
                }
                EXPECT(ok);
                EXPECT(count <= 0 ? n_valid == 0 : true);
                // the optional outputs absent
                std::unique_ptr<uint8_t[]> table2(new uint8_t[(size_t)n * 64]);
                EXPECT(cvgs_warp_table_from_boxes_host(&d, table2.get(), nullptr, nullptr) == CVGS_OK && std::memcmp(table.get(), table2.get(), (size_t)n * 64) == 0);
            }
    // one item, one buffer each; the device entry point lowers a good descriptor into the frame the launcher sees
    {
        std::unique_ptr<float[]> one(new float[4]{10.f, 5.f, 40.f, 50.f});
        std::unique_ptr<uint8_t[]> table(new uint8_t[64]);
        std::unique_ptr<float[]> rect(new float[4]);
        std::unique_ptr<int32_t[]> valid(new int32_t[1]);
        cvgs_box_warp_desc d = desc(1, CVGS_BOX_SHAPE_STRETCH, 30, 45);
        d.scale[0] = d.scale[1] = 1.f; d.pad[1] = 0.f;
        d.boxes = one.get();
        EXPECT(cvgs_warp_table_from_boxes_host(&d, table.get(), rect.get(), valid.get()) == CVGS_OK && valid[0] == 1);
        WarpPlane P;
        std::memcpy(&P, table.get(), 64);
        EXPECT(P.m[0] == 1.f && P.m[2] == 10.f && P.m[4] == 1.f && P.m[5] == 5.f && rect[0] == 10.f && rect[3] == 50.f);
        cvgs_box_warp_desc descs[16];
        for (int k = 0; k < 16; ++k) {
            descs[k] = desc(100 + k, k & 1, 192, 256);
            descs[k].boxes = (const float*)(uintptr_t)(0x100000 + 0x10000 * k);
            descs[k].table_out = (void*)(uintptr_t)(0x1000000 + 0x10000 * k);
            descs[k].boxes_out = (float*)(uintptr_t)(0x2000000 + 0x10000 * k);
            descs[k].valid_out = (int32_t*)(uintptr_t)(0x3000000 + 0x10000 * k);
        }
        EXPECT(cvgs_warp_tables_from_boxes(descs, 16, nullptr) == CVGS_OK && g_frames.size() == 16);
        EXPECT(g_frames[15].max_items == 115 && g_frames[15].shape == 1 && g_frames[15].valid == descs[15].valid_out && g_frames[3].boxes == descs[3].boxes);
        descs[7].valid_out = (int32_t*)((uintptr_t)descs[6].table_out + 64 * 105); // the last entry of frame 6's table
        EXPECT(cvgs_warp_tables_from_boxes(descs, 16, nullptr) == CVGS_ERR_INVALID && g_text.find("overlap") != std::string::npos);
    }
    std::printf("%d checks, %d bad\n", checks, bad);
    return bad ? 1 : 0;
}
