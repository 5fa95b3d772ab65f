// cvGS::DeviceBoxSelect without a GPU (tests/test_box_select.py): the facade compiles, the caller-owned spelling allocates nothing and
// lowers to a cvgs_box_select_desc whose bytes the test compares with the Python binding's; what boxes() / count() return is what
// cvGS::DeviceCrops::update takes.  Makes no HIP call.
#include <cstdio>

#include "cvGPUSpeedup.h"

int main() {
    // pretend device addresses: nothing is dereferenced
    auto at = [](uintptr_t a) { return reinterpret_cast<void*>(a); };
    const float* head = static_cast<const float*>(at(0x10000));
    cvGS::DeviceBoxSelect sel(cv::Size(1920, 1080), 8400, 1024, 50, at(0x20000), static_cast<float*>(at(0x30000)), static_cast<int32_t*>(at(0x30400)),
                              static_cast<float*>(at(0x30800)), static_cast<int32_t*>(at(0x30c00)));
    sel.candidates(head, 6, head + 4, 6, CVGS_CAND_CXCYWH_F32, static_cast<const int32_t*>(at(0x10014)), 6, static_cast<const int32_t*>(at(0x40000)))
        .thresholds(0.25f, 0.5f)
        .transform(3.0f, 3.0f, 0.0f, -420.0f);
    if (sel.boxes() != at(0x30000) || sel.count() != at(0x30400) || sel.scores() != at(0x30800) || sel.indices() != at(0x30c00) || sel.maxOut() != 50) return 1;
    const cvgs_box_select_desc& d = sel.desc();
    const unsigned char* b = reinterpret_cast<const unsigned char*>(&d);
    std::printf("desc ");
    for (size_t i = 0; i < sizeof(d); ++i) std::printf("%02x", b[i]);
    std::printf("\n");
    // the plain spelling: XYXY, dense, class-agnostic, identity transform
    cvGS::DeviceBoxSelect plain(cv::Size(640, 480), 1000, 300, 300, at(0x20000), static_cast<float*>(at(0x30000)), static_cast<int32_t*>(at(0x30400)));
    plain.candidates(head, 4, static_cast<const float*>(at(0x18000)), 1).thresholds(0.5f, 0.45f);
    const unsigned char* pb = reinterpret_cast<const unsigned char*>(&plain.desc());
    std::printf("plain ");
    for (size_t i = 0; i < sizeof(cvgs_box_select_desc); ++i) std::printf("%02x", pb[i]);
    std::printf("\n");
    return 0;
}
