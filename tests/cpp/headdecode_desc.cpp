// cvGS::DeviceHeadDecode without a GPU (tests/test_head_decode.py): the facade compiles, the caller-owned spelling allocates nothing and
// lowers to a cvgs_head_desc whose bytes the test compares with the Python binding's; feed() points a DeviceBoxSelect at the decoder's
// outputs.  Makes no HIP call.
#include <cstdio>

#include "cvGPUSpeedup.h"

static void dump(const char* name, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    std::printf("%s ", name);
    for (size_t i = 0; i < n; ++i) std::printf("%02x", b[i]);
    std::printf("\n");
}

int main() {
    // pretend device addresses: nothing is dereferenced
    auto at = [](uintptr_t a) { return reinterpret_cast<void*>(a); };
    auto fp = [&](uintptr_t a) { return static_cast<float*>(at(a)); };
    auto ip = [&](uintptr_t a) { return static_cast<int32_t*>(at(a)); };
    // a bf16 [4 + 80, 8400] head
    cvGS::DeviceHeadDecode dec(8400, at(0x100000), fp(0x200000), fp(0x300000), ip(0x400000), ip(0x500000), ip(0x600000));
    dec.layout(at(0x10000), CVGS_HEAD_BF16, 1, 8400, 80).threshold(0.25f);
    if (dec.boxes() != at(0x200000) || dec.scores() != at(0x300000) || dec.classes() != at(0x400000) || dec.count() != at(0x500000) ||
        dec.indices() != at(0x600000) || dec.maxCandidates() != 8400)
        return 1;
    dump("desc", &dec.desc(), sizeof(cvgs_head_desc));
    // an fp32 [N, 5 + 3] head with objectness, two leading attributes, no index output
    cvGS::DeviceHeadDecode rows(1000, at(0x100000), fp(0x200000), fp(0x300000), ip(0x400000), ip(0x500000));
    rows.layout(at(0x10000), CVGS_HEAD_F32, 10, 1, 3, 2, 7, 6).threshold(0.5f);
    dump("rows", &rows.desc(), sizeof(cvgs_head_desc));
    // feed(): the selector reads the decoder's outputs and its device count
    cvGS::DeviceBoxSelect sel(cv::Size(1920, 1080), 8400, 1024, 50, at(0x700000), fp(0x800000), ip(0x800400));
    sel.thresholds(0.25f, 0.5f);
    dec.feed(sel, CVGS_CAND_CXCYWH_F32);
    dump("select", &sel.desc(), sizeof(cvgs_box_select_desc));
    cvGS::DeviceBoxSelect other(cv::Size(1920, 1080), 100, 64, 50, at(0x700000), fp(0x800000), ip(0x800400));
    try {
        dec.feed(other);
        return 2; // a selector of another size must be refused
    } catch (const std::runtime_error&) {
    }
    return 0;
}
