// cvGS::DevicePointGather without a GPU (tests/test_point_gather.py): the facade compiles, the caller-owned spelling allocates nothing and
// lowers to a cvgs_point_gather_desc whose bytes the test compares with the Python binding's; from() takes the selector's indices and
// count and the decoder's indices, and refuses objects of another size or without indices.  Makes no HIP call.
#include <cstdio>

#include "cvGPUSpeedup.h"

static void dump(const char* name, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    std::printf("%s ", name);
    for (size_t i = 0; i < n; ++i) std::printf("%02x", b[i]);
    std::printf("\n");
}

template <typename F>
static bool throws(F f) {
    try {
        f();
    } catch (const std::runtime_error&) {
        return true;
    }
    return false;
}

int main() {
    // pretend device addresses: nothing is dereferenced
    auto at = [](uintptr_t a) { return reinterpret_cast<void*>(a); };
    auto fp = [&](uintptr_t a) { return static_cast<float*>(at(a)); };
    auto ip = [&](uintptr_t a) { return static_cast<int32_t*>(at(a)); };
    cvGS::DeviceHeadDecode dec(8400, at(0x100000), fp(0x200000), fp(0x300000), ip(0x400000), ip(0x500000), ip(0x600000));
    cvGS::DeviceBoxSelect sel(cv::Size(1920, 1080), 8400, 1024, 50, at(0x700000), fp(0x800000), ip(0x800400), fp(0x800600), ip(0x800800));
    // a bf16 [4 + 1 + 5 * 3, 8400] head: x, y, confidence from attribute 5; through select's and decode's indices
    cvGS::DevicePointGather gather(8400, 50, 5, fp(0x900000), fp(0xA00000), ip(0xB00000));
    gather.layout(at(0x10000), CVGS_HEAD_BF16, 1, 8400, 5, 3, 2).transform(3.0f, 1.6875f, 0.0f, -20.0f).from(sel, dec);
    if (gather.points() != at(0x900000) || gather.count() != at(0x800400) || gather.conf() != at(0xA00000) || gather.source() != at(0xB00000) ||
        gather.maxOut() != 50 || gather.nPoints() != 5)
        return 1;
    dump("desc", &gather.desc(), sizeof(cvgs_point_gather_desc));
    // an fp32 [8400, 4 + 1 + 5 * 2] head selected in place: select's indices are raw candidate indices
    cvGS::DevicePointGather direct(8400, 50, 5, fp(0x900000));
    direct.layout(at(0x10000), CVGS_HEAD_F32, 15, 1, 5, 2).from(sel);
    dump("direct", &direct.desc(), sizeof(cvgs_point_gather_desc));
    // from() refuses another maxOut / maxCandidates and objects built without indices
    cvGS::DeviceBoxSelect fewer(cv::Size(1920, 1080), 8400, 1024, 40, at(0x700000), fp(0x800000), ip(0x800400), fp(0x800600), ip(0x800800));
    cvGS::DeviceBoxSelect smaller(cv::Size(1920, 1080), 100, 64, 50, at(0x700000), fp(0x800000), ip(0x800400), fp(0x800600), ip(0x800800));
    cvGS::DeviceBoxSelect blind(cv::Size(1920, 1080), 8400, 1024, 50, at(0x700000), fp(0x800000), ip(0x800400));
    cvGS::DeviceHeadDecode other(100, at(0x100000), fp(0x200000), fp(0x300000), ip(0x400000), ip(0x500000), ip(0x600000));
    cvGS::DeviceHeadDecode mute(8400, at(0x100000), fp(0x200000), fp(0x300000), ip(0x400000), ip(0x500000));
    if (!throws([&] { gather.from(fewer); }) || !throws([&] { gather.from(smaller); }) || !throws([&] { gather.from(blind); }) ||
        !throws([&] { gather.from(sel, other); }) || !throws([&] { gather.from(sel, mute); }))
        return 2;
    return 0;
}
