// cvgs/bfloat16.h -- the host-side spelling of CV_16BF elements (engine extension: the bfloat16 hand-off).  A 2-byte standard-layout type
// that builds with g++ and hipcc alike: 16 bits of storage with round-to-nearest-even conversions from float (overflow to +-inf, NaN stays
// a quiet NaN with its sign) and the exact widening back.  A double is converted through float, the order the engine rounds in (two
// roundings, like the double -> float -> bf16 conversion it spells).  The arithmetic is the device's; the host only stores and reads.
#pragma once

#include <cstdint>
#include <cstring>
#include <type_traits>

namespace cvgs {
struct bfloat16_t {
    uint16_t bits = 0;
    bfloat16_t() = default;
    bfloat16_t(float v) : bits(from_float(v)) {}
    bfloat16_t(double v) : bits(from_float((float)v)) {}
    bfloat16_t(int v) : bits(from_float((float)v)) {}
    operator float() const { return to_float(bits); }

    static bfloat16_t from_bits(uint16_t b) {
        bfloat16_t r;
        r.bits = b;
        return r;
    }
    static uint16_t from_float(float f) {
        uint32_t u;
        std::memcpy(&u, &f, 4);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u); // NaN: quiet, sign kept
        return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);                    // RNE; a carry into the exponent is the overflow to inf
    }
    static float to_float(uint16_t b) {
        const uint32_t u = (uint32_t)b << 16;
        float f;
        std::memcpy(&f, &u, 4);
        return f;
    }
};
static_assert(sizeof(bfloat16_t) == 2 && std::is_standard_layout<bfloat16_t>::value, "bfloat16_t is 16 bits of storage");
} // namespace cvgs
