// k_area_axis.hpp -- one axis of an INTER_AREA output pixel, shared by the AREA kernels of pixel sources (k_area.hip) and of 4:2:0 decoder
// surfaces (k_yuv_area.hip).  The arithmetic is the contract written down in include/cvgs_hip.h (strict fp32, every operation rounded
// once, in the written order): every kernel runs THIS text for it, so the kernels of one read kind are bit-identical to each other.
#pragma once

#include "k_common.hpp"

namespace cvgs {

// One axis of one output pixel: the taps are source indices i0 .. i0 + cnt - 1 (clamped to n - 1), tap j weighs area_w(A, j), W is their sum.
struct AreaAxis {
    float a, b; // shrinking: the footprint [a, b) in source pixels; not shrinking: a = the bilinear source position, b unused
    float W;
    int i0, cnt;
    bool shrink;
};

__device__ __forceinline__ float area_w(const AreaAxis& A, int j) {
    if (A.shrink) {
        if (A.b <= A.a) return 1.0f; // (a footprint that rounding emptied: the single tap i0)
        const int i = A.i0 + j;
        return fminf((float)(i + 1), A.b) - fmaxf((float)i, A.a);
    }
    return j == 0 ? (float)(A.i0 + 1) - A.a : A.a - (float)A.i0; // the bilinear pair
}

// t = output coordinate inside the window, f = source step per output pixel, n = source extent
__device__ __forceinline__ AreaAxis area_axis(int t, float f, int n) {
    AreaAxis A;
    A.shrink = f > 1.0f;
    A.a = (float)t * f;
    if (A.shrink) {
        A.b = fminf((float)(t + 1) * f, (float)n);
        A.i0 = min((int)floorf(A.a), n - 1);
        const int i1 = max(min((int)ceilf(A.b), n), A.i0 + 1);
        A.cnt = i1 - A.i0;
        float W = 0.0f;
        for (int j = 0; j < A.cnt; ++j) W = W + area_w(A, j);
        A.W = W;
    } else {
        A.b = 0.0f;
        A.i0 = (int)floorf(A.a);
        A.cnt = 2;
        A.W = 1.0f; // by definition, not summed
    }
    return A;
}

// The chroma twin of a luma axis L over n luma samples, on the grid of nc = (n + 1) >> 1 half-resolution chroma samples (4:2:0, and the
// horizontal axis of it): tap j weighs area_w(C, j) and reads chroma sample area_chroma_index(C, j, n).
//   shrinking: the same box seen from the chroma grid, [a / 2, b / 2) -- a chroma sample weighs half the luma area it sits under;
//   not shrinking: the two luma taps with their luma weights, each on the chroma sample of its luma sample (both kept, in this order,
//     also when they name one sample); W = 1.0f.
__device__ __forceinline__ AreaAxis area_chroma_axis(const AreaAxis& L, int n) {
    if (!L.shrink) return L;
    const int nc = (n + 1) >> 1;
    AreaAxis C;
    C.shrink = true;
    C.a = L.a * 0.5f;
    C.b = L.b * 0.5f;
    C.i0 = min((int)floorf(C.a), nc - 1);
    const int c1 = max(min((int)ceilf(C.b), nc), C.i0 + 1);
    C.cnt = c1 - C.i0;
    float W = 0.0f;
    for (int j = 0; j < C.cnt; ++j) W = W + area_w(C, j);
    C.W = W;
    return C;
}

__device__ __forceinline__ int area_chroma_index(const AreaAxis& C, int j, int n) {
    return C.shrink ? C.i0 + j : (min(C.i0 + j, n - 1) >> 1);
}

} // namespace cvgs
