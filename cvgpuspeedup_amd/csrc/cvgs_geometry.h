// cvgs_geometry.h -- the per-plane resize geometry and the box -> rectangle rule, ONE spelling for the host-side lowering (cvgs_api.cpp)
// and the device-side table builder (k_boxes.hip).  Bit-exactness of fx / fy is part of the parity contract: both sides compile this text
// with -ffp-contract=off, gfx950 divides fp32 and fp64 correctly rounded (HIP's default), and roundf is exact on both -- so a table
// written on the device equals the host-built one byte for byte (tests/test_gpu_boxes.py compares them).
#pragma once

#include <math.h>
#include <stdint.h>

#include "cvgs_device.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define CVGS_HD __host__ __device__
#else
#define CVGS_HD
#endif

namespace cvgs {

// Host half of fk::Resize::build: the kernel-side scale factors and the aspect-ratio window.
// IGNORE_AR follows cv::cuda::resize's host code (scale = float(1.0 / (double(dst)/src))).
// PRESERVE_AR* fits the source inside the target keeping its aspect ratio (scale by height, fall
// back to width), centred (or left-aligned), extent rounded to nearest (RN_EVEN: down to even).
CVGS_HD inline void plane_geometry(int sw, int sh, int dw, int dh, int ar, PlaneParams& P) {
    int tw = dw, th = dh, x0 = 0, y0 = 0;
    if (ar != CVGS_IGNORE_AR) {
        float s = (float)dh / (float)sh;
        tw = (int)roundf(s * (float)sw); // half away from zero (std::round)
        if (ar == CVGS_PRESERVE_AR_RN_EVEN) tw -= tw % 2;
        if (tw > dw) {
            s = (float)dw / (float)sw;
            tw = dw;
            th = (int)roundf(s * (float)sh);
            if (ar == CVGS_PRESERVE_AR_RN_EVEN) th -= th % 2;
        }
        tw = tw < 1 ? 1 : tw;
        th = th < 1 ? 1 : th;
        x0 = ar == CVGS_PRESERVE_AR_LEFT ? 0 : (dw - tw) / 2;
        y0 = (dh - th) / 2;
    }
    P.fx = (float)(1.0 / ((double)tw / (double)sw));
    P.fy = (float)(1.0 / ((double)th / (double)sh));
    P.x1 = x0;
    P.y1 = y0;
    P.x2 = x0 + tw - 1;
    P.y2 = y0 + th - 1;
}

// One axis of a detector box clamped into [0, extent] (cvgs_hip_ext.h: cvgs_box_format).  *lo / *hi: the first pixel and one past the last.
// XYXY_F32: edges in pixel coordinates, `b` exclusive; the clamp comes first, so +-inf and values beyond the int range never reach the
// conversion (extent <= 2^24 is exact in fp32).  The caller has refused NaN.
CVGS_HD inline void box_axis_f32(float a, float b, int extent, int* lo, int* hi) {
    const float e = (float)extent;
    *lo = (int)floorf(fminf(fmaxf(a, 0.f), e));
    *hi = (int)ceilf(fminf(fmaxf(b, 0.f), e));
}
// XYWH_I32: origin and size; origin + size is formed in 64 bits.  The caller has refused size <= 0.
CVGS_HD inline void box_axis_i32(int32_t o, int32_t n, int extent, int* lo, int* hi) {
    const int64_t end = (int64_t)o + (int64_t)n;
    *lo = o < 0 ? 0 : (o > extent ? extent : o);
    *hi = end < 0 ? 0 : (end > (int64_t)extent ? extent : (int)end);
}
// 4:2:0 surfaces: the origin down to even, the end up to even and back into the (even) extent.
CVGS_HD inline void box_axis_snap_even(int extent, int* lo, int* hi) {
    *lo &= ~1;
    *hi = (*hi + 1) & ~1;
    if (*hi > extent) *hi = extent;
}

} // namespace cvgs
