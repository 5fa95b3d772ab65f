// cvgs_geometry.h -- the per-plane resize geometry, the box -> rectangle rule and the landmark -> warp fit, ONE spelling for the host side
// (cvgs_api.cpp: lowering; cvgs_detect.cpp: the table builders' and detector stages' host entries) and the device-side table builders (k_boxes.hip, k_points.hip).  Bit-exactness of fx / fy is part of the parity contract: both sides compile this text
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

// ---- landmarks -> inverse warp (cvgs_hip_ext.h: cvgs_warp_fit) -------------------------------------------------------------------------
// The K points of ONE item (`pts`: x0 y0 x1 y1 ..., frame pixels) and the template (`tmpl`: the same layout, destination pixels) become the
// nine floats of a WarpPlane::m, DESTINATION -> SOURCE.  Returns false, with the invalid entry in m, when the item is invalid.  Everything is
// computed in double in the order written here -- sums over the points in index order, no sqrt / sin / cos -- and narrowed to float at the
// end: host and device compile this text with -ffp-contract=off and divide correctly rounded, so they agree bit for bit
// (tests/test_gpu_warp_points.py).  `pts` is read in place (twice for the similarity fit), never copied into an array: on the device it
// points into global memory and the function needs no scratch.  Whatever `pts` holds, m only decides WHERE inside the host-validated frame
// a plane reads: the warp kernels test 0 <= sx < w && 0 <= sy < h before any tap, which NaN, +-inf and huge values all fail.
CVGS_HD inline bool fit_finite(double v) { return v - v == 0.0; } // false for NaN and +-inf
CVGS_HD inline void warp_fit_invalid(float* m) { // every destination pixel -> (-1, -1): outside any source
    m[0] = 0.f; m[1] = 0.f; m[2] = -1.f;
    m[3] = 0.f; m[4] = 0.f; m[5] = -1.f;
    m[6] = 0.f; m[7] = 0.f; m[8] = 1.f;
}
// `live`: the item's index lies below the (clamped) count.  The caller has validated fit, k and the template on the host.
CVGS_HD inline bool warp_fit(int fit, int k, const float* pts, const float* tmpl, bool live, float* m) {
    warp_fit_invalid(m);
    if (!live) return false;
    double m0, m1, m2, m3, m4, m5;
    if (fit == CVGS_WARP_FIT_AFFINE3) {
        // M (q_j, 1) = p_j: the linear part maps the template's edge vectors onto the points' (Cramer's rule), the translation fixes point 0
        const double p0x = (double)pts[0], p0y = (double)pts[1], p1x = (double)pts[2], p1y = (double)pts[3], p2x = (double)pts[4], p2y = (double)pts[5];
        if (!(fit_finite(p0x) && fit_finite(p0y) && fit_finite(p1x) && fit_finite(p1y) && fit_finite(p2x) && fit_finite(p2y))) return false;
        const double q0x = (double)tmpl[0], q0y = (double)tmpl[1];
        const double e1x = (double)tmpl[2] - q0x, e1y = (double)tmpl[3] - q0y, e2x = (double)tmpl[4] - q0x, e2y = (double)tmpl[5] - q0y;
        const double det = e1x * e2y - e1y * e2x; // != 0: checked on the host
        const double d1x = p1x - p0x, d1y = p1y - p0y, d2x = p2x - p0x, d2y = p2y - p0y;
        m0 = (d1x * e2y - d2x * e1y) / det;
        m1 = (d2x * e1x - d1x * e2x) / det;
        m3 = (d1y * e2y - d2y * e1y) / det;
        m4 = (d2y * e1x - d1y * e2x) / det;
        m2 = p0x - (m0 * q0x + m1 * q0y);
        m5 = p0y - (m3 * q0x + m4 * q0y);
    } else {
        // forward fit p -> q: q ~ [a -b; b a] p + t, least squares in closed form
        double px = 0.0, py = 0.0, qx = 0.0, qy = 0.0;
        bool finite = true;
        for (int i = 0; i < k; ++i) {
            const double x = (double)pts[2 * i], y = (double)pts[2 * i + 1];
            finite = finite && fit_finite(x) && fit_finite(y);
            px = px + x;
            py = py + y;
            qx = qx + (double)tmpl[2 * i];
            qy = qy + (double)tmpl[2 * i + 1];
        }
        if (!finite) return false;
        const double kd = (double)k;
        px = px / kd; py = py / kd; qx = qx / kd; qy = qy / kd;
        double den = 0.0, sa = 0.0, sb = 0.0;
        for (int i = 0; i < k; ++i) {
            const double pcx = (double)pts[2 * i] - px, pcy = (double)pts[2 * i + 1] - py;
            const double qcx = (double)tmpl[2 * i] - qx, qcy = (double)tmpl[2 * i + 1] - qy;
            den = den + (pcx * pcx + pcy * pcy);
            sa = sa + (pcx * qcx + pcy * qcy);
            sb = sb + (pcx * qcy - pcy * qcx);
        }
        if (den == 0.0 || !fit_finite(den)) return false;
        const double a = sa / den, b = sb / den;
        const double tx = qx - (a * px - b * py), ty = qy - (b * px + a * py);
        const double n = a * a + b * b;
        if (n == 0.0 || !fit_finite(n)) return false;
        // the inverse: p = (1/n) [a b; -b a] (q - t)
        const double ia = a / n, ib = b / n;
        m0 = ia;
        m1 = ib;
        m2 = -(ia * tx + ib * ty);
        m3 = -ib;
        m4 = ia;
        m5 = ib * tx - ia * ty;
    }
    const float f0 = (float)m0, f1 = (float)m1, f2 = (float)m2, f3 = (float)m3, f4 = (float)m4, f5 = (float)m5;
    if (!(fit_finite((double)f0) && fit_finite((double)f1) && fit_finite((double)f2) && fit_finite((double)f3) && fit_finite((double)f4) &&
          fit_finite((double)f5)))
        return false;
    m[0] = f0; m[1] = f1; m[2] = f2;
    m[3] = f3; m[4] = f4; m[5] = f5;
    return true;
}

// ---- a box -> the inverse warp of its context crop (cvgs_hip_ext.h: cvgs_warp_tables_from_boxes, THE CONTRACT) ---------------------------
// Steps 1-7 for ONE item: `box` = (xa, ya, xb, yb), edge coordinates, read in place; `scale` / `pad` = the descriptor's two floats each.
// m receives the nine floats of a WarpPlane::m, rect the four of boxes_out[i] (always written: zeros for an invalid item).  Returns
// whether the item is valid.  Double throughout, one rounding per operation in the order written, narrowed at the end: host and device
// compile this text with -ffp-contract=off and divide correctly rounded, so they agree bit for bit.
// `live`: the item's index lies below the (clamped) count.  The caller has validated shape, scale, pad and the target on the host.
CVGS_HD inline bool box_warp_fit(int shape, const float* box, const float* scale, const float* pad, int dst_w, int dst_h, bool live, float* m, float* rect) {
    warp_fit_invalid(m);
    rect[0] = 0.f; rect[1] = 0.f; rect[2] = 0.f; rect[3] = 0.f;
    if (!live) return false;
    const double xa = (double)box[0], ya = (double)box[1], xb = (double)box[2], yb = (double)box[3];
    if (!(fit_finite(xa) && fit_finite(ya) && fit_finite(xb) && fit_finite(yb))) return false;
    const double w = xb - xa, h = yb - ya;
    if (!(w > 0.0 && h > 0.0)) return false;
    const double cx = (xa + xb) * 0.5, cy = (ya + yb) * 0.5;
    double w1 = w * (double)scale[0];
    w1 = w1 + (double)pad[0];
    double h1 = h * (double)scale[1];
    h1 = h1 + (double)pad[1];
    const double dw = (double)dst_w, dh = (double)dst_h;
    if (shape == CVGS_BOX_SHAPE_EXPAND) { // the shorter side grows; no rounded ratio of the target's sides
        const double t1 = w1 * dh, t2 = h1 * dw;
        if (t1 > t2) h1 = t1 / dw;
        else if (t2 > t1) w1 = t2 / dh;
    }
    const double hw = w1 * 0.5, hh = h1 * 0.5;
    const double m0 = w1 / dw, m4 = h1 / dh;
    const double m2 = (cx - hw) + (m0 * 0.5 - 0.5), m5 = (cy - hh) + (m4 * 0.5 - 0.5);
    const float f0 = (float)m0, f2 = (float)m2, f4 = (float)m4, f5 = (float)m5;
    if (!(fit_finite((double)f0) && fit_finite((double)f2) && fit_finite((double)f4) && fit_finite((double)f5))) return false;
    m[0] = f0; m[2] = f2;
    m[4] = f4; m[5] = f5;
    rect[0] = (float)(cx - hw); rect[1] = (float)(cy - hh);
    rect[2] = (float)(cx + hw); rect[3] = (float)(cy + hh);
    return true;
}

// ---- detector candidates -> selected boxes (cvgs_hip_ext.h: cvgs_boxes_select, THE CONTRACT) ---------------------------------------------
// Steps 2-5 for ONE live candidate: `c` = its four coordinates as read, `xf` = (sx, sy, ox, oy).  Returns whether it is a member; then
// out[0..3] = (xa, ya, xb, yb) clamped into the frame.  Strict fp32, one rounding per operation in the order written (both sides compile
// this with -ffp-contract=off); the clamp is spelled with comparisons so that -0.0f and a NaN from inf - inf both give +0.0f on either side.
CVGS_HD inline float select_clamp(float v, float e) {
    v = v > 0.0f ? v : 0.0f;
    return v < e ? v : e;
}
CVGS_HD inline bool select_prepare(int fmt, float c0, float c1, float c2, float c3, float score, float score_thr, const float* xf, int w, int h, float* out) {
    if (score != score || !(score >= score_thr) || c0 != c0 || c1 != c1 || c2 != c2 || c3 != c3) return false;
    float xa = c0, ya = c1, xb = c2, yb = c3;
    if (fmt == CVGS_CAND_CXCYWH_F32) {
        const float hw = c2 * 0.5f, hh = c3 * 0.5f;
        xa = c0 - hw;
        xb = c0 + hw;
        ya = c1 - hh;
        yb = c1 + hh;
    }
    xa = xa * xf[0]; xa = xa + xf[2];
    xb = xb * xf[0]; xb = xb + xf[2];
    ya = ya * xf[1]; ya = ya + xf[3];
    yb = yb * xf[1]; yb = yb + xf[3];
    const float fw = (float)w, fh = (float)h;
    xa = select_clamp(xa, fw);
    xb = select_clamp(xb, fw);
    ya = select_clamp(ya, fh);
    yb = select_clamp(yb, fh);
    out[0] = xa; out[1] = ya; out[2] = xb; out[3] = yb;
    return xb > xa && yb > ya;
}
// Step 6: member j (score sj) comes before member i (score si).  A strict total order over members: no score is NaN.
CVGS_HD inline bool select_precedes(float sj, int j, float si, int i) { return sj > si || (sj == si && j < i); }
// Step 7: the kept box (jxa .. jyb) suppresses the box (ixa .. iyb).  Clamped boxes: every value lies in [0, extent], none is NaN or -0.
CVGS_HD inline bool select_suppresses(float jxa, float jya, float jxb, float jyb, float ixa, float iya, float ixb, float iyb, float iou_thr) {
    const float iw = fminf(ixb, jxb) - fmaxf(ixa, jxa);
    const float ih = fminf(iyb, jyb) - fmaxf(iya, jya);
    if (!(iw > 0.0f && ih > 0.0f)) return false;
    const float inter = iw * ih;
    const float area_i = (ixb - ixa) * (iyb - iya);
    const float area_j = (jxb - jxa) * (jyb - jya);
    const float uni = (area_i + area_j) - inter;
    return inter > iou_thr * uni;
}

// ---- a detector's raw head -> select's candidates (cvgs_hip_ext.h: cvgs_head_decode, THE CONTRACT) ------------------------------------------
// Step 1: every element widens to fp32 exactly.  bf16 is the top half of an fp32; fp16 is re-biased, its subnormals (m * 2^-24) normalised
// by the position of their leading bit.  Integer operations only, so host and device cannot differ; a NaN keeps its payload (none is stored).
CVGS_HD inline float head_bits_f32(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
CVGS_HD inline float head_widen_bf16(uint16_t h) { return head_bits_f32((uint32_t)h << 16); }
CVGS_HD inline float head_widen_f16(uint16_t h) {
    const uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 31u) return head_bits_f32(s | 0x7f800000u | (m << 13));
    if (e != 0u) return head_bits_f32(s | ((e + 112u) << 23) | (m << 13));
    if (m == 0u) return head_bits_f32(s);
    const uint32_t sh = (uint32_t)__builtin_clz(m) - 21u; // 1..10: the shift that brings the leading bit of m to bit 10
    return head_bits_f32(s | ((113u - sh) << 23) | (((m << sh) & 0x3ffu) << 13));
}
// Step 2, sequential form: class score v of class c, visited in ascending c from (best, cls) = (-inf, 0).  A NaN never wins (v > best is
// false), the first of equal scores stays (-0.0f == 0.0f), and best carries the winner's bits.
CVGS_HD inline void head_best_step(float v, int c, float* best, int* cls) {
    if (v > *best) {
        *best = v;
        *cls = c;
    }
}
// Step 2, combining form: (v, c) beats (b, cb).  Over partial results of the sequential form on disjoint class subsets (each visited in
// ascending c; an empty subset is the identity (-inf, 0)) the maximum under this relation is the sequential result over all classes: no
// partial result holds a NaN, and a partial (-inf, x) always has x == 0.
CVGS_HD inline bool head_best_wins(float v, int c, float b, int cb) { return v > b || (v == b && c < cb); }
// Step 3: one fp32 multiplication with an objectness value, none without.
CVGS_HD inline float head_score(float best, bool has_obj, float obj) { return has_obj ? obj * best : best; }
// Step 4.  A NaN score fails score >= thr.
CVGS_HD inline bool head_member(float score, float thr, float c0, float c1, float c2, float c3) {
    return score >= thr && !(c0 != c0 || c1 != c1 || c2 != c2 || c3 != c3);
}

// ---- landmarks of kept detections -> the points of cvgs_warp_tables_from_points (cvgs_hip_ext.h: cvgs_points_gather, THE CONTRACT) ----------
// The element of attribute `attr` of candidate `c`, in size_t: 65534 * (2^31 - 1) + 8191 * (2^31 - 1) needs 48 bits.
CVGS_HD inline size_t gather_elem_index(int32_t c, int32_t cand_stride, int32_t attr, int32_t attr_stride) {
    return (size_t)c * (size_t)cand_stride + (size_t)attr * (size_t)attr_stride;
}
// Step 1.
CVGS_HD inline int gather_live(const int32_t* kept_count, int max_out) {
    const int live = kept_count ? *kept_count : max_out;
    return live < 0 ? 0 : (live > max_out ? max_out : live);
}
// Step 2: the raw candidate of row j, or -1 for an invalid row.  An index is read only for j < live and only through an index that passed
// its own test.
CVGS_HD inline int32_t gather_source(const GatherFrame& f, int j, int live) {
    if (j >= live) return -1;
    const int32_t k = f.kept_index[j];
    if (k < 0 || k >= f.max_cand) return -1;
    if (!f.cand_index) return k;
    const int32_t c = f.cand_index[k];
    return c < 0 || c >= f.max_cand ? -1 : c;
}
template <int E>
CVGS_HD inline float gather_read(const void* head, size_t idx) {
    if (E == CVGS_HEAD_F32) return ((const float*)head)[idx];
    const uint16_t h = ((const uint16_t*)head)[idx];
    return E == CVGS_HEAD_F16 ? head_widen_f16(h) : head_widen_bf16(h);
}
// Step 3: detector -> frame pixels, two roundings; every NaN becomes the one quiet NaN.
static constexpr uint32_t kGatherNaN = 0x7fc00000u;
CVGS_HD inline float gather_map(float v, float s, float o) {
    v = v * s;
    v = v + o;
    return v != v ? head_bits_f32(kGatherNaN) : v;
}
// Steps 2-5 for point p of row j: what work-item j * n_points + p of k_points_gather does and what the host entry loops over.  `f`'s output
// pointers are the buffers written (the host entry puts its own there).
template <int E>
CVGS_HD inline void gather_point(const GatherFrame& f, int j, int p, int live) {
    const int32_t c = gather_source(f, j, live);
    float x = head_bits_f32(kGatherNaN), y = x, conf = 0.0f;
    if (c >= 0) {
        const int32_t a = f.point_attr + p * f.point_step;
        x = gather_map(gather_read<E>(f.head, gather_elem_index(c, f.cand_stride, a, f.attr_stride)), f.xf[0], f.xf[2]);
        y = gather_map(gather_read<E>(f.head, gather_elem_index(c, f.cand_stride, a + 1, f.attr_stride)), f.xf[1], f.xf[3]);
        if (f.conf_out) conf = gather_read<E>(f.head, gather_elem_index(c, f.cand_stride, a + f.conf_offset, f.attr_stride));
    }
    const size_t o = (size_t)j * (size_t)f.n_points + (size_t)p;
    f.points_out[2 * o] = x;
    f.points_out[2 * o + 1] = y;
    if (f.conf_out) f.conf_out[o] = conf;
    if (p == 0 && f.source_out) f.source_out[j] = c;
}

} // namespace cvgs
