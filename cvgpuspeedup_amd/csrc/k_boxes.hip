// k_boxes.hip -- device plane tables from a detector's device-side boxes (cvgs_plane_tables_from_boxes, include/cvgs_hip_ext.h).
// One launch = the tables of up to CVGS_MAX_CHAINS frames: grid y = frame, one work-item per box, the frames' descriptors in the
// kernel arguments.  Each work-item reads 16 bytes of box (and the frame's count), clamps the box into the frame and writes one 48-byte
// PlaneParams -- the bytes cvgs_plane_table_build writes on the host for the same view: the geometry is the host's own text
// (cvgs_geometry.h), compiled with the same flags.  Every store is a plain per-lane store into table[i] / rects[i], i < max_boxes.
#include <hip/hip_runtime.h>

#include "cvgs_geometry.h"

namespace cvgs {

template <int N>
struct BoxArgs {
    BoxFrame f[N];
};

template <int N>
__global__ __launch_bounds__(64) void k_boxes(const BoxArgs<N> a) {
    const BoxFrame& f = a.f[blockIdx.y];
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i >= f.max_boxes) return; // (frames of one launch may hold different numbers of boxes)
    int live = f.count ? *f.count : f.max_boxes;
    live = live < 0 ? 0 : (live > f.max_boxes ? f.max_boxes : live);

    int l = 0, r = 0, t = 0, b = 0;
    bool ok = i < live;
    if (f.fmt == CVGS_BOX_XYXY_F32) {
        const float* q = (const float*)f.boxes + (size_t)i * 4;
        const float xa = q[0], ya = q[1], xb = q[2], yb = q[3];
        ok = ok && !(xa != xa || ya != ya || xb != xb || yb != yb);
        if (ok) {
            box_axis_f32(xa, xb, f.w, &l, &r);
            box_axis_f32(ya, yb, f.h, &t, &b);
        }
    } else {
        const int32_t* q = (const int32_t*)f.boxes + (size_t)i * 4;
        const int32_t x = q[0], y = q[1], w = q[2], h = q[3];
        ok = ok && w > 0 && h > 0;
        if (ok) {
            box_axis_i32(x, w, f.w, &l, &r);
            box_axis_i32(y, h, f.h, &t, &b);
        }
    }
    if (ok && f.yuv420) {
        box_axis_snap_even(f.w, &l, &r);
        box_axis_snap_even(f.h, &t, &b);
    }
    ok = ok && r > l && b > t;

    PlaneParams P;
    P.step = f.step;
    if (ok) { // 0 <= l < r <= w, 0 <= t < b <= h: a view inside the frame
        P.data = f.data + (size_t)t * (size_t)f.step + (size_t)l * (size_t)f.esz;
        P.w = r - l;
        P.h = b - t;
        // 4:2:0: chroma of the view's luma row 0 = frame chroma + (t/2)*step + l, seen from the view's data (t is even)
        P.uv_off = f.yuv420 ? (int32_t)((int64_t)f.uv_off - (int64_t)(t / 2) * (int64_t)f.step) : 0;
        plane_geometry(P.w, P.h, f.dst_w, f.dst_h, f.ar, P);
    } else { // the whole frame behind an empty destination window: background in every pixel
        P.data = f.data;
        P.w = f.w;
        P.h = f.h;
        P.uv_off = f.uv_off;
        P.fx = P.fy = 1.f;
        P.x1 = P.y1 = 0;
        P.x2 = P.y2 = -1;
    }
    f.table[i] = P;
    if (f.rects) {
        int32_t* o = f.rects + (size_t)i * 4;
        o[0] = ok ? l : 0;
        o[1] = ok ? t : 0;
        o[2] = ok ? r - l : 0;
        o[3] = ok ? b - t : 0;
    }
}

template <int N>
static hipError_t launch_boxes_t(const BoxFrame* frames, int n, hipStream_t s) {
    BoxArgs<N> a;
    int most = 1;
    for (int i = 0; i < N; ++i) {
        a.f[i] = i < n ? frames[i] : BoxFrame{};
        if (i < n && frames[i].max_boxes > most) most = frames[i].max_boxes;
    }
    hipLaunchKernelGGL(k_boxes<N>, dim3((unsigned)((most + 63) / 64), (unsigned)n, 1), dim3(64, 1, 1), 0, s, a);
    return hipGetLastError();
}

int launch_boxes(const BoxFrame* frames, int n, void* stream) {
    if (n < 1 || n > CVGS_MAX_CHAINS) return (int)hipErrorInvalidValue;
    const hipStream_t s = (hipStream_t)stream;
    return (int)(n <= kBoxFramesSmall ? launch_boxes_t<kBoxFramesSmall>(frames, n, s) : launch_boxes_t<CVGS_MAX_CHAINS>(frames, n, s));
}

} // namespace cvgs
