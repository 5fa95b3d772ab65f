// k_points.hip -- device warp tables from a detector's device-side landmarks (cvgs_warp_tables_from_points, include/cvgs_hip_ext.h).
// One launch = the tables of up to CVGS_WARP_MAX_FRAMES frames: grid y = frame, one work-item per item, the frames' descriptors and
// templates in the kernel arguments (3.2 KB).  Each work-item reads its K points straight from global memory inside the fit's loops (no
// per-lane array, no LDS) and writes one 64-byte WarpPlane: the host-validated frame, the fit of cvgs_geometry.h -- the text the host
// builder runs, compiled with the same flags -- and the destination size.  Every store is a plain per-lane store into table[i] / valid[i],
// i < max_items; every load of a point lies inside points[max_items][n_points][2].
#include <hip/hip_runtime.h>

#include "cvgs_geometry.h"

namespace cvgs {

struct PointArgs {
    PointFrame f[CVGS_WARP_MAX_FRAMES];
};

__global__ __launch_bounds__(64) void k_points(const PointArgs a) {
    const PointFrame& f = a.f[blockIdx.y];
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i >= f.max_items) return; // (frames of one launch may hold different numbers of items)
    int live = f.count ? *f.count : f.max_items;
    live = live < 0 ? 0 : (live > f.max_items ? f.max_items : live);

    WarpPlane P;
    P.data = f.data;
    P.w = f.w;
    P.h = f.h;
    P.step = f.step;
    P.dw = f.dst_w;
    P.dh = f.dst_h;
    const bool ok = warp_fit(f.fit, f.n_points, f.points + (size_t)i * (size_t)f.n_points * 2, f.tmpl, i < live, P.m);
    f.table[i] = P;
    if (f.valid) f.valid[i] = ok ? 1 : 0;
}

int launch_points(const PointFrame* frames, int n, void* stream) {
    if (n < 1 || n > CVGS_WARP_MAX_FRAMES) return (int)hipErrorInvalidValue;
    PointArgs a;
    int most = 1;
    for (int i = 0; i < CVGS_WARP_MAX_FRAMES; ++i) {
        a.f[i] = i < n ? frames[i] : PointFrame{};
        if (i < n && frames[i].max_items > most) most = frames[i].max_items;
    }
    hipLaunchKernelGGL(k_points, dim3((unsigned)((most + 63) / 64), (unsigned)n, 1), dim3(64, 1, 1), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

} // namespace cvgs
