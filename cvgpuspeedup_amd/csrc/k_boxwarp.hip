// k_boxwarp.hip -- device warp tables from a detector's device-side boxes (cvgs_warp_tables_from_boxes, include/cvgs_hip_ext.h).
// One launch = the tables of up to CVGS_WARP_MAX_FRAMES frames: grid y = frame, one work-item per item, the frames' descriptors in the
// kernel arguments (1.5 KB).  Each work-item reads its four floats straight from global memory (no LDS, no atomic, no scratch) and writes
// one 64-byte WarpPlane: the host-validated frame, the matrix of cvgs_geometry.h's box_warp_fit -- the text the host entry runs, compiled
// with the same flags -- and the destination size; then the shaped rectangle and the validity flag where they are asked for.  Every store
// is a plain per-lane store into table[i] / boxes_out[i] / valid[i], i < max_items; the one load lies inside boxes[max_items][4].
#include <hip/hip_runtime.h>

#include "cvgs_geometry.h"

namespace cvgs {

struct BoxWarpArgs {
    BoxWarpFrame f[CVGS_WARP_MAX_FRAMES];
};

__global__ __launch_bounds__(64) void k_box_warps(const BoxWarpArgs a) {
    const BoxWarpFrame& f = a.f[blockIdx.y];
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i >= f.max_items) return; // (frames of one launch may hold different numbers of items)
    const int live = gather_live(f.count, f.max_items);

    WarpPlane P;
    P.data = f.data;
    P.w = f.w;
    P.h = f.h;
    P.step = f.step;
    P.dw = f.dst_w;
    P.dh = f.dst_h;
    float rect[4];
    const bool ok = box_warp_fit(f.shape, f.boxes + (size_t)i * 4, f.scale, f.pad, f.dst_w, f.dst_h, i < live, P.m, rect);
    f.table[i] = P;
    if (f.boxes_out) {
        float* o = f.boxes_out + (size_t)i * 4;
        o[0] = rect[0]; o[1] = rect[1]; o[2] = rect[2]; o[3] = rect[3];
    }
    if (f.valid) f.valid[i] = ok ? 1 : 0;
}

int launch_box_warps(const BoxWarpFrame* frames, int n, void* stream) {
    if (n < 1 || n > CVGS_WARP_MAX_FRAMES) return (int)hipErrorInvalidValue;
    BoxWarpArgs a;
    int most = 1;
    for (int i = 0; i < CVGS_WARP_MAX_FRAMES; ++i) {
        a.f[i] = i < n ? frames[i] : BoxWarpFrame{};
        if (i < n && frames[i].max_items > most) most = frames[i].max_items;
    }
    hipLaunchKernelGGL(k_box_warps, dim3((unsigned)((most + 63) / 64), (unsigned)n, 1), dim3(64, 1, 1), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

} // namespace cvgs
