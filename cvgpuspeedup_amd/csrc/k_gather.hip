// k_gather.hip -- the landmarks of the detections cvgs_boxes_select kept -> the points cvgs_warp_tables_from_points reads
// (cvgs_points_gather, include/cvgs_hip_ext.h: THE CONTRACT).  ONE launch per call, up to CVGS_GATHER_MAX_FRAMES frames, the frames'
// descriptors in the kernel arguments (1.75 KB).  Grid (ceil(max over frames of max_out * n_points / 256), frame), 256 work-items.
//   k_points_gather   work-item t of a frame owns (row j, point p) = (t / n_points, t % n_points): it finds the row's raw candidate
//                     (kept_index, optionally through cand_index, every index tested before it is used -- cvgs_geometry.h: gather_source),
//                     reads the point's x, y (and confidence) from the head in place, maps them to frame pixels and stores them at
//                     points_out[2 t], [2 t + 1] (conf_out[t]); the lane with p == 0 stores source_out[j].  Consecutive lanes store
//                     consecutive (x, y) pairs, so a wave's store is one contiguous span of 512 bytes.  The loads are a gather by nature:
//                     an [A, N] head gives one element per candidate and attribute, an [N, A] head a short run per candidate.
// The body is the host entry's own text (gather_point<E>), instantiated per element type and chosen on a workgroup-uniform switch, since
// the frames of one call may hold different types.  No LDS, no atomic, no scratch.  A frame with fewer items than the grid covers exits
// on a workgroup-uniform test.  The work is a few thousand elements per call: the launch boundary is the cost, and nothing here is tuned
// beyond the coalesced stores.
// Every load of the head has a candidate index in [0, max_cand) and an attribute the host validated; every load of kept_index has
// j < live <= max_out, every load of cand_index an index in [0, max_cand); every store has t < max_out * n_points (j < max_out).
#include <hip/hip_runtime.h>

#include "cvgs_geometry.h"

namespace cvgs {

struct GatherArgs {
    GatherFrame f[CVGS_GATHER_MAX_FRAMES];
};

__global__ __launch_bounds__(kGatherTile) void k_points_gather(const GatherArgs a) {
    const GatherFrame& f = a.f[blockIdx.y];
    const int items = f.max_out * f.n_points; // <= 65535 * 64
    const int first = (int)blockIdx.x * kGatherTile;
    if (first >= items) return; // (frames of one call may hold different numbers of items)
    const int t = first + (int)threadIdx.x;
    if (t >= items) return;
    const int live = gather_live(f.kept_count, f.max_out);
    const int j = t / f.n_points, p = t - j * f.n_points;
    switch (f.elem) { // workgroup-uniform
    case CVGS_HEAD_F32: gather_point<CVGS_HEAD_F32>(f, j, p, live); break;
    case CVGS_HEAD_F16: gather_point<CVGS_HEAD_F16>(f, j, p, live); break;
    default: gather_point<CVGS_HEAD_BF16>(f, j, p, live); break;
    }
}

int launch_gather(const GatherFrame* frames, int n, void* stream) {
    if (n < 1 || n > CVGS_GATHER_MAX_FRAMES) return (int)hipErrorInvalidValue;
    GatherArgs a;
    int most = 1;
    for (int i = 0; i < CVGS_GATHER_MAX_FRAMES; ++i) {
        a.f[i] = i < n ? frames[i] : GatherFrame{};
        if (i < n && frames[i].max_out * frames[i].n_points > most) most = frames[i].max_out * frames[i].n_points;
    }
    const dim3 grid((unsigned)((most + kGatherTile - 1) / kGatherTile), (unsigned)n, 1);
    hipLaunchKernelGGL(k_points_gather, grid, dim3(kGatherTile, 1, 1), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

} // namespace cvgs
