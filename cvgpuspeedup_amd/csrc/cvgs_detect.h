// cvgs_detect.h -- what the host files of the detector-side entry points share (cvgs_detect.cpp, cvgs_boxwarp.cpp): the collector of a
// call's output ranges, the one shape of a device stage, the live count of a host twin and the whole-frame checks of the table builders.
// Host only: no HIP header and no HIP call.
#pragma once

#include "cvgs_geometry.h"
#include "cvgs_host.h"

namespace cvgs {

// The bytes one call writes, as [lo, hi) ranges: a stage states its outputs as a list of add() calls (a null pointer: an optional output
// that is not asked for).  A range beyond the capacity is not stored, and the call is then refused like an overlapping one.
struct OutRanges {
    static constexpr int kCapacity = 6 * 16; // the stage with the most: head_decode, 6 outputs x 16 frames
    ByteRange r[kCapacity];
    int n = 0;
    bool full = false;
    void add(const void* p, size_t bytes) {
        if (p && n < kCapacity) r[n++] = ByteRange{(const uint8_t*)p, (const uint8_t*)p + bytes};
        else if (p) full = true;
    }
    bool overlaps() const {
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < i; ++j)
                if (r[i].lo < r[j].hi && r[j].lo < r[i].hi) return true;
        return full;
    }
};

// One call of a device stage: up to MaxFrames descriptors, each checked into its frame and its outputs collected (the first defect of the first
// bad descriptor is the answer), the outputs against each other, one launch.  text: null descriptors, range of n, overlap (null: no such test), launch.
template <int MaxFrames, int Outs, typename Desc, typename Frame>
int run_stage(const char* const (&text)[4], const Desc* descs, int32_t n, void* stream, int (*check)(const Desc&, OutRanges*, Frame&),
              int (*launch)(const Frame*, int, void*)) {
    static_assert(MaxFrames * Outs <= OutRanges::kCapacity || Outs == 0, "the collector holds every output of a full call");
    if (!descs) return fail(CVGS_ERR_INVALID, text[0]);
    if (n < 1 || n > MaxFrames) return fail(CVGS_ERR_INVALID, text[1]);
    Frame frames[MaxFrames];
    OutRanges outs;
    for (int i = 0; i < n; ++i)
        if (const int rc = check(descs[i], &outs, frames[i])) return rc;
    if (text[2] && outs.overlaps()) return fail(CVGS_ERR_INVALID, text[2]);
    const int e = launch(frames, n, stream);
    return e ? hip_fail(e, text[3]) : CVGS_OK;
}

// What a host twin works on: *count, or `max` without one, clamped into [0, max] (cvgs_geometry.h: one text with k_gather.hip)
inline int live_count(const int32_t* count, int max) { return gather_live(count, max); }

// A whole frame as the source of a table builder, as lower() checks a host-described plane; in two parts: warp tables refuse CV_64F between them
inline int check_frame_type(int src_type, int* esz) {
    *esz = depth_bytes(type_depth(src_type)) * CVGS_TYPE_CN(src_type);
    return CVGS_TYPE_CN(src_type) > 4 || *esz < 1 ? fail(CVGS_ERR_INVALID, "bad source type") : CVGS_OK;
}
inline int check_frame_plane(const cvgs_image2d& im, int esz) {
    if (!im.data || im.width < 1 || im.height < 1) return fail(CVGS_ERR_INVALID, "empty source plane");
    if (im.width > kMaxDim || im.height > kMaxDim) return fail(CVGS_ERR_UNSUPPORTED, "source plane wider or taller than 2^24 pixels");
    if ((int64_t)im.step < (int64_t)im.width * esz) return fail(CVGS_ERR_INVALID, "source step smaller than a row");
    return CVGS_OK;
}

} // namespace cvgs
