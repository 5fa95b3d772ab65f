// cvgs_host.h -- what the two host files of the C-ABI share: cvgs_api.cpp (chains: lowering, dispatch, ticks, CircularTensor, the queue) and
// cvgs_detect.cpp / cvgs_boxwarp.cpp (the detector-side stages and their table builders).  Host only: no kernel includes this, and it needs no HIP header.
#pragma once

#include <stdint.h>

#include <string>

#include "cvgs_device.h"

namespace cvgs {

// The one way an entry point fails: the text cvgs_last_error() returns, and the code to return.  Defined in cvgs_api.cpp, beside the
// thread's error text and tick note.  hip_fail appends HIP's own text for `hip_error` (a hipError_t) to `what`.
int fail(int code, const std::string& msg);
int hip_fail(int hip_error, const char* what);

inline int depth_bytes(int depth) {
    switch (depth) {
    case CVGS_DEPTH_8U: case CVGS_DEPTH_8S: return 1;
    case CVGS_DEPTH_16U: case CVGS_DEPTH_16S: case CVGS_DEPTH_16F: case kDepthBF16: return 2;
    case CVGS_DEPTH_32S: case CVGS_DEPTH_32F: return 4;
    case CVGS_DEPTH_64F: return 8;
    }
    return 0;
}
// The depth of a public element type as ChainArgs carries it: CV_16BF (depth 16F with CVGS_TYPE_FLAG_BF16) becomes kDepthBF16.
// The flag means nothing beside another depth (today's handling of the bits above the channel field: ignored).
inline int type_depth(int type) {
    return CVGS_TYPE_DEPTH(type) == CVGS_DEPTH_16F && CVGS_TYPE_IS_BF16(type) ? kDepthBF16 : CVGS_TYPE_DEPTH(type);
}
inline bool is_resize(int kind) { return kind == CVGS_READ_RESIZE_LINEAR || kind == CVGS_READ_NV12_RESIZE_LINEAR; }
constexpr int kMaxDim = CVGS_MAX_DIM; // widest / tallest plane the 32-bit index arithmetic of the kernels is specified for
inline bool is_nv12(int kind) { return kind == CVGS_READ_NV12 || kind == CVGS_READ_NV12_RESIZE_LINEAR || kind == CVGS_READ_NV12_RESIZE_AREA; }
inline bool is_warp(int kind) { return kind == CVGS_READ_WARP_AFFINE || kind == CVGS_READ_WARP_PERSPECTIVE; }
// INTER_AREA: the bilinear resize's fields, geometry and plane table, kernels of its own (k_area.hip).  NOT in is_resize(): every site that
// asks is_resize() means "a bilinear kernel may serve this"; the sites that mean "planes carry plane_geometry" ask has_geometry().
inline bool is_area(int kind) { return kind == CVGS_READ_RESIZE_AREA; }
// INTER_AREA of 4:2:0 decoder surfaces: the bilinear NV12 resize's fields, geometry and plane table, kernels of its own (k_yuv_area.hip).
// In is_nv12() (a decoder surface is validated and addressed as one), NOT in is_resize() and NOT in is_area() (whose sites speak of pixels).
inline bool is_yuv_area(int kind) { return kind == CVGS_READ_NV12_RESIZE_AREA; }
inline bool any_area(int kind) { return is_area(kind) || is_yuv_area(kind); }
inline bool has_geometry(int kind) { return is_resize(kind) || any_area(kind); }
// [lo, hi): the bytes a chain reads or writes (cvgs_api.cpp: independence of a tick's chains), the bytes one output of a stage covers
// (cvgs_detect.cpp: the outputs of one call must not overlap)
struct ByteRange { const uint8_t* lo; const uint8_t* hi; };

} // namespace cvgs
