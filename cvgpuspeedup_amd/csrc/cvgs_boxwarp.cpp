// cvgs_boxwarp.cpp -- device warp tables from a detector's device-side boxes (include/cvgs_hip_ext.h: cvgs_warp_tables_from_boxes) and the
// host twin the kernel is held to.  Host logic only, as cvgs_detect.cpp: no HIP header and no HIP call -- a stream is a void*, the
// launcher's answer an int.  Everything is validated here, on the host, before the launcher makes the first HIP call; the accepted path
// allocates nothing, takes no lock and reads no environment.
#include <cstring>

#include "cvgs_detect.h"

using namespace cvgs;

namespace {
// The shaping and the matrix (cvgs_geometry.h: box_warp_fit) are one text for the kernel (k_boxwarp.hip) and for cvgs_warp_table_from_boxes_host.
// `outs` null: cvgs_warp_table_from_boxes_host -- the descriptor's output pointers are not used
int check_box_warp_desc(const cvgs_box_warp_desc& d, OutRanges* outs, BoxWarpFrame& f) {
    if (d.struct_size != sizeof(cvgs_box_warp_desc)) return fail(CVGS_ERR_INVALID, "cvgs_box_warp_desc size mismatch (ABI)");
    if (d.flags) return fail(CVGS_ERR_INVALID, "warp_tables_from_boxes: flags must be 0");
    if (d.read_kind < CVGS_READ_PIXEL || d.read_kind > CVGS_READ_WARP_PERSPECTIVE) return fail(CVGS_ERR_INVALID, "bad read kind");
    if (!is_warp(d.read_kind)) return fail(CVGS_ERR_UNSUPPORTED, "warp_tables_from_boxes: warp tables serve the warp reads (WARP_AFFINE / WARP_PERSPECTIVE) only");
    if (d.max_items < 1 || d.max_items > 65535) return fail(CVGS_ERR_INVALID, "max_items must be in [1, 65535]");
    if (d.shape != CVGS_BOX_SHAPE_STRETCH && d.shape != CVGS_BOX_SHAPE_EXPAND) return fail(CVGS_ERR_INVALID, "warp_tables_from_boxes: bad box shape");
    if (!fit_finite((double)d.scale[0]) || !fit_finite((double)d.scale[1]) || !(d.scale[0] > 0.0f) || !(d.scale[1] > 0.0f))
        return fail(CVGS_ERR_INVALID, "warp_tables_from_boxes: scale (x, y) must be finite and positive");
    if (!fit_finite((double)d.pad[0]) || !fit_finite((double)d.pad[1]) || !(d.pad[0] >= 0.0f) || !(d.pad[1] >= 0.0f))
        return fail(CVGS_ERR_INVALID, "warp_tables_from_boxes: pad (x, y) must be finite and not negative");
    if (!d.boxes) return fail(CVGS_ERR_INVALID, "warp_tables_from_boxes: boxes is null");
    if (outs && !d.table_out) return fail(CVGS_ERR_INVALID, "warp_tables_from_boxes: table_out is null");
    if ((outs && (((uintptr_t)d.table_out & 7) || (((uintptr_t)d.boxes_out | (uintptr_t)d.valid_out) & 3))) || (((uintptr_t)d.boxes | (uintptr_t)d.count) & 3))
        return fail(CVGS_ERR_INVALID, "warp_tables_from_boxes: table_out needs 8-byte, boxes / count / boxes_out / valid_out 4-byte alignment");
    if (d.dst_width < 1 || d.dst_height < 1) return fail(CVGS_ERR_INVALID, "warp target must be positive");
    if (d.dst_width > kMaxDim || d.dst_height > kMaxDim) return fail(CVGS_ERR_UNSUPPORTED, "warp target wider or taller than 2^24 pixels");
    const cvgs_image2d& im = d.frame;
    int esz, rc;
    if ((rc = check_frame_type(d.src_type, &esz))) return rc;
    if (type_depth(d.src_type) == CVGS_DEPTH_64F) return fail(CVGS_ERR_UNSUPPORTED, "device warp tables: CV_64F sources take host descriptors");
    if ((rc = check_frame_plane(im, esz))) return rc;
    if (im.uv_offset) return fail(CVGS_ERR_INVALID, "warp_tables_from_boxes: uv_offset belongs to the NV12 kinds");
    f = BoxWarpFrame{};
    f.data = (const uint8_t*)im.data;
    f.boxes = d.boxes; f.count = d.count;
    f.w = im.width; f.h = im.height; f.step = im.step;
    f.dst_w = d.dst_width; f.dst_h = d.dst_height;
    f.shape = d.shape; f.max_items = d.max_items;
    f.scale[0] = d.scale[0]; f.scale[1] = d.scale[1]; f.pad[0] = d.pad[0]; f.pad[1] = d.pad[1];
    if (!outs) return CVGS_OK;
    f.table = (WarpPlane*)d.table_out; f.boxes_out = d.boxes_out; f.valid = d.valid_out;
    outs->add(f.table, (size_t)f.max_items * sizeof(WarpPlane));
    outs->add(f.boxes_out, (size_t)f.max_items * 4 * sizeof(float));
    outs->add(f.valid, (size_t)f.max_items * sizeof(int32_t));
    return CVGS_OK;
}
} // namespace

extern "C" {
int cvgs_warp_tables_from_boxes(const cvgs_box_warp_desc* descs, int32_t n, cvgs_stream_t stream) {
    static const char* const text[4] = {"warp_tables_from_boxes: null descriptors", "warp_tables_from_boxes: n must be in [1, 16]", "warp_tables_from_boxes: the output buffers of one call overlap", "warp_tables_from_boxes: kernel launch"};
    return run_stage<CVGS_WARP_MAX_FRAMES, 3>(text, descs, n, stream, check_box_warp_desc, launch_box_warps);
}

int cvgs_warp_table_from_boxes_host(const cvgs_box_warp_desc* desc, void* table_out_host, float* boxes_out_host, int32_t* valid_out_host) {
    if (!desc || !table_out_host) return fail(CVGS_ERR_INVALID, "warp_table_from_boxes_host: null argument");
    BoxWarpFrame f;
    if (const int rc = check_box_warp_desc(*desc, nullptr, f)) return rc;
    const int live = live_count(f.count, f.max_items);
    for (int i = 0; i < f.max_items; ++i) { // k_box_warps' body
        WarpPlane P;
        std::memset(&P, 0, sizeof(P));
        P.data = f.data; P.w = f.w; P.h = f.h; P.step = f.step;
        P.dw = f.dst_w; P.dh = f.dst_h;
        float rect[4];
        const bool ok = box_warp_fit(f.shape, f.boxes + (size_t)i * 4, f.scale, f.pad, f.dst_w, f.dst_h, i < live, P.m, rect);
        std::memcpy((uint8_t*)table_out_host + (size_t)i * sizeof(WarpPlane), &P, sizeof(P));
        if (boxes_out_host) std::memcpy(boxes_out_host + (size_t)i * 4, rect, sizeof(rect));
        if (valid_out_host) valid_out_host[i] = ok ? 1 : 0;
    }
    return CVGS_OK;
}
} // extern "C"
