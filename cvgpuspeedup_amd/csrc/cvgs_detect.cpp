// cvgs_detect.cpp -- the detector-side entry points of the C-ABI (include/cvgs_hip_ext.h): device plane tables from boxes, device warp
// tables from landmarks, box selection, head decoding, landmark gathering, and the host twins the kernels are held to.  (Warp tables from
// boxes: cvgs_boxwarp.cpp, over the same stage helpers, cvgs_detect.h.)
// Host logic only: no HIP header and no HIP call -- a stream is a void*, a launcher's answer an int, and failures go through cvgs_host.h.
// Every entry point validates everything here, on the host, before its launcher makes the first HIP call.  On the accepted path a device
// entry point allocates nothing; it takes no lock and reads no environment.
#include <algorithm>
#include <cstring>
#include <vector>

#include "cvgs_detect.h"
#include "cvgs_geometry.h"
#include "cvgs_host.h"

using namespace cvgs;

namespace {
// detector -> frame pixels (select's boxes, gather's points): scales finite and positive, offsets finite
int check_xform(const float* xf, const char* name) {
    if (!fit_finite((double)xf[0]) || !fit_finite((double)xf[1]) || !(xf[0] > 0.0f) || !(xf[1] > 0.0f))
        return fail(CVGS_ERR_INVALID, std::string(name) + ": xform scales (sx, sy) must be finite and positive");
    if (!fit_finite((double)xf[2]) || !fit_finite((double)xf[3])) return fail(CVGS_ERR_INVALID, std::string(name) + ": xform offsets (ox, oy) must be finite");
    return CVGS_OK;
}

// (head_decode and points_gather keep their head-addressing lines in place: gather's max_out and kept_index sit between them)
inline size_t head_elem_bytes(int elem) { return elem == CVGS_HEAD_F32 ? 4 : 2; }

// ---- device plane tables from device-side boxes ---------------------------------------------------------------------------------------
// The kernel (k_boxes.hip) clamps every box into the frame described here, so the checks below bound what the table's planes read.
int check_box_table_desc(const cvgs_box_table_desc& d, OutRanges*, BoxFrame& f) { // (this stage has no overlap test: nothing is collected)
    if (d.struct_size != sizeof(cvgs_box_table_desc)) return fail(CVGS_ERR_INVALID, "cvgs_box_table_desc size mismatch (ABI)");
    if (d.flags) return fail(CVGS_ERR_INVALID, "plane_tables_from_boxes: flags must be 0");
    if (is_area(d.read_kind)) return fail(CVGS_ERR_UNSUPPORTED, "plane_tables_from_boxes: an INTER_AREA chain takes the table of the same chain spelled CVGS_READ_RESIZE_LINEAR (one layout: build it with that kind)");
    if (is_yuv_area(d.read_kind)) return fail(CVGS_ERR_UNSUPPORTED, "plane_tables_from_boxes: an INTER_AREA chain over a decoder surface takes the table of the same chain spelled CVGS_READ_NV12_RESIZE_LINEAR (one layout: build it with that kind)");
    if (d.read_kind < CVGS_READ_PIXEL || d.read_kind > CVGS_READ_WARP_PERSPECTIVE) return fail(CVGS_ERR_INVALID, "bad read kind");
    if (is_warp(d.read_kind)) return fail(CVGS_ERR_UNSUPPORTED, "plane_tables_from_boxes: warp reads (WARP_AFFINE / WARP_PERSPECTIVE) take host descriptors");
    if (!is_resize(d.read_kind))
        return fail(CVGS_ERR_UNSUPPORTED, "plane_tables_from_boxes: per-pixel reads (READ_PIXEL / READ_NV12) are not served, boxes feed the resize kinds");
    const bool yuv = is_nv12(d.read_kind);
    if (yuv) {
        if (d.yuv_layout < CVGS_YUV_NV12 || d.yuv_layout > CVGS_YUV_I444) return fail(CVGS_ERR_INVALID, "bad yuv_layout");
        if (d.yuv_layout != CVGS_YUV_NV12 && d.yuv_layout != CVGS_YUV_NV21)
            return fail(CVGS_ERR_UNSUPPORTED, "plane_tables_from_boxes: device plane tables serve the NV12 / NV21 layouts only (P010 / I420 / YV12 / YUYV / UYVY / I444: host descriptors)");
        if (d.src_type != CVGS_MAKETYPE(CVGS_DEPTH_8U, 1)) return fail(CVGS_ERR_INVALID, "NV12 reads need a CV_8UC1 source");
    }
    if (d.max_boxes < 1 || d.max_boxes > 65535) return fail(CVGS_ERR_INVALID, "max_boxes must be in [1, 65535]");
    if (d.box_format != CVGS_BOX_XYXY_F32 && d.box_format != CVGS_BOX_XYWH_I32) return fail(CVGS_ERR_INVALID, "bad box format");
    if (!d.boxes) return fail(CVGS_ERR_INVALID, "plane_tables_from_boxes: boxes is null");
    if (!d.table_out) return fail(CVGS_ERR_INVALID, "plane_tables_from_boxes: table_out is null");
    if (((uintptr_t)d.table_out & 7) || (((uintptr_t)d.boxes | (uintptr_t)d.count | (uintptr_t)d.rects_out) & 3))
        return fail(CVGS_ERR_INVALID, "plane_tables_from_boxes: table_out needs 8-byte, boxes / count / rects_out 4-byte alignment");
    if (d.dst_width < 1 || d.dst_height < 1) return fail(CVGS_ERR_INVALID, "resize target must be positive");
    if (d.dst_width > kMaxDim || d.dst_height > kMaxDim) return fail(CVGS_ERR_UNSUPPORTED, "resize target wider or taller than 2^24 pixels");
    if (d.aspect_ratio < CVGS_PRESERVE_AR || d.aspect_ratio > CVGS_PRESERVE_AR_LEFT) return fail(CVGS_ERR_INVALID, "bad aspect ratio mode");
    const cvgs_image2d& im = d.frame;
    int esz, rc;
    if ((rc = check_frame_type(d.src_type, &esz)) || (rc = check_frame_plane(im, esz))) return rc;
    // the aspect-ratio fit rounds dst_height / h * w (and dst_width / w * h) to an int: keep every box of the frame inside its range
    if ((int64_t)d.dst_height * im.width > ((int64_t)1 << 30) || (int64_t)d.dst_width * im.height > ((int64_t)1 << 30))
        return fail(CVGS_ERR_UNSUPPORTED, "plane_tables_from_boxes: dst_height * frame width or dst_width * frame height beyond 2^30");
    int64_t uv_off = 0;
    if (yuv) {
        if ((im.width & 1) || (im.height & 1)) return fail(CVGS_ERR_INVALID, "NV12 planes need even dimensions");
        if (im.uv_offset < 0 || (im.uv_offset & 1)) return fail(CVGS_ERR_INVALID, "NV12 uv_offset must be even and non-negative");
        if (im.step & 1) return fail(CVGS_ERR_INVALID, "plane_tables_from_boxes: NV12 frames need an even step (the chroma offset of a crop at row t is uv_offset - (t/2)*step and must be even)");
        uv_off = im.uv_offset ? (int64_t)im.uv_offset : (int64_t)im.height * im.step;
        if (uv_off > INT32_MAX) return fail(CVGS_ERR_UNSUPPORTED, "4:2:0 surfaces whose luma plane exceeds 2 GiB");
        if (uv_off < (int64_t)(im.height / 2) * im.step) return fail(CVGS_ERR_INVALID, "plane_tables_from_boxes: NV12 uv_offset lies inside the luma rows");
    } else if (im.uv_offset) {
        return fail(CVGS_ERR_INVALID, "plane_tables_from_boxes: uv_offset belongs to the NV12 kinds");
    }
    f = BoxFrame{};
    f.data = (const uint8_t*)im.data;
    f.boxes = d.boxes; f.count = d.count;
    f.table = (PlaneParams*)d.table_out; f.rects = d.rects_out;
    f.w = im.width; f.h = im.height; f.step = im.step;
    f.uv_off = (int32_t)uv_off; f.esz = esz; f.yuv420 = yuv ? 1 : 0;
    f.dst_w = d.dst_width; f.dst_h = d.dst_height; f.ar = d.aspect_ratio;
    f.fmt = d.box_format; f.max_boxes = d.max_boxes;
    return CVGS_OK;
}

// ---- device warp tables from device-side landmarks ------------------------------------------------------------------------------------
// The fit itself (cvgs_geometry.h: warp_fit) is one text for the kernel (k_points.hip) and for cvgs_warp_table_build_host.
// `outs` null: cvgs_warp_table_build_host -- desc.table_out is not used
int check_warp_table_desc(const cvgs_warp_table_desc& d, OutRanges* outs, PointFrame& f) {
    if (d.struct_size != sizeof(cvgs_warp_table_desc)) return fail(CVGS_ERR_INVALID, "cvgs_warp_table_desc size mismatch (ABI)");
    if (d.flags) return fail(CVGS_ERR_INVALID, "warp_tables_from_points: flags must be 0");
    if (d.read_kind < CVGS_READ_PIXEL || d.read_kind > CVGS_READ_WARP_PERSPECTIVE) return fail(CVGS_ERR_INVALID, "bad read kind");
    if (!is_warp(d.read_kind)) return fail(CVGS_ERR_UNSUPPORTED, "warp_tables_from_points: warp tables serve the warp reads (WARP_AFFINE / WARP_PERSPECTIVE) only");
    if (d.max_items < 1 || d.max_items > 65535) return fail(CVGS_ERR_INVALID, "max_items must be in [1, 65535]");
    if (d.fit != CVGS_WARP_FIT_SIMILARITY && d.fit != CVGS_WARP_FIT_AFFINE3) return fail(CVGS_ERR_INVALID, "bad warp fit");
    if (d.fit == CVGS_WARP_FIT_SIMILARITY && (d.n_points < 2 || d.n_points > CVGS_WARP_MAX_POINTS))
        return fail(CVGS_ERR_INVALID, "warp_tables_from_points: the similarity fit takes 2..16 points");
    if (d.fit == CVGS_WARP_FIT_AFFINE3 && d.n_points != 3) return fail(CVGS_ERR_INVALID, "warp_tables_from_points: the AFFINE3 fit takes exactly 3 points");
    if (!d.points) return fail(CVGS_ERR_INVALID, "warp_tables_from_points: points is null");
    if (outs && !d.table_out) return fail(CVGS_ERR_INVALID, "warp_tables_from_points: table_out is null");
    if ((outs && ((uintptr_t)d.table_out & 7)) || (((uintptr_t)d.points | (uintptr_t)d.count | (uintptr_t)d.valid_out) & 3))
        return fail(CVGS_ERR_INVALID, "warp_tables_from_points: table_out needs 8-byte, points / count / valid_out 4-byte alignment");
    if (d.dst_width < 1 || d.dst_height < 1) return fail(CVGS_ERR_INVALID, "warp target must be positive");
    if (d.dst_width > kMaxDim || d.dst_height > kMaxDim) return fail(CVGS_ERR_UNSUPPORTED, "warp target wider or taller than 2^24 pixels");
    // the template
    bool coincide = true;
    for (int i = 0; i < d.n_points; ++i) {
        if (!fit_finite((double)d.tmpl[i][0]) || !fit_finite((double)d.tmpl[i][1])) return fail(CVGS_ERR_INVALID, "warp_tables_from_points: template entry is not finite");
        coincide = coincide && d.tmpl[i][0] == d.tmpl[0][0] && d.tmpl[i][1] == d.tmpl[0][1];
    }
    if (d.fit == CVGS_WARP_FIT_SIMILARITY && coincide) return fail(CVGS_ERR_INVALID, "warp_tables_from_points: the template's points all coincide");
    if (d.fit == CVGS_WARP_FIT_AFFINE3) {
        const double q0x = (double)d.tmpl[0][0], q0y = (double)d.tmpl[0][1];
        const double e1x = (double)d.tmpl[1][0] - q0x, e1y = (double)d.tmpl[1][1] - q0y, e2x = (double)d.tmpl[2][0] - q0x, e2y = (double)d.tmpl[2][1] - q0y;
        const double det = e1x * e2y - e1y * e2x; // as warp_fit forms it
        if (det == 0.0 || !fit_finite(det)) return fail(CVGS_ERR_INVALID, "warp_tables_from_points: the AFFINE3 template has zero area");
    }
    const cvgs_image2d& im = d.frame;
    int esz, rc;
    if ((rc = check_frame_type(d.src_type, &esz))) return rc;
    if (type_depth(d.src_type) == CVGS_DEPTH_64F) return fail(CVGS_ERR_UNSUPPORTED, "device warp tables: CV_64F sources take host descriptors");
    if ((rc = check_frame_plane(im, esz))) return rc;
    if (im.uv_offset) return fail(CVGS_ERR_INVALID, "warp_tables_from_points: uv_offset belongs to the NV12 kinds");
    f = PointFrame{};
    f.data = (const uint8_t*)im.data;
    f.points = d.points; f.count = d.count;
    f.table = (WarpPlane*)d.table_out; f.valid = d.valid_out;
    f.w = im.width; f.h = im.height; f.step = im.step;
    f.dst_w = d.dst_width; f.dst_h = d.dst_height;
    f.fit = d.fit; f.n_points = d.n_points;
    f.max_items = d.max_items;
    for (int i = 0; i < d.n_points; ++i) { f.tmpl[2 * i] = d.tmpl[i][0]; f.tmpl[2 * i + 1] = d.tmpl[i][1]; }
    if (!outs) return CVGS_OK;
    outs->add(f.table, (size_t)f.max_items * sizeof(WarpPlane));
    outs->add(f.valid, (size_t)f.max_items * sizeof(int32_t));
    return CVGS_OK;
}

// ---- device-side box selection (THE CONTRACT: include/cvgs_hip_ext.h) -------------------------------------------------------------------
// Steps 2-5, the order and the suppression predicate (cvgs_geometry.h) are one text for the kernels (k_select.hip) and the host twin.
// `outs` null: cvgs_boxes_select_host -- desc.scratch and the descriptor's output pointers are not used
int check_select_desc(const cvgs_box_select_desc& d, OutRanges* outs, SelectFrame& f) {
    if (d.struct_size != sizeof(cvgs_box_select_desc)) return fail(CVGS_ERR_INVALID, "cvgs_box_select_desc size mismatch (ABI)");
    if (d.flags) return fail(CVGS_ERR_INVALID, "boxes_select: flags must be 0");
    if (d.frame_width < 1 || d.frame_height < 1) return fail(CVGS_ERR_INVALID, "boxes_select: frame_width / frame_height must be positive");
    if (d.frame_width > kMaxDim || d.frame_height > kMaxDim) return fail(CVGS_ERR_UNSUPPORTED, "boxes_select: frame wider or taller than 2^24 pixels");
    if (d.box_format != CVGS_CAND_XYXY_F32 && d.box_format != CVGS_CAND_CXCYWH_F32) return fail(CVGS_ERR_INVALID, "boxes_select: bad box format");
    if (d.max_candidates < 1 || d.max_candidates > 65535) return fail(CVGS_ERR_INVALID, "boxes_select: max_candidates must be in [1, 65535]");
    if (!d.boxes) return fail(CVGS_ERR_INVALID, "boxes_select: boxes is null");
    if (!d.scores) return fail(CVGS_ERR_INVALID, "boxes_select: scores is null");
    if (d.box_stride < 4) return fail(CVGS_ERR_INVALID, "boxes_select: box_stride must be at least 4 floats");
    if (d.score_stride < 1) return fail(CVGS_ERR_INVALID, "boxes_select: score_stride must be at least 1 float");
    if (d.classes && d.class_stride < 1) return fail(CVGS_ERR_INVALID, "boxes_select: class_stride must be at least 1 with classes");
    if (d.pre_nms_k < 1 || d.pre_nms_k > CVGS_SELECT_MAX_PRE_NMS) return fail(CVGS_ERR_INVALID, "boxes_select: pre_nms_k must be in [1, 1024]");
    if (d.max_out < 1 || d.max_out > d.pre_nms_k) return fail(CVGS_ERR_INVALID, "boxes_select: max_out must be in [1, pre_nms_k]");
    if (d.reserved) return fail(CVGS_ERR_INVALID, "boxes_select: reserved must be 0");
    if (d.score_threshold != d.score_threshold) return fail(CVGS_ERR_INVALID, "boxes_select: score_threshold is NaN");
    if (!(d.iou_threshold >= 0.0f && d.iou_threshold <= 1.0f)) return fail(CVGS_ERR_INVALID, "boxes_select: iou_threshold must be in [0, 1]");
    if (const int rc = check_xform(d.xform, "boxes_select")) return rc;
    if (((uintptr_t)d.boxes | (uintptr_t)d.scores | (uintptr_t)d.classes | (uintptr_t)d.count) & 3)
        return fail(CVGS_ERR_INVALID, "boxes_select: boxes / scores / classes / count need 4-byte alignment");
    if (outs) {
        if (!d.scratch) return fail(CVGS_ERR_INVALID, "boxes_select: scratch is null");
        if (!d.boxes_out) return fail(CVGS_ERR_INVALID, "boxes_select: boxes_out is null");
        if (!d.count_out) return fail(CVGS_ERR_INVALID, "boxes_select: count_out is null");
        if (((uintptr_t)d.scratch & 7) || (((uintptr_t)d.boxes_out | (uintptr_t)d.count_out | (uintptr_t)d.scores_out | (uintptr_t)d.index_out) & 3))
            return fail(CVGS_ERR_INVALID, "boxes_select: scratch needs 8-byte, boxes_out / count_out / scores_out / index_out 4-byte alignment");
    }
    f = SelectFrame{};
    f.boxes = d.boxes; f.scores = d.scores; f.classes = d.classes; f.count = d.count;
    if (outs) {
        f.scratch = (uint8_t*)d.scratch;
        f.boxes_out = d.boxes_out; f.count_out = d.count_out; f.scores_out = d.scores_out; f.index_out = d.index_out;
    }
    f.w = d.frame_width; f.h = d.frame_height; f.fmt = d.box_format; f.max_cand = d.max_candidates;
    f.box_stride = d.box_stride; f.score_stride = d.score_stride; f.class_stride = d.classes ? d.class_stride : 0;
    f.pre_k = d.pre_nms_k; f.max_out = d.max_out;
    f.score_thr = d.score_threshold; f.iou_thr = d.iou_threshold;
    for (int k = 0; k < 4; ++k) f.xf[k] = d.xform[k];
    if (!outs) return CVGS_OK;
    outs->add(f.scratch, select_scratch_bytes(f.pre_k));
    outs->add(f.boxes_out, (size_t)f.max_out * 4 * sizeof(float));
    outs->add(f.count_out, sizeof(int32_t));
    outs->add(f.scores_out, (size_t)f.max_out * sizeof(float));
    outs->add(f.index_out, (size_t)f.max_out * sizeof(int32_t));
    return CVGS_OK;
}

// ---- a detector's raw head -> select's candidates (THE CONTRACT: include/cvgs_hip_ext.h) ------------------------------------------------
// The widening, the best class in both forms, the score and the membership test (cvgs_geometry.h): one text for k_head.hip and the host twin.
// `outs` null: cvgs_head_decode_host -- desc.scratch and the descriptor's output pointers are not used
int check_head_desc(const cvgs_head_desc& d, OutRanges* outs, HeadFrame& f) {
    if (d.struct_size != sizeof(cvgs_head_desc)) return fail(CVGS_ERR_INVALID, "cvgs_head_desc size mismatch (ABI)");
    if (d.flags) return fail(CVGS_ERR_INVALID, "head_decode: flags must be 0");
    if (d.reserved) return fail(CVGS_ERR_INVALID, "head_decode: reserved must be 0");
    if (d.elem_type != CVGS_HEAD_F32 && d.elem_type != CVGS_HEAD_F16 && d.elem_type != CVGS_HEAD_BF16) return fail(CVGS_ERR_INVALID, "head_decode: bad elem_type");
    if (d.max_candidates < 1 || d.max_candidates > 65535) return fail(CVGS_ERR_INVALID, "head_decode: max_candidates must be in [1, 65535]");
    if (!d.head) return fail(CVGS_ERR_INVALID, "head_decode: head is null");
    if (d.cand_stride < 1) return fail(CVGS_ERR_INVALID, "head_decode: cand_stride must be at least 1 element");
    if (d.attr_stride < 1) return fail(CVGS_ERR_INVALID, "head_decode: attr_stride must be at least 1 element");
    if (d.num_classes < 1 || d.num_classes > CVGS_HEAD_MAX_CLASSES) return fail(CVGS_ERR_INVALID, "head_decode: num_classes must be in [1, 4096]");
    if (d.box_attr < 0 || d.box_attr + 3 > CVGS_HEAD_MAX_ATTR) return fail(CVGS_ERR_INVALID, "head_decode: box_attr .. box_attr + 3 must lie in [0, 8191]");
    if (d.obj_attr < -1 || d.obj_attr > CVGS_HEAD_MAX_ATTR) return fail(CVGS_ERR_INVALID, "head_decode: obj_attr must be -1 or lie in [0, 8191]");
    if (d.class_attr < 0 || d.class_attr > CVGS_HEAD_MAX_ATTR || d.class_attr + d.num_classes - 1 > CVGS_HEAD_MAX_ATTR)
        return fail(CVGS_ERR_INVALID, "head_decode: class_attr .. class_attr + num_classes - 1 must lie in [0, 8191]");
    if (d.score_threshold != d.score_threshold) return fail(CVGS_ERR_INVALID, "head_decode: score_threshold is NaN");
    if ((uintptr_t)d.head & (head_elem_bytes(d.elem_type) - 1)) return fail(CVGS_ERR_INVALID, "head_decode: head needs the alignment of its element type");
    if (outs) {
        if (!d.scratch) return fail(CVGS_ERR_INVALID, "head_decode: scratch is null");
        if (!d.boxes_out) return fail(CVGS_ERR_INVALID, "head_decode: boxes_out is null");
        if (!d.scores_out) return fail(CVGS_ERR_INVALID, "head_decode: scores_out is null");
        if (!d.classes_out) return fail(CVGS_ERR_INVALID, "head_decode: classes_out is null");
        if (!d.count_out) return fail(CVGS_ERR_INVALID, "head_decode: count_out is null");
        if (((uintptr_t)d.scratch & 7) ||
            (((uintptr_t)d.boxes_out | (uintptr_t)d.scores_out | (uintptr_t)d.classes_out | (uintptr_t)d.index_out | (uintptr_t)d.count_out) & 3))
            return fail(CVGS_ERR_INVALID, "head_decode: scratch needs 8-byte, boxes_out / scores_out / classes_out / index_out / count_out 4-byte alignment");
    }
    f = HeadFrame{};
    f.head = d.head;
    if (outs) {
        f.scratch = (uint8_t*)d.scratch;
        f.boxes_out = d.boxes_out; f.scores_out = d.scores_out; f.classes_out = d.classes_out; f.index_out = d.index_out; f.count_out = d.count_out;
    }
    f.elem = d.elem_type; f.n = d.max_candidates;
    f.cand_stride = d.cand_stride; f.attr_stride = d.attr_stride;
    f.box_attr = d.box_attr; f.obj_attr = d.obj_attr; f.class_attr = d.class_attr; f.num_classes = d.num_classes;
    f.score_thr = d.score_threshold;
    // the score launch's form: contiguous attributes are read by a group of lanes per candidate (the next power of two at or above
    // num_classes, 4 .. 64), everything else by one lane per candidate
    f.group = 0;
    if (d.attr_stride == 1) {
        int g = 4;
        while (g < 64 && g < d.num_classes) g *= 2;
        f.group = g;
    }
    if (!outs) return CVGS_OK;
    const size_t N = (size_t)f.n;
    outs->add(f.scratch, head_scratch_bytes(f.n));
    outs->add(f.boxes_out, N * 4 * sizeof(float));
    outs->add(f.scores_out, N * sizeof(float));
    outs->add(f.classes_out, N * sizeof(int32_t));
    outs->add(f.count_out, sizeof(int32_t));
    outs->add(f.index_out, N * sizeof(int32_t));
    return CVGS_OK;
}

inline float head_host_at(int elem, const void* head, size_t idx) { // step 1
    if (elem == CVGS_HEAD_F32) return ((const float*)head)[idx];
    const uint16_t h = ((const uint16_t*)head)[idx];
    return elem == CVGS_HEAD_F16 ? head_widen_f16(h) : head_widen_bf16(h);
}

// ---- the landmarks of kept detections -> the points of cvgs_warp_tables_from_points (THE CONTRACT: include/cvgs_hip_ext.h) --------------
// The row's source, the element index, the widening and the mapping (cvgs_geometry.h: gather_point): one text for k_gather.hip and the host twin.
// the outputs: the descriptor's (cvgs_points_gather) or the caller's in their place (cvgs_points_gather_host, `outs` null)
int check_gather_desc(const cvgs_point_gather_desc& d, float* points_out, float* conf_out, int32_t* source_out, OutRanges* outs, GatherFrame& f) {
    if (d.struct_size != sizeof(cvgs_point_gather_desc)) return fail(CVGS_ERR_INVALID, "cvgs_point_gather_desc size mismatch (ABI)");
    if (d.flags) return fail(CVGS_ERR_INVALID, "points_gather: flags must be 0");
    if (d.reserved) return fail(CVGS_ERR_INVALID, "points_gather: reserved must be 0");
    if (d.elem_type != CVGS_HEAD_F32 && d.elem_type != CVGS_HEAD_F16 && d.elem_type != CVGS_HEAD_BF16) return fail(CVGS_ERR_INVALID, "points_gather: bad elem_type");
    if (d.max_candidates < 1 || d.max_candidates > 65535) return fail(CVGS_ERR_INVALID, "points_gather: max_candidates must be in [1, 65535]");
    if (d.max_out < 1 || d.max_out > 65535) return fail(CVGS_ERR_INVALID, "points_gather: max_out must be in [1, 65535]");
    if (!d.head) return fail(CVGS_ERR_INVALID, "points_gather: head is null");
    if (!d.kept_index) return fail(CVGS_ERR_INVALID, "points_gather: kept_index is null");
    if (d.cand_stride < 1) return fail(CVGS_ERR_INVALID, "points_gather: cand_stride must be at least 1 element");
    if (d.attr_stride < 1) return fail(CVGS_ERR_INVALID, "points_gather: attr_stride must be at least 1 element");
    if (d.point_step < 2) return fail(CVGS_ERR_INVALID, "points_gather: point_step must be at least 2 attributes");
    if (d.n_points < 1 || d.n_points > CVGS_GATHER_MAX_POINTS) return fail(CVGS_ERR_INVALID, "points_gather: n_points must be in [1, 64]");
    if (d.conf_offset != -1 && (d.conf_offset < 2 || d.conf_offset >= d.point_step))
        return fail(CVGS_ERR_INVALID, "points_gather: conf_offset must be -1 or lie in [2, point_step)");
    if (!points_out) return fail(CVGS_ERR_INVALID, "points_gather: points_out is null");
    if (conf_out && d.conf_offset == -1) return fail(CVGS_ERR_INVALID, "points_gather: conf_out given without a conf_offset");
    if (!conf_out && d.conf_offset != -1) return fail(CVGS_ERR_INVALID, "points_gather: conf_offset given without conf_out");
    // the last attribute addressed: y, or the confidence, of the last point (64 bits: point_step has no upper bound of its own)
    const int64_t last = (int64_t)d.point_attr + (int64_t)(d.n_points - 1) * (int64_t)d.point_step + (d.conf_offset > 1 ? d.conf_offset : 1);
    if (d.point_attr < 0 || last > CVGS_HEAD_MAX_ATTR) return fail(CVGS_ERR_INVALID, "points_gather: the attributes of the points must lie in [0, 8191]");
    if ((uintptr_t)d.head & (head_elem_bytes(d.elem_type) - 1)) return fail(CVGS_ERR_INVALID, "points_gather: head needs the alignment of its element type");
    if (((uintptr_t)d.kept_index | (uintptr_t)d.kept_count | (uintptr_t)d.cand_index | (uintptr_t)points_out | (uintptr_t)conf_out | (uintptr_t)source_out) & 3)
        return fail(CVGS_ERR_INVALID, "points_gather: kept_index / kept_count / cand_index / points_out / conf_out / source_out need 4-byte alignment");
    if (const int rc = check_xform(d.xform, "points_gather")) return rc;
    f = GatherFrame{};
    f.head = d.head; f.kept_index = d.kept_index; f.kept_count = d.kept_count; f.cand_index = d.cand_index;
    f.points_out = points_out; f.conf_out = conf_out; f.source_out = source_out;
    f.elem = d.elem_type; f.max_cand = d.max_candidates;
    f.cand_stride = d.cand_stride; f.attr_stride = d.attr_stride;
    f.point_attr = d.point_attr; f.point_step = d.point_step;
    f.n_points = d.n_points; f.conf_offset = d.conf_offset;
    f.max_out = d.max_out;
    for (int k = 0; k < 4; ++k) f.xf[k] = d.xform[k];
    if (!outs) return CVGS_OK;
    const size_t items = (size_t)f.max_out * (size_t)f.n_points;
    outs->add(f.points_out, items * 2 * sizeof(float));
    outs->add(f.conf_out, items * sizeof(float));
    outs->add(f.source_out, (size_t)f.max_out * sizeof(int32_t));
    return CVGS_OK;
}
int check_gather_device(const cvgs_point_gather_desc& d, OutRanges* outs, GatherFrame& f) { return check_gather_desc(d, d.points_out, d.conf_out, d.source_out, outs, f); }

} // namespace

extern "C" {
int cvgs_plane_tables_from_boxes(const cvgs_box_table_desc* descs, int32_t n, cvgs_stream_t stream) {
    static const char* const text[4] = {"plane_tables_from_boxes: null descriptors", "plane_tables_from_boxes: n must be in [1, CVGS_MAX_CHAINS]", nullptr, "plane_tables_from_boxes: kernel launch"};
    return run_stage<CVGS_MAX_CHAINS, 0>(text, descs, n, stream, check_box_table_desc, launch_boxes);
}

size_t cvgs_warp_table_bytes(int32_t planes) { return planes > 0 ? (size_t)planes * sizeof(WarpPlane) : 0; }

int cvgs_warp_tables_from_points(const cvgs_warp_table_desc* descs, int32_t n, cvgs_stream_t stream) {
    static const char* const text[4] = {"warp_tables_from_points: null descriptors", "warp_tables_from_points: n must be in [1, 16]", "warp_tables_from_points: the output buffers of one call overlap", "warp_tables_from_points: kernel launch"};
    return run_stage<CVGS_WARP_MAX_FRAMES, 2>(text, descs, n, stream, check_warp_table_desc, launch_points);
}

int cvgs_warp_table_build_host(const cvgs_warp_table_desc* desc, void* table_out_host) {
    if (!desc || !table_out_host) return fail(CVGS_ERR_INVALID, "warp_table_build_host: null argument");
    PointFrame f;
    if (const int rc = check_warp_table_desc(*desc, nullptr, f)) return rc;
    const int live = live_count(f.count, f.max_items);
    for (int i = 0; i < f.max_items; ++i) { // k_points' body
        WarpPlane P;
        std::memset(&P, 0, sizeof(P));
        P.data = f.data; P.w = f.w; P.h = f.h; P.step = f.step;
        P.dw = f.dst_w; P.dh = f.dst_h;
        const bool ok = warp_fit(f.fit, f.n_points, f.points + (size_t)i * (size_t)f.n_points * 2, f.tmpl, i < live, P.m);
        std::memcpy((uint8_t*)table_out_host + (size_t)i * sizeof(WarpPlane), &P, sizeof(P));
        if (f.valid) f.valid[i] = ok ? 1 : 0;
    }
    return CVGS_OK;
}

size_t cvgs_boxes_select_scratch_bytes(int32_t max_candidates, int32_t pre_nms_k) {
    return max_candidates < 1 || max_candidates > 65535 || pre_nms_k < 1 || pre_nms_k > CVGS_SELECT_MAX_PRE_NMS ? 0 : select_scratch_bytes(pre_nms_k);
}

int cvgs_boxes_select(const cvgs_box_select_desc* descs, int32_t n, cvgs_stream_t stream) {
    static const char* const text[4] = {"boxes_select: null descriptors", "boxes_select: n must be in [1, 16]", "boxes_select: the output and scratch buffers of one call overlap", "boxes_select: kernel launch"};
    return run_stage<CVGS_SELECT_MAX_FRAMES, 5>(text, descs, n, stream, check_select_desc, launch_select);
}

int cvgs_boxes_select_host(const cvgs_box_select_desc* desc, void* boxes_out, int32_t* count_out, float* scores_out, int32_t* index_out) {
    if (!desc || !boxes_out || !count_out) return fail(CVGS_ERR_INVALID, "boxes_select_host: null argument");
    SelectFrame f;
    if (const int rc = check_select_desc(*desc, nullptr, f)) return rc;
    const int live = live_count(f.count, f.max_cand);
    struct Cand { float box[4], score; int32_t index, cls; };
    std::vector<Cand> work; // steps 2-5, then step 6: the order k_select_rank finds by counting
    for (int i = 0; i < live; ++i) {
        const float* q = f.boxes + (size_t)i * (size_t)f.box_stride;
        Cand c;
        c.score = f.scores[(size_t)i * (size_t)f.score_stride];
        c.index = i;
        if (!select_prepare(f.fmt, q[0], q[1], q[2], q[3], c.score, f.score_thr, f.xf, f.w, f.h, c.box)) continue;
        c.cls = f.classes ? f.classes[(size_t)i * (size_t)f.class_stride] : 0;
        work.push_back(c);
    }
    std::sort(work.begin(), work.end(), [](const Cand& a, const Cand& b) { return select_precedes(a.score, a.index, b.score, b.index); });
    if (work.size() > (size_t)f.pre_k) work.resize((size_t)f.pre_k);
    std::vector<int> kept; // step 7
    for (size_t i = 0; i < work.size() && (int)kept.size() < f.max_out; ++i) {
        const Cand& c = work[i];
        bool sup = false;
        for (size_t k = 0; k < kept.size() && !sup; ++k) {
            const Cand& j = work[(size_t)kept[k]];
            sup = j.cls == c.cls && select_suppresses(j.box[0], j.box[1], j.box[2], j.box[3], c.box[0], c.box[1], c.box[2], c.box[3], f.iou_thr);
        }
        if (!sup) kept.push_back((int)i);
    }
    float* bo = (float*)boxes_out; // step 8: every element
    for (int k = 0; k < f.max_out; ++k) {
        const Cand* c = k < (int)kept.size() ? &work[(size_t)kept[(size_t)k]] : nullptr;
        for (int e = 0; e < 4; ++e) bo[(size_t)k * 4 + e] = c ? c->box[e] : 0.0f;
        if (scores_out) scores_out[k] = c ? c->score : 0.0f;
        if (index_out) index_out[k] = c ? c->index : -1;
    }
    *count_out = (int32_t)kept.size();
    return CVGS_OK;
}

size_t cvgs_head_decode_scratch_bytes(int32_t max_candidates) {
    return max_candidates < 1 || max_candidates > 65535 ? 0 : head_scratch_bytes(max_candidates);
}

int cvgs_head_decode(const cvgs_head_desc* descs, int32_t n, cvgs_stream_t stream) {
    static const char* const text[4] = {"head_decode: null descriptors", "head_decode: n must be in [1, 16]", "head_decode: the output and scratch buffers of one call overlap", "head_decode: kernel launch"};
    return run_stage<CVGS_HEAD_MAX_FRAMES, 6>(text, descs, n, stream, check_head_desc, launch_head);
}

int cvgs_head_decode_host(const cvgs_head_desc* desc, float* boxes_out, float* scores_out, int32_t* classes_out, int32_t* index_out, int32_t* count_out) {
    if (!desc || !boxes_out || !scores_out || !classes_out || !count_out) return fail(CVGS_ERR_INVALID, "head_decode_host: null argument");
    HeadFrame f;
    if (const int rc = check_head_desc(*desc, nullptr, f)) return rc;
    const size_t as = (size_t)f.attr_stride;
    const bool has_obj = f.obj_attr >= 0;
    int k = 0;
    for (int i = 0; i < f.n; ++i) { // steps 1-5, in candidate order
        const size_t at = (size_t)i * (size_t)f.cand_stride;
        float best = -INFINITY;
        int cls = 0;
        for (int c = 0; c < f.num_classes; ++c) head_best_step(head_host_at(f.elem, f.head, at + (size_t)(f.class_attr + c) * as), c, &best, &cls);
        const float obj = has_obj ? head_host_at(f.elem, f.head, at + (size_t)f.obj_attr * as) : 0.0f;
        const float s = head_score(best, has_obj, obj);
        float co[4];
        for (int e = 0; e < 4; ++e) co[e] = head_host_at(f.elem, f.head, at + (size_t)(f.box_attr + e) * as);
        if (!head_member(s, f.score_thr, co[0], co[1], co[2], co[3])) continue;
        for (int e = 0; e < 4; ++e) boxes_out[(size_t)k * 4 + e] = co[e];
        scores_out[k] = s;
        classes_out[k] = cls;
        if (index_out) index_out[k] = i;
        ++k;
    }
    *count_out = k;
    for (; k < f.n; ++k) { // step 6
        for (int e = 0; e < 4; ++e) boxes_out[(size_t)k * 4 + e] = 0.0f;
        scores_out[k] = 0.0f;
        classes_out[k] = 0;
        if (index_out) index_out[k] = -1;
    }
    return CVGS_OK;
}

int cvgs_points_gather(const cvgs_point_gather_desc* descs, int32_t n, cvgs_stream_t stream) {
    static const char* const text[4] = {"points_gather: null descriptors", "points_gather: n must be in [1, 16]", "points_gather: the output buffers of one call overlap", "points_gather: kernel launch"};
    return run_stage<CVGS_GATHER_MAX_FRAMES, 3>(text, descs, n, stream, check_gather_device, launch_gather);
}

int cvgs_points_gather_host(const cvgs_point_gather_desc* desc, float* points_out, float* conf_out, int32_t* source_out) {
    if (!desc) return fail(CVGS_ERR_INVALID, "points_gather_host: null argument");
    GatherFrame f;
    if (const int rc = check_gather_desc(*desc, points_out, conf_out, source_out, nullptr, f)) return rc;
    const int live = live_count(f.kept_count, f.max_out);
    for (int j = 0; j < f.max_out; ++j) // k_points_gather's work-items, in order
        for (int p = 0; p < f.n_points; ++p) {
            switch (f.elem) {
            case CVGS_HEAD_F32: gather_point<CVGS_HEAD_F32>(f, j, p, live); break;
            case CVGS_HEAD_F16: gather_point<CVGS_HEAD_F16>(f, j, p, live); break;
            default: gather_point<CVGS_HEAD_BF16>(f, j, p, live); break;
            }
        }
    return CVGS_OK;
}
} // extern "C"
