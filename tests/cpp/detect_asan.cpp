// The detector-side host file of the C-ABI (csrc/cvgs_detect.cpp) as a stand-alone program for AddressSanitizer + UBSan: no HIP, no library.
//   make -C tests/cpp bin/detect_asan && tests/cpp/bin/detect_asan        (tests/test_detect_refusals.py builds and runs it too)
// The file is compiled INTO this program; cvgs::fail / cvgs::hip_fail record code and text here, and the five launchers keep the frames they
// are handed.  Checked: (1) the frames a good descriptor lowers to, field by field; (2) the output-range collector at its full capacity,
// and the overlap refusal from its last slot; (3) given a case file, every host twin over heap buffers of exactly the size the contract
// states, so that the sanitizer guards their ends, against the bytes recorded from the parent commit's library.  The last line is the verdict: "N checks, 0 bad".
#include "../../cvgpuspeedup_amd/csrc/cvgs_detect.cpp"

#include <cstdio>
#include <cstdlib>
#include <memory>

namespace {
int g_code = 0;
std::string g_text;
std::vector<BoxFrame> g_box;
std::vector<PointFrame> g_point;
std::vector<SelectFrame> g_select;
std::vector<HeadFrame> g_head;
std::vector<GatherFrame> g_gather;
} // namespace

namespace cvgs {
int fail(int code, const std::string& msg) { g_code = code; g_text = msg; return code; }
int hip_fail(int hip_error, const char* what) { return fail(CVGS_ERR_HIP, std::string(what) + ": hip error " + std::to_string(hip_error)); }
int launch_boxes(const BoxFrame* f, int n, void*) { g_box.assign(f, f + n); return 0; }
int launch_points(const PointFrame* f, int n, void*) { g_point.assign(f, f + n); return 0; }
int launch_select(const SelectFrame* f, int n, void*) { g_select.assign(f, f + n); return 0; }
int launch_head(const HeadFrame* f, int n, void*) { g_head.assign(f, f + n); return n == 3 ? 719 : 0; } // (three frames: the launch "fails")
int launch_gather(const GatherFrame* f, int n, void*) { g_gather.assign(f, f + n); return 0; }
} // namespace cvgs

namespace {
int checks = 0, bad = 0;
void expect(bool ok, const char* what, int line) {
    ++checks;
    if (!ok) { ++bad; std::printf("WRONG line %d: %s   (last text: %s)\n", line, what, g_text.c_str()); }
}
#define EXPECT(c) expect((c), #c, __LINE__)

template <typename T> T* at(uintptr_t a) { return (T*)a; } // a pretend device address: never dereferenced

cvgs_head_desc head_desc(int num_classes, int attr_stride, int k) {
    cvgs_head_desc d{};
    const uintptr_t o = (uintptr_t)k << 24;
    d.struct_size = sizeof(d);
    d.head = at<void>(0x10000);
    d.elem_type = CVGS_HEAD_BF16; d.max_candidates = 8400;
    d.cand_stride = attr_stride == 1 ? 4 + 4096 : 1; d.attr_stride = attr_stride;
    d.box_attr = 0; d.obj_attr = -1; d.class_attr = 4; d.num_classes = num_classes;
    d.score_threshold = 0.25f;
    d.scratch = at<void>(0x100000 + o); d.boxes_out = at<float>(0x200000 + o); d.scores_out = at<float>(0x300000 + o);
    d.classes_out = at<int32_t>(0x400000 + o); d.count_out = at<int32_t>(0x500000 + o); d.index_out = at<int32_t>(0x600000 + o);
    return d;
}
cvgs_box_select_desc select_desc(int k) {
    cvgs_box_select_desc d{};
    const uintptr_t o = (uintptr_t)k << 24;
    d.struct_size = sizeof(d);
    d.frame_width = 1920; d.frame_height = 1080; d.box_format = CVGS_CAND_CXCYWH_F32; d.max_candidates = 8400;
    d.boxes = at<float>(0x10000); d.scores = at<float>(0x40000); d.classes = at<int32_t>(0x60000); d.count = at<int32_t>(0x80000);
    d.box_stride = 4; d.score_stride = 1; d.class_stride = 1; d.pre_nms_k = 1024; d.max_out = 50;
    d.score_threshold = 0.25f; d.iou_threshold = 0.5f;
    d.xform[0] = 3.0f; d.xform[1] = 1.6875f; d.xform[2] = 0.0f; d.xform[3] = -20.0f;
    d.scratch = at<void>(0x100000 + o); d.boxes_out = at<float>(0x200000 + o); d.count_out = at<int32_t>(0x210000 + o);
    d.scores_out = at<float>(0x220000 + o); d.index_out = at<int32_t>(0x230000 + o);
    return d;
}
cvgs_point_gather_desc gather_desc(int k) {
    cvgs_point_gather_desc d{};
    const uintptr_t o = (uintptr_t)k << 24;
    d.struct_size = sizeof(d);
    d.head = at<void>(0x10000); d.elem_type = CVGS_HEAD_BF16; d.max_candidates = 8400; d.cand_stride = 1; d.attr_stride = 8400;
    d.point_attr = 5; d.point_step = 3; d.n_points = 5; d.conf_offset = 2; d.max_out = 50;
    d.kept_index = at<int32_t>(0x100000); d.kept_count = at<int32_t>(0x300000); d.cand_index = at<int32_t>(0x400000);
    d.xform[0] = 3.0f; d.xform[1] = 1.6875f; d.xform[2] = 0.0f; d.xform[3] = -20.0f;
    d.points_out = at<float>(0x200000 + o); d.conf_out = at<float>(0x500000 + o); d.source_out = at<int32_t>(0x600000 + o);
    return d;
}
cvgs_warp_table_desc warp_desc(int k, int fit = CVGS_WARP_FIT_SIMILARITY) {
    cvgs_warp_table_desc d{};
    const uintptr_t o = (uintptr_t)k << 24;
    d.struct_size = sizeof(d);
    d.frame = cvgs_image2d{at<void>(4096), 97, 61, 304, 0};
    d.src_type = CVGS_MAKETYPE(CVGS_DEPTH_8U, 3); d.read_kind = CVGS_READ_WARP_AFFINE;
    d.dst_width = 112; d.dst_height = 96; d.fit = fit; d.n_points = fit == CVGS_WARP_FIT_SIMILARITY ? 5 : 3;
    const float t[5][2] = {{38.25f, 51.5f}, {73.5f, 51.5f}, {56.0f, 71.75f}, {41.5f, 92.25f}, {70.75f, 92.25f}};
    for (int i = 0; i < 5; ++i) { d.tmpl[i][0] = t[i][0]; d.tmpl[i][1] = t[i][1]; }
    d.max_items = 24;
    d.points = at<float>(0x100000); d.count = at<int32_t>(0x180000);
    d.table_out = at<void>(0x200000 + o); d.valid_out = at<int32_t>(0x300000 + o);
    return d;
}
cvgs_box_table_desc box_desc() {
    cvgs_box_table_desc d{};
    d.struct_size = sizeof(d);
    d.frame = cvgs_image2d{at<void>(4096), 130, 66, 132, 0};
    d.read_kind = CVGS_READ_NV12_RESIZE_LINEAR; d.src_type = CVGS_MAKETYPE(CVGS_DEPTH_8U, 1); d.yuv_layout = CVGS_YUV_NV21;
    d.dst_width = 64; d.dst_height = 128; d.aspect_ratio = CVGS_PRESERVE_AR; d.box_format = CVGS_BOX_XYWH_I32; d.max_boxes = 24;
    d.boxes = at<void>(1 << 20); d.count = at<int32_t>(3 << 20); d.table_out = at<void>(2 << 20); d.rects_out = at<int32_t>(5 << 20);
    return d;
}

// ---- (1) the frames a good descriptor lowers to -----------------------------------------------------------------------------------------
void frames_field_by_field() {
    const cvgs_box_table_desc b = box_desc();
    EXPECT(cvgs_plane_tables_from_boxes(&b, 1, nullptr) == CVGS_OK && g_box.size() == 1);
    const BoxFrame& bf = g_box[0];
    EXPECT(bf.data == b.frame.data && bf.boxes == b.boxes && bf.count == b.count && (void*)bf.table == b.table_out && bf.rects == b.rects_out);
    EXPECT(bf.w == 130 && bf.h == 66 && bf.step == 132 && bf.uv_off == 66 * 132 && bf.esz == 1 && bf.yuv420 == 1);
    EXPECT(bf.dst_w == 64 && bf.dst_h == 128 && bf.ar == CVGS_PRESERVE_AR && bf.fmt == CVGS_BOX_XYWH_I32 && bf.max_boxes == 24);
    EXPECT(bf.pad[0] == 0 && bf.pad[1] == 0 && bf.pad[2] == 0);

    const cvgs_warp_table_desc w = warp_desc(0);
    EXPECT(cvgs_warp_tables_from_points(&w, 1, nullptr) == CVGS_OK && g_point.size() == 1);
    const PointFrame& pf = g_point[0];
    EXPECT(pf.data == w.frame.data && pf.points == w.points && pf.count == w.count && (void*)pf.table == w.table_out && pf.valid == w.valid_out);
    EXPECT(pf.w == 97 && pf.h == 61 && pf.step == 304 && pf.dst_w == 112 && pf.dst_h == 96 && pf.fit == CVGS_WARP_FIT_SIMILARITY && pf.n_points == 5 && pf.max_items == 24);
    bool tmpl = true;
    for (int i = 0; i < 2 * CVGS_WARP_MAX_POINTS; ++i) tmpl = tmpl && pf.tmpl[i] == (i < 10 ? w.tmpl[i / 2][i % 2] : 0.0f);
    EXPECT(tmpl);

    const cvgs_box_select_desc s = select_desc(0);
    EXPECT(cvgs_boxes_select(&s, 1, nullptr) == CVGS_OK && g_select.size() == 1);
    const SelectFrame& sf = g_select[0];
    EXPECT(sf.boxes == s.boxes && sf.scores == s.scores && sf.classes == s.classes && sf.count == s.count && (void*)sf.scratch == s.scratch);
    EXPECT(sf.boxes_out == s.boxes_out && sf.count_out == s.count_out && sf.scores_out == s.scores_out && sf.index_out == s.index_out);
    EXPECT(sf.w == 1920 && sf.h == 1080 && sf.fmt == CVGS_CAND_CXCYWH_F32 && sf.max_cand == 8400 && sf.box_stride == 4 && sf.score_stride == 1 && sf.class_stride == 1);
    EXPECT(sf.pre_k == 1024 && sf.max_out == 50 && sf.score_thr == 0.25f && sf.iou_thr == 0.5f && sf.pad == 0);
    EXPECT(sf.xf[0] == 3.0f && sf.xf[1] == 1.6875f && sf.xf[2] == 0.0f && sf.xf[3] == -20.0f);
    cvgs_box_select_desc s2 = select_desc(0);
    s2.classes = nullptr; s2.class_stride = 7; // class-agnostic: the stride is not carried
    EXPECT(cvgs_boxes_select(&s2, 1, nullptr) == CVGS_OK && g_select[0].classes == nullptr && g_select[0].class_stride == 0);

    const int classes[] = {1, 4, 5, 64, 65}, groups[] = {4, 4, 8, 64, 64};
    for (int i = 0; i < 5; ++i) {
        const cvgs_head_desc h = head_desc(classes[i], 1, 0);
        EXPECT(cvgs_head_decode(&h, 1, nullptr) == CVGS_OK && g_head.size() == 1 && g_head[0].group == groups[i] && g_head[0].num_classes == classes[i]);
    }
    cvgs_head_desc h = head_desc(80, 2, 0);
    h.cand_stride = 200;
    EXPECT(cvgs_head_decode(&h, 1, nullptr) == CVGS_OK && g_head[0].group == 0 && g_head[0].attr_stride == 2 && g_head[0].cand_stride == 200);
    const HeadFrame& hf = g_head[0];
    EXPECT(hf.head == h.head && (void*)hf.scratch == h.scratch && hf.boxes_out == h.boxes_out && hf.scores_out == h.scores_out && hf.classes_out == h.classes_out);
    EXPECT(hf.index_out == h.index_out && hf.count_out == h.count_out && hf.elem == CVGS_HEAD_BF16 && hf.n == 8400);
    EXPECT(hf.box_attr == 0 && hf.obj_attr == -1 && hf.class_attr == 4 && hf.num_classes == 80 && hf.score_thr == 0.25f);

    const cvgs_point_gather_desc g = gather_desc(0);
    EXPECT(cvgs_points_gather(&g, 1, nullptr) == CVGS_OK && g_gather.size() == 1);
    const GatherFrame& gf = g_gather[0];
    EXPECT(gf.head == g.head && gf.kept_index == g.kept_index && gf.kept_count == g.kept_count && gf.cand_index == g.cand_index);
    EXPECT(gf.points_out == g.points_out && gf.conf_out == g.conf_out && gf.source_out == g.source_out && gf.elem == CVGS_HEAD_BF16 && gf.max_cand == 8400);
    EXPECT(gf.cand_stride == 1 && gf.attr_stride == 8400 && gf.point_attr == 5 && gf.point_step == 3 && gf.n_points == 5 && gf.conf_offset == 2 && gf.max_out == 50 && gf.pad == 0);
    EXPECT(gf.xf[0] == 3.0f && gf.xf[1] == 1.6875f && gf.xf[2] == 0.0f && gf.xf[3] == -20.0f);

    // a launcher's error becomes the stage's "kernel launch" failure
    const cvgs_head_desc three[3] = {head_desc(80, 1, 0), head_desc(80, 1, 1), head_desc(80, 1, 2)};
    EXPECT(cvgs_head_decode(three, 3, nullptr) == CVGS_ERR_HIP && g_text == "head_decode: kernel launch: hip error 719");
}

// ---- (2) the collector at its full capacity -------------------------------------------------------------------------------------------
void full_capacity() {
    cvgs_head_desc h[16];
    for (int k = 0; k < 16; ++k) h[k] = head_desc(80, 1, k); // 16 x 6 ranges
    EXPECT(cvgs_head_decode(h, 16, nullptr) == CVGS_OK && g_head.size() == 16);
    h[15].index_out = (int32_t*)h[0].scratch;
    EXPECT(cvgs_head_decode(h, 16, nullptr) == CVGS_ERR_INVALID && g_text == "head_decode: the output and scratch buffers of one call overlap");
    cvgs_box_select_desc s[16];
    for (int k = 0; k < 16; ++k) s[k] = select_desc(k); // 16 x 5
    EXPECT(cvgs_boxes_select(s, 16, nullptr) == CVGS_OK && g_select.size() == 16);
    s[15].index_out = (int32_t*)s[0].scratch;
    EXPECT(cvgs_boxes_select(s, 16, nullptr) == CVGS_ERR_INVALID && g_text == "boxes_select: the output and scratch buffers of one call overlap");
    cvgs_point_gather_desc g[16];
    for (int k = 0; k < 16; ++k) g[k] = gather_desc(k); // 16 x 3
    EXPECT(cvgs_points_gather(g, 16, nullptr) == CVGS_OK && g_gather.size() == 16);
    g[15].source_out = (int32_t*)g[0].points_out;
    EXPECT(cvgs_points_gather(g, 16, nullptr) == CVGS_ERR_INVALID && g_text == "points_gather: the output buffers of one call overlap");
    cvgs_warp_table_desc w[16];
    for (int k = 0; k < 16; ++k) w[k] = warp_desc(k); // 16 x 2
    EXPECT(cvgs_warp_tables_from_points(w, 16, nullptr) == CVGS_OK && g_point.size() == 16);
    w[15].valid_out = (int32_t*)w[0].table_out;
    EXPECT(cvgs_warp_tables_from_points(w, 16, nullptr) == CVGS_ERR_INVALID && g_text == "warp_tables_from_points: the output buffers of one call overlap");
    // the boxes stage has no overlap test: frames sharing every buffer are launched
    std::vector<cvgs_box_table_desc> b((size_t)CVGS_MAX_CHAINS, box_desc());
    EXPECT(cvgs_plane_tables_from_boxes(b.data(), CVGS_MAX_CHAINS, nullptr) == CVGS_OK && g_box.size() == (size_t)CVGS_MAX_CHAINS);
}

// ---- (3) the host twins over buffers of exactly the contract's size ----------------------------------------------------------------------
// One line of the case file (tests/detect_refusal_cases.py: twin_line) per call:  stage int ... # input-hex ... # expected-output-hex ...
// ("-": a buffer that is not given).  Inputs and outputs live in heap blocks of exactly their size; the outputs must equal the expected
// bytes, which were recorded from the library of the commit that still had the twins in cvgs_api.cpp.
struct Block {
    std::unique_ptr<uint8_t[]> p;
    size_t n = 0;
    bool given = false;
    template <typename T> T* as() const { return given ? (T*)p.get() : nullptr; }
};
Block from_hex(const std::string& h) {
    Block b;
    if (h == "-") return b;
    b.given = true;
    b.n = h.size() / 2;
    b.p.reset(new uint8_t[b.n ? b.n : 1]);
    auto nib = [](char c) { return c <= '9' ? c - '0' : c - 'a' + 10; };
    for (size_t i = 0; i < b.n; ++i) b.p[i] = (uint8_t)(nib(h[2 * i]) * 16 + nib(h[2 * i + 1]));
    return b;
}
Block blank(size_t n, bool given = true) {
    Block b;
    b.given = given;
    b.n = given ? n : 0;
    b.p.reset(new uint8_t[n ? n : 1]);
    std::memset(b.p.get(), 0xa5, n);
    return b;
}
float bits(long long v) { const uint32_t u = (uint32_t)v; float f; std::memcpy(&f, &u, 4); return f; }
bool same(const Block& got, const Block& want) { return got.given == want.given && got.n == want.n && (!got.n || std::memcmp(got.p.get(), want.p.get(), got.n) == 0); }

void twin_case(const std::string& stage, const std::vector<long long>& v, const std::vector<Block>& in, const std::vector<Block>& want, int32_t* count_store) {
    const bool opt = true;
    if (stage == "select") { // n_cand pre_k max_out has_count count thr iou xform[4]
        cvgs_box_select_desc d = select_desc(0);
        d.frame_width = 640; d.frame_height = 480; d.max_candidates = (int)v[0]; d.pre_nms_k = (int)v[1]; d.max_out = (int)v[2];
        *count_store = (int32_t)v[4]; d.count = v[3] ? count_store : nullptr;
        d.score_threshold = bits(v[5]); d.iou_threshold = bits(v[6]);
        for (int k = 0; k < 4; ++k) d.xform[k] = bits(v[7 + k]);
        d.boxes = in[0].as<float>(); d.scores = in[1].as<float>(); d.classes = in[2].as<int32_t>();
        EXPECT(in[0].n == (size_t)v[0] * 16 && in[1].n == (size_t)v[0] * 4 && in[2].n == (size_t)v[0] * 4 && want.size() == 4);
        const size_t m = (size_t)v[2];
        Block bo = blank(m * 16), co = blank(4), so = blank(m * 4), io = blank(m * 4);
        EXPECT(cvgs_boxes_select_host(&d, bo.p.get(), co.as<int32_t>(), so.as<float>(), io.as<int32_t>()) == CVGS_OK);
        EXPECT(same(bo, want[0]) && same(co, want[1]) && same(so, want[2]) && same(io, want[3]));
        Block bo2 = blank(m * 16), co2 = blank(4); // without the optional outputs
        EXPECT(cvgs_boxes_select_host(&d, bo2.p.get(), co2.as<int32_t>(), nullptr, nullptr) == CVGS_OK && same(bo2, want[0]) && same(co2, want[1]));
    } else if (stage == "head") { // n elem cand_stride attr_stride box_attr obj_attr class_attr num_classes thr
        cvgs_head_desc d = head_desc((int)v[7], (int)v[3], 0);
        d.max_candidates = (int)v[0]; d.elem_type = (int)v[1]; d.cand_stride = (int)v[2]; d.box_attr = (int)v[4]; d.obj_attr = (int)v[5]; d.class_attr = (int)v[6];
        d.score_threshold = bits(v[8]);
        d.head = in[0].p.get();
        const size_t n = (size_t)v[0];
        EXPECT(in[0].n == n * 8 * (v[1] == CVGS_HEAD_F32 ? 4 : 2) && want.size() == 5);
        Block bo = blank(n * 16), so = blank(n * 4), ko = blank(n * 4), io = blank(n * 4), co = blank(4);
        EXPECT(cvgs_head_decode_host(&d, bo.as<float>(), so.as<float>(), ko.as<int32_t>(), io.as<int32_t>(), co.as<int32_t>()) == CVGS_OK);
        EXPECT(same(bo, want[0]) && same(so, want[1]) && same(ko, want[2]) && same(io, want[3]) && same(co, want[4]));
        Block bo2 = blank(n * 16), so2 = blank(n * 4), ko2 = blank(n * 4), co2 = blank(4); // without index_out
        EXPECT(cvgs_head_decode_host(&d, bo2.as<float>(), so2.as<float>(), ko2.as<int32_t>(), nullptr, co2.as<int32_t>()) == CVGS_OK);
        EXPECT(same(bo2, want[0]) && same(so2, want[1]) && same(ko2, want[2]) && same(co2, want[4]));
    } else if (stage == "gather") { // max_cand cand_stride attr_stride point_attr point_step n_points conf_offset max_out has_count kept_count xform[4]
        cvgs_point_gather_desc d = gather_desc(0);
        d.elem_type = CVGS_HEAD_F32; d.max_candidates = (int)v[0]; d.cand_stride = (int)v[1]; d.attr_stride = (int)v[2]; d.point_attr = (int)v[3];
        d.point_step = (int)v[4]; d.n_points = (int)v[5]; d.conf_offset = (int)v[6]; d.max_out = (int)v[7];
        *count_store = (int32_t)v[9]; d.kept_count = v[8] ? count_store : nullptr;
        for (int k = 0; k < 4; ++k) d.xform[k] = bits(v[10 + k]);
        d.head = in[0].p.get(); d.kept_index = in[1].as<int32_t>(); d.cand_index = in[2].as<int32_t>();
        const size_t items = (size_t)v[7] * (size_t)v[5];
        EXPECT(in[0].n == (size_t)v[0] * (size_t)v[1] * 4 && in[1].n == (size_t)v[7] * 4 && in[2].n == (size_t)v[0] * 4 && want.size() == 3);
        Block po = blank(items * 8), co = blank(items * 4, v[6] != -1), so = blank((size_t)v[7] * 4);
        EXPECT(cvgs_points_gather_host(&d, po.as<float>(), co.as<float>(), so.as<int32_t>()) == CVGS_OK);
        EXPECT(same(po, want[0]) && same(co, want[1]) && same(so, want[2]));
        Block po2 = blank(items * 8), co2 = blank(items * 4, v[6] != -1); // without source_out
        EXPECT(cvgs_points_gather_host(&d, po2.as<float>(), co2.as<float>(), nullptr) == CVGS_OK && same(po2, want[0]) && same(co2, want[1]));
    } else if (stage == "warp") { // fit n_points max_items has_count count; inputs: template, points
        cvgs_warp_table_desc d = warp_desc(0, (int)v[0]);
        d.n_points = (int)v[1]; d.max_items = (int)v[2];
        *count_store = (int32_t)v[4]; d.count = v[3] ? count_store : nullptr;
        EXPECT(in[0].n == (size_t)v[1] * 8 && in[1].n == (size_t)v[2] * (size_t)v[1] * 8 && want.size() == 2);
        std::memcpy(d.tmpl, in[0].p.get(), in[0].n);
        d.points = in[1].as<float>();
        Block table = blank(cvgs_warp_table_bytes((int32_t)v[2])), valid = blank((size_t)v[2] * 4);
        d.valid_out = valid.as<int32_t>();
        EXPECT(cvgs_warp_table_build_host(&d, table.p.get()) == CVGS_OK && same(table, want[0]) && same(valid, want[1]));
        Block table2 = blank(table.n); // without valid_out
        d.valid_out = nullptr;
        EXPECT(cvgs_warp_table_build_host(&d, table2.p.get()) == CVGS_OK && same(table2, want[0]));
    } else {
        EXPECT(!opt);
    }
}

void host_twins(const char* path) {
    std::FILE* f = std::fopen(path, "r");
    EXPECT(f != nullptr);
    if (!f) return;
    std::string text;
    char chunk[65536];
    for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, f)) > 0;) text.append(chunk, n);
    std::fclose(f);
    int lines = 0;
    for (size_t at = 0; at < text.size();) {
        const size_t end = text.find('\n', at);
        const std::string line = text.substr(at, end == std::string::npos ? std::string::npos : end - at);
        at = end == std::string::npos ? text.size() : end + 1;
        if (line.empty()) continue;
        std::string stage;
        std::vector<long long> v;
        std::vector<Block> bufs[2];
        int part = 0;
        for (size_t i = 0; i < line.size();) {
            const size_t sp = line.find(' ', i);
            const std::string tok = line.substr(i, sp == std::string::npos ? std::string::npos : sp - i);
            i = sp == std::string::npos ? line.size() : sp + 1;
            if (tok == "#") ++part;
            else if (part == 0 && stage.empty()) stage = tok;
            else if (part == 0) v.push_back(std::atoll(tok.c_str()));
            else if (part < 3) bufs[part - 1].push_back(from_hex(tok));
        }
        std::unique_ptr<int32_t> count(new int32_t(0)); // the live count, on the heap like everything a twin reads
        twin_case(stage, v, bufs[0], bufs[1], count.get());
        ++lines;
    }
    EXPECT(lines >= 40);
}
} // namespace

int main(int argc, char** argv) {
    frames_field_by_field();
    full_capacity();
    if (argc > 1) host_twins(argv[1]); // (without a case file: parts 1 and 2 only)
    std::printf("%d checks, %d bad\n", checks, bad);
    return bad ? 1 : 0;
}
