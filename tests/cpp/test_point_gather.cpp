// test_point_gather.cpp -- cvGS::DevicePointGather: a detector's raw head -> aligned crops without the host in the loop, on the facade.
// DeviceHeadDecode -> DeviceBoxSelect -> DevicePointGather -> DeviceWarps::update -> executeOperations(warp(...)) over an fp32
// [N, 4 + 1 + 2 * 5] head whose landmarks sit around each box.  Checked against the four HOST entries (cvgs_head_decode_host,
// cvgs_boxes_select_host, cvgs_points_gather_host, cvgs_warp_table_build_host): the device's points, sources and table equal theirs byte for
// byte, and the tensor equals the host-described warp whose matrices are the nine floats of each host-built table entry.
#include "common.h"

namespace {

constexpr int N = 300, K = 5, A = 4 + 1 + 2 * K, MAX_OUT = 8, W = 96, H = 64;
const cv::Size DS(32, 32);
constexpr int kPlane = 32 * 32;
const std::vector<cv::Point2f> kTmpl = {{10.9f, 14.8f}, {21.0f, 14.7f}, {16.0f, 20.5f}, {11.9f, 26.4f}, {20.2f, 26.3f}};

struct Entry { // one 64-byte table entry
    const void* data;
    int32_t w, h, step;
    float m[9];
    int32_t dw, dh;
};
static_assert(sizeof(Entry) == 64, "warp table entry");

template <typename Read>
void run_chain(const cv::cuda::Stream& s, const Read& rd, cv::cuda::GpuMat& out) {
    cvGS::executeOperations(s, rd, cvGS::cvtColor<cv::COLOR_RGB2BGR, CV_32FC3>(), cvGS::multiply<CV_32FC3>(cv::Scalar(0.3, 0.3, 0.3)),
                            cvGS::subtract<CV_32FC3>(cv::Scalar(1.0, 4.0, 3.2)), cvGS::divide<CV_32FC3>(cv::Scalar(3.2, 0.6, 11.8)),
                            cvGS::split<CV_32FC3>(out, DS));
}

uint32_t next(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
float unit(uint32_t& s) { return (float)(next(s) >> 8) / 16777216.0f; }

} // namespace

int main() {
    cv::cuda::Stream stream;
    cv::Mat h_frame(H, W, CV_8UC3);
    fill_random(h_frame, 0xFACE5);
    cv::cuda::GpuMat frame;
    frame.upload(h_frame);

    // the head in the coordinates of a 160 x 160 detector input: a tenth of the candidates over the threshold
    std::vector<float> head((size_t)N * A);
    uint32_t seed = 12345u;
    for (int i = 0; i < N; ++i) {
        float* c = &head[(size_t)i * A];
        c[0] = 160.f * unit(seed); c[1] = 160.f * unit(seed);
        c[2] = 8.f + 40.f * unit(seed); c[3] = 8.f + 40.f * unit(seed);
        c[4] = (i % 10 == 3) ? 0.5f + 0.4f * unit(seed) : 0.1f * unit(seed);
        for (int p = 0; p < K; ++p) {
            c[5 + 2 * p] = c[0] + (kTmpl[(size_t)p].x / 32.f - 0.5f) * c[2] + unit(seed);
            c[6 + 2 * p] = c[1] + (kTmpl[(size_t)p].y / 32.f - 0.5f) * c[3] + unit(seed);
        }
    }
    float* d_head = nullptr;
    HIP_OK(hipMalloc((void**)&d_head, head.size() * sizeof(float)));
    HIP_OK(hipMemcpy(d_head, head.data(), head.size() * sizeof(float), hipMemcpyHostToDevice));
    const float sx = (float)W / 160.f, sy = (float)H / 160.f, ox = 0.5f * sx - 0.5f, oy = 0.5f * sy - 0.5f; // (pixel-centre landmarks)

    cvGS::DeviceHeadDecode decode(N);
    decode.layout(d_head, CVGS_HEAD_F32, A, 1, 1).threshold(0.25f);
    cvGS::DeviceBoxSelect select(cv::Size(W, H), N, 256, MAX_OUT);
    select.thresholds(0.25f, 0.5f).transform(sx, sy, 0.f, 0.f);
    decode.feed(select, CVGS_CAND_CXCYWH_F32);
    cvGS::DevicePointGather gather(N, MAX_OUT, K, false, true);
    gather.layout(d_head, CVGS_HEAD_F32, A, 1, 5, 2).transform(sx, sy, ox, oy).from(select, decode);
    cvGS::DeviceWarps faces(MAX_OUT);
    decode.enqueue(stream);
    select.enqueue(stream);
    gather.enqueue(stream);
    faces.update(stream, frame, gather.points(), gather.count(), CVGS_WARP_FIT_SIMILARITY, kTmpl, DS);
    const size_t bytes = (size_t)MAX_OUT * 3 * kPlane * sizeof(float);
    cv::cuda::GpuMat out(MAX_OUT, 3 * kPlane, CV_32FC1), want(MAX_OUT, 3 * kPlane, CV_32FC1);
    HIP_OK(hipMemset(out.data, 0xff, bytes));
    run_chain(stream, cvGS::warp<fk::WarpType::Affine, CV_8UC3>(faces), out);
    stream.waitForCompletion();

    // the four host entries
    std::vector<float> h_boxes((size_t)N * 4), h_scores((size_t)N);
    std::vector<int32_t> h_classes((size_t)N), h_index((size_t)N);
    int32_t h_count = -1;
    cvgs_head_desc hd = decode.desc();
    hd.head = head.data();
    CHECK(cvgs_head_decode_host(&hd, h_boxes.data(), h_scores.data(), h_classes.data(), h_index.data(), &h_count) == CVGS_OK, "cvgs_head_decode_host");
    cvgs_box_select_desc sd = select.desc();
    sd.boxes = h_boxes.data(); sd.scores = h_scores.data(); sd.classes = h_classes.data(); sd.count = &h_count;
    std::vector<float> k_boxes((size_t)MAX_OUT * 4), k_scores((size_t)MAX_OUT);
    std::vector<int32_t> k_index((size_t)MAX_OUT);
    int32_t kept = -1;
    CHECK(cvgs_boxes_select_host(&sd, k_boxes.data(), &kept, k_scores.data(), k_index.data()) == CVGS_OK, "cvgs_boxes_select_host");
    CHECK(kept >= 3 && kept <= MAX_OUT, "between 3 and " << MAX_OUT << " detections are kept: " << kept);
    cvgs_point_gather_desc gd = gather.desc();
    gd.head = head.data(); gd.kept_index = k_index.data(); gd.kept_count = &kept; gd.cand_index = h_index.data();
    std::vector<float> h_points((size_t)MAX_OUT * K * 2);
    std::vector<int32_t> h_source((size_t)MAX_OUT);
    CHECK(cvgs_points_gather_host(&gd, h_points.data(), nullptr, h_source.data()) == CVGS_OK, "cvgs_points_gather_host: " << cvgs_last_error());
    CHECK(bit_equal(fetch(gather.points(), h_points.size() * sizeof(float)).data(), h_points.data(), h_points.size() * sizeof(float)),
          "the device's points equal the host entry's");
    CHECK(bit_equal(fetch(gather.source(), h_source.size() * 4).data(), h_source.data(), h_source.size() * 4), "the device's sources equal the host entry's");
    for (int j = 0; j < MAX_OUT; ++j) CHECK((h_source[(size_t)j] >= 0) == (j < kept) && (j >= kept || h_source[(size_t)j] % 10 == 3), "row " << j << " comes from a hot candidate");

    cvgs_warp_table_desc wd;
    std::memset(&wd, 0, sizeof(wd));
    wd.struct_size = sizeof(wd);
    wd.frame = cvgs_image2d{frame.data, frame.cols, frame.rows, (int32_t)frame.step, 0};
    wd.src_type = frame.type();
    wd.read_kind = CVGS_READ_WARP_AFFINE;
    wd.dst_width = DS.width; wd.dst_height = DS.height;
    wd.fit = CVGS_WARP_FIT_SIMILARITY; wd.n_points = K;
    for (int p = 0; p < K; ++p) { wd.tmpl[p][0] = kTmpl[(size_t)p].x; wd.tmpl[p][1] = kTmpl[(size_t)p].y; }
    wd.max_items = MAX_OUT;
    wd.points = h_points.data(); wd.count = &kept;
    std::vector<uint8_t> h_table((size_t)MAX_OUT * sizeof(Entry));
    CHECK(cvgs_warp_table_build_host(&wd, h_table.data()) == CVGS_OK, "cvgs_warp_table_build_host");
    CHECK(bit_equal(fetch(faces.table(), h_table.size()).data(), h_table.data(), h_table.size()), "the device's warp table equals the host-built one");

    fk::WarpRead<fk::WarpType::Affine, CUDA_T(CV_8UC3)> host_rd;
    host_rd.planes.resize(MAX_OUT, cvgs_image2d{frame.data, frame.cols, frame.rows, (int32_t)frame.step, 0});
    host_rd.params.resize(MAX_OUT);
    host_rd.used = MAX_OUT;
    for (int i = 0; i < MAX_OUT; ++i) {
        Entry e;
        std::memcpy(&e, h_table.data() + (size_t)i * sizeof(Entry), sizeof(Entry));
        for (int y = 0; y < 3; ++y)
            for (int x = 0; x < 3; ++x) host_rd.params[(size_t)i].transformMatrix[y][x] = e.m[3 * y + x];
        host_rd.params[(size_t)i].dstSize = fk::Size(DS.width, DS.height);
    }
    run_chain(stream, host_rd, want);
    stream.waitForCompletion();
    CHECK(bit_equal(fetch(out.data, bytes).data(), fetch(want.data, bytes).data(), bytes), "head -> aligned crops on the device == the host entries' warps");

    // from() refuses a selector of another size
    cvGS::DeviceBoxSelect other(cv::Size(W, H), N, 256, MAX_OUT - 1);
    bool threw = false;
    try { gather.from(other); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw, "from(selector of another maxOut) throws");
    HIP_OK(hipFree(d_head));
    return report("test_point_gather");
}
