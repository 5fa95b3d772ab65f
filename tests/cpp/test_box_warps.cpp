// test_box_warps.cpp -- cvGS::DeviceWarps::updateFromBoxes: context crops from device-side boxes (cvgs_warp_tables_from_boxes) on the facade.
// The boxes of three cameras reach the device once; updateFromBoxes shapes them there (context factor, the target's aspect ratio, no
// clamp) and warp<WT, T>(warps) reads the device table.  Checked: the table, boxesOut and valid() against cvgs_warp_table_from_boxes_host
// byte for byte; executeOperations over the table against the host-described warp (fk::WarpRead) with the table's own floats, bit for bit;
// a ChainBatch over the three cameras against one executeOperations per camera, bit for bit.
#include "common.h"

namespace {

constexpr int CAMS = 3, N = 7, W = 97, H = 61;
const cv::Size DS(12, 16);
constexpr int kPlane = 12 * 16;

template <typename Read>
void run_chain(const cv::cuda::Stream& s, const Read& rd, cv::cuda::GpuMat& out) {
    cvGS::executeOperations(s, rd, cvGS::cvtColor<cv::COLOR_RGB2BGR, CV_32FC3>(), cvGS::multiply<CV_32FC3>(cv::Scalar(0.3, 0.3, 0.3)),
                            cvGS::subtract<CV_32FC3>(cv::Scalar(1.0, 4.0, 3.2)), cvGS::divide<CV_32FC3>(cv::Scalar(3.2, 0.6, 11.8)),
                            cvGS::split<CV_32FC3>(out, DS));
}

void add_chain(cvGS::ChainBatch& tick, const cvGS::DeviceWarps& warps, cv::cuda::GpuMat& out) {
    tick.add(cvGS::warp<fk::WarpType::Affine, CV_8UC3>(warps), cvGS::cvtColor<cv::COLOR_RGB2BGR, CV_32FC3>(), cvGS::multiply<CV_32FC3>(cv::Scalar(0.3, 0.3, 0.3)),
             cvGS::subtract<CV_32FC3>(cv::Scalar(1.0, 4.0, 3.2)), cvGS::divide<CV_32FC3>(cv::Scalar(3.2, 0.6, 11.8)), cvGS::split<CV_32FC3>(out, DS));
}

struct Entry { // one 64-byte table entry
    const void* data;
    int32_t w, h, step;
    float m[9];
    int32_t dw, dh;
};
static_assert(sizeof(Entry) == 64, "warp table entry");

} // namespace

int main() {
    cv::cuda::Stream stream;
    const size_t bytes = (size_t)N * 3 * kPlane * sizeof(float);
    std::vector<cv::cuda::GpuMat> frames(CAMS), outs, wants, ticks;
    std::vector<std::unique_ptr<cvGS::DeviceWarps>> warps;
    std::vector<float*> d_boxes(CAMS, nullptr), d_shaped(CAMS, nullptr);
    int32_t* d_count = nullptr;
    HIP_OK(hipMalloc((void**)&d_count, CAMS * sizeof(int32_t)));
    const int32_t counts[CAMS] = {N, N - 1, N + 3};
    HIP_OK(hipMemcpy(d_count, counts, sizeof(counts), hipMemcpyHostToDevice));
    const cv::Point2f scale(1.25f, 1.25f), pad(0.f, 2.5f);
    for (int c = 0; c < CAMS; ++c) {
        cv::Mat h_frame(H, W, CV_8UC3);
        fill_random(h_frame, 0xB0C5 + (unsigned)c);
        frames[(size_t)c].upload(h_frame);
        // inside, across the left / top edge, across the right / bottom edge, larger than the frame, wholly outside, inverted, a NaN
        std::vector<float> boxes = {20.f + c, 10.f, 50.f, 45.f + c,   -8.f, -6.f + c, 14.5f, 20.f,   80.f, 40.5f, 110.f + c, 75.f,   -20.f, -20.f, 120.f, 90.f + c,
                                    130.f, 10.f, 160.f, 40.f,   50.f, 30.f, 40.f, 50.f,   10.f, std::nanf(""), 30.f, 40.f};
        HIP_OK(hipMalloc((void**)&d_boxes[(size_t)c], boxes.size() * sizeof(float)));
        HIP_OK(hipMalloc((void**)&d_shaped[(size_t)c], boxes.size() * sizeof(float)));
        HIP_OK(hipMemcpy(d_boxes[(size_t)c], boxes.data(), boxes.size() * sizeof(float), hipMemcpyHostToDevice));
        warps.emplace_back(new cvGS::DeviceWarps(N));
        warps.back()->updateFromBoxes(stream, frames[(size_t)c], d_boxes[(size_t)c], d_count + c, DS, CVGS_BOX_SHAPE_EXPAND, scale, pad, d_shaped[(size_t)c]);
        for (auto* v : {&outs, &wants, &ticks}) {
            v->emplace_back(N, 3 * kPlane, CV_32FC1);
            HIP_OK(hipMemset(v->back().data, 0xff, bytes));
        }
        run_chain(stream, cvGS::warp<fk::WarpType::Affine, CV_8UC3>(*warps.back()), outs.back());
        stream.waitForCompletion();

        // the host twin: the same descriptor over host boxes and a host count
        cvgs_box_warp_desc d;
        std::memset(&d, 0, sizeof(d));
        d.struct_size = sizeof(d);
        d.frame = cvgs_image2d{frames[(size_t)c].data, W, H, (int32_t)frames[(size_t)c].step, 0};
        d.src_type = CV_8UC3; d.read_kind = CVGS_READ_WARP_AFFINE;
        d.dst_width = DS.width; d.dst_height = DS.height;
        d.shape = CVGS_BOX_SHAPE_EXPAND; d.max_items = N;
        d.scale[0] = scale.x; d.scale[1] = scale.y; d.pad[0] = pad.x; d.pad[1] = pad.y;
        d.boxes = boxes.data(); d.count = &counts[c];
        std::vector<uint8_t> h_tab((size_t)N * sizeof(Entry));
        std::vector<float> h_shaped((size_t)N * 4);
        std::vector<int32_t> h_valid((size_t)N);
        CHECK(cvgs_warp_table_from_boxes_host(&d, h_tab.data(), h_shaped.data(), h_valid.data()) == CVGS_OK, "the host twin accepts the descriptor: " << cvgs_last_error());
        const std::vector<uint8_t> tab = fetch(warps.back()->table(), h_tab.size());
        CHECK(bit_equal(tab.data(), h_tab.data(), h_tab.size()), "camera " << c << ": the device table == the host twin's");
        CHECK(bit_equal(fetch(d_shaped[(size_t)c], (size_t)N * 16).data(), h_shaped.data(), (size_t)N * 16), "camera " << c << ": boxesOut == the host twin's");
        CHECK(bit_equal(fetch(warps.back()->valid(), (size_t)N * 4).data(), h_valid.data(), (size_t)N * 4), "camera " << c << ": valid() == the host twin's");
        const int live = counts[c] < N ? counts[c] : N;
        for (int i = 0; i < N; ++i) CHECK(h_valid[(size_t)i] == (i < 5 && i < live ? 1 : 0), "camera " << c << ": validity of item " << i);
        CHECK(h_shaped[0] < 20.f + c && h_shaped[2] > 50.f && h_shaped[4] < -8.f && h_shaped[14] > 90.f + c, "camera " << c << ": the shaped boxes grew and are not clamped");

        // the host-described warp with the table's own floats
        fk::WarpRead<fk::WarpType::Affine, CUDA_T(CV_8UC3)> host_rd;
        host_rd.planes.resize(N, cvgs_image2d{frames[(size_t)c].data, W, H, (int32_t)frames[(size_t)c].step, 0});
        host_rd.params.resize(N);
        host_rd.used = N;
        for (int i = 0; i < N; ++i) {
            Entry e;
            std::memcpy(&e, tab.data() + (size_t)i * sizeof(Entry), sizeof(Entry));
            for (int y = 0; y < 3; ++y)
                for (int x = 0; x < 3; ++x) host_rd.params[(size_t)i].transformMatrix[y][x] = e.m[3 * y + x];
            host_rd.params[(size_t)i].dstSize = fk::Size(DS.width, DS.height);
        }
        run_chain(stream, host_rd, wants.back());
        stream.waitForCompletion();
        CHECK(bit_equal(fetch(outs.back().data, bytes).data(), fetch(wants.back().data, bytes).data(), bytes), "camera " << c << ": executeOperations over updateFromBoxes == host-described warps");
    }

    // a ChainBatch over the three cameras: the bytes of one executeOperations per camera
    cvGS::ChainBatch tick;
    for (int c = 0; c < CAMS; ++c) add_chain(tick, *warps[(size_t)c], ticks[(size_t)c]);
    tick.execute(stream);
    const std::string note = cvgs_last_error();
    stream.waitForCompletion();
    CHECK(note.rfind("tick:", 0) == 0, "the ChainBatch ran as a tick (got: " << note << ")");
    for (int c = 0; c < CAMS; ++c)
        CHECK(bit_equal(fetch(ticks[(size_t)c].data, bytes).data(), fetch(outs[(size_t)c].data, bytes).data(), bytes), "ChainBatch tick, camera " << c);
    CHECK(!bit_equal(fetch(outs[0].data, bytes).data(), fetch(outs[1].data, bytes).data(), bytes), "the cameras differ");

    // recorded ticks: one executeOperations per camera on a recording stream
    for (int c = 0; c < CAMS; ++c) HIP_OK(hipMemset(ticks[(size_t)c].data, 0xff, bytes));
    cvGS::recordTicks(stream, CAMS);
    for (int c = 0; c < CAMS; ++c) run_chain(stream, cvGS::warp<fk::WarpType::Affine, CV_8UC3>(*warps[(size_t)c]), ticks[(size_t)c]);
    cvGS::stopRecording(stream);
    stream.waitForCompletion();
    for (int c = 0; c < CAMS; ++c)
        CHECK(bit_equal(fetch(ticks[(size_t)c].data, bytes).data(), fetch(outs[(size_t)c].data, bytes).data(), bytes), "recorded tick, camera " << c);

    for (int c = 0; c < CAMS; ++c) { HIP_OK(hipFree(d_boxes[(size_t)c])); HIP_OK(hipFree(d_shaped[(size_t)c])); }
    HIP_OK(hipFree(d_count));
    return report("test_box_warps");
}
