// test_warp_tick.cpp -- cvGS::DeviceWarps + cvGS::ChainBatch: the aligned crops of three cameras in ONE launch (the warp tick of
// cvgs_execute_many).  Three DeviceWarps are fitted to device-side landmarks; the ChainBatch over them is captured (one kernel node, a
// "tick: ..." note) and executed, and its tensors equal those of one executeOperations per camera bit for bit.
#include "common.h"

namespace {

constexpr int CAMS = 3, N = 6, K = 5, W = 97, H = 61;
const cv::Size DS(16, 8);
constexpr int kPlane = 16 * 8;
const std::vector<cv::Point2f> kTmpl = {{4.f, 2.f}, {11.f, 2.f}, {7.5f, 4.f}, {5.f, 6.f}, {10.f, 6.f}};

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

} // namespace

int main() {
    cv::cuda::Stream stream;
    const size_t bytes = (size_t)N * 3 * kPlane * sizeof(float);
    std::vector<cv::cuda::GpuMat> frames(CAMS), outs, wants;
    std::vector<std::unique_ptr<cvGS::DeviceWarps>> warps;
    std::vector<float*> d_pts(CAMS, nullptr);
    int32_t* d_count = nullptr;
    HIP_OK(hipMalloc((void**)&d_count, CAMS * sizeof(int32_t)));
    const int32_t counts[CAMS] = {N, N - 1, N + 3};
    HIP_OK(hipMemcpy(d_count, counts, sizeof(counts), hipMemcpyHostToDevice));
    for (int c = 0; c < CAMS; ++c) {
        cv::Mat h_frame(H, W, CV_8UC3);
        fill_random(h_frame, 0xFACE + (unsigned)c);
        frames[(size_t)c].upload(h_frame);
        // item i: the template scaled, rotated and moved (some partly or wholly outside the frame); camera 1 holds a NaN item
        std::vector<float> pts((size_t)N * K * 2);
        for (int i = 0; i < N; ++i) {
            const double ang = 0.5235987755982988 * (i + 2 * c), sc = 0.6 + 0.5 * i + 0.2 * c, cx = -10.0 + 21.0 * i + 3.0 * c, cy = 5.0 + 10.0 * i;
            for (int j = 0; j < K; ++j) {
                const double x = kTmpl[(size_t)j].x - 7.5, y = kTmpl[(size_t)j].y - 4.0;
                pts[((size_t)i * K + j) * 2] = (float)(cx + sc * (std::cos(ang) * x - std::sin(ang) * y));
                pts[((size_t)i * K + j) * 2 + 1] = (float)(cy + sc * (std::sin(ang) * x + std::cos(ang) * y));
            }
        }
        if (c == 1) pts[(size_t)2 * K * 2 + 3] = std::nanf("");
        HIP_OK(hipMalloc((void**)&d_pts[(size_t)c], pts.size() * sizeof(float)));
        HIP_OK(hipMemcpy(d_pts[(size_t)c], pts.data(), pts.size() * sizeof(float), hipMemcpyHostToDevice));
        warps.emplace_back(new cvGS::DeviceWarps(N));
        warps.back()->update(stream, frames[(size_t)c], d_pts[(size_t)c], d_count + c, CVGS_WARP_FIT_SIMILARITY, kTmpl, DS);
        outs.emplace_back(N, 3 * kPlane, CV_32FC1);
        wants.emplace_back(N, 3 * kPlane, CV_32FC1);
        HIP_OK(hipMemset(outs.back().data, 0xff, bytes));
        HIP_OK(hipMemset(wants.back().data, 0xee, bytes));
    }
    // one executeOperations per camera: what the tick must equal
    for (int c = 0; c < CAMS; ++c) run_chain(stream, cvGS::warp<fk::WarpType::Affine, CV_8UC3>(*warps[(size_t)c]), wants[(size_t)c]);
    stream.waitForCompletion();

    // the ChainBatch captured: ONE kernel node, and the call's note says "tick: ..."
    {
        cvGS::ChainBatch tick;
        for (int c = 0; c < CAMS; ++c) add_chain(tick, *warps[(size_t)c], outs[(size_t)c]);
        hipStream_t raw = cv::cuda::StreamAccessor::getStream(stream);
        hipGraph_t graph = nullptr;
        HIP_OK(hipStreamBeginCapture(raw, hipStreamCaptureModeGlobal));
        tick.execute(stream);
        const std::string note = cvgs_last_error();
        HIP_OK(hipStreamEndCapture(raw, &graph));
        size_t nodes = 0;
        HIP_OK(hipGraphGetNodes(graph, nullptr, &nodes));
        HIP_OK(hipGraphDestroy(graph));
        CHECK(nodes == 1, "a ChainBatch of three DeviceWarps chains is ONE kernel node (got " << nodes << ", note: " << note << ")");
        CHECK(note.rfind("tick:", 0) == 0, "the call's note says tick (got: " << note << ")");
    }
    // ... and executed: the bytes of one executeOperations per camera
    {
        cvGS::ChainBatch tick;
        for (int c = 0; c < CAMS; ++c) add_chain(tick, *warps[(size_t)c], outs[(size_t)c]);
        tick.execute(stream);
        stream.waitForCompletion();
        for (int c = 0; c < CAMS; ++c)
            CHECK(bit_equal(fetch(outs[(size_t)c].data, bytes).data(), fetch(wants[(size_t)c].data, bytes).data(), bytes), "ChainBatch tick, camera " << c);
    }
    CHECK(!bit_equal(fetch(outs[0].data, bytes).data(), fetch(outs[1].data, bytes).data(), bytes), "the cameras differ");
    for (int c = 0; c < CAMS; ++c) HIP_OK(hipFree(d_pts[(size_t)c]));
    HIP_OK(hipFree(d_count));
    return report("test_warp_tick");
}
