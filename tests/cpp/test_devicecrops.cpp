// test_devicecrops.cpp -- cvGS::DeviceCrops: crops from device-side boxes (cvgs_plane_tables_from_boxes) on the facade.
// The boxes reach the device once; DeviceCrops::update builds the plane table there and resize<T, INTER_LINEAR, AR>(crops, bg) reads it --
// through executeOperations, through a ChainBatch tick of two cameras (one builder launch for both), and on a stream that records ticks.
// Checked against the same chains over host-described crops (cvGS::crop of the clamped rectangles), bit for bit; invalid boxes against a
// batch with usedPlanes = 0.
#include "common.h"

namespace {

constexpr int N = 12, W = 97, H = 61;
const cv::Size DS(16, 8);
constexpr int kPlane = 16 * 8;
// (x, y, w, h): inside, clipped at each edge, empty, outside
const int32_t kBoxes[N][4] = {{5, 5, 40, 30}, {0, 0, 97, 61}, {90, 50, 30, 30}, {-10, -10, 30, 30}, {50, 20, 0, 10}, {96, 60, 1, 1},
                              {97, 10, 5, 5}, {10, 10, 3, 2}, {20, 61, 5, 5}, {30, 30, 20, 25}, {-50, 5, 20, 20}, {60, 0, 37, 61}};

bool clamp_box(const int32_t* b, cv::Rect& r) {
    if (b[2] <= 0 || b[3] <= 0) return false;
    const int64_t l = std::min<int64_t>(std::max<int64_t>(b[0], 0), W), rr = std::min<int64_t>(std::max<int64_t>((int64_t)b[0] + b[2], 0), W);
    const int64_t t = std::min<int64_t>(std::max<int64_t>(b[1], 0), H), bb = std::min<int64_t>(std::max<int64_t>((int64_t)b[1] + b[3], 0), H);
    if (rr <= l || bb <= t) return false;
    r = cv::Rect((int)l, (int)t, (int)(rr - l), (int)(bb - t));
    return true;
}

template <typename Read>
void run_chain(const cv::cuda::Stream& s, const Read& rd, cv::cuda::GpuMat& out) {
    cvGS::executeOperations(s, rd, cvGS::cvtColor<cv::COLOR_RGB2BGR, CV_32FC3>(), cvGS::multiply<CV_32FC3>(cv::Scalar(0.3, 0.3, 0.3)),
                            cvGS::subtract<CV_32FC3>(cv::Scalar(1.0, 4.0, 3.2)), cvGS::divide<CV_32FC3>(cv::Scalar(3.2, 0.6, 11.8)),
                            cvGS::split<CV_32FC3>(out, DS));
}

// the host-described result: valid boxes as crops, invalid ones as default planes
std::vector<uint8_t> host_described(cv::cuda::Stream& s, const cv::cuda::GpuMat& frame, int count, const cv::Scalar& bg) {
    const size_t plane = (size_t)3 * kPlane * sizeof(float);
    std::vector<uint8_t> want((size_t)N * plane);
    for (int i = 0; i < N; ++i) {
        cv::Rect r;
        const bool ok = i < count && clamp_box(kBoxes[i], r);
        std::array<cv::cuda::GpuMat, 1> one{ok ? frame(r) : frame};
        cv::cuda::GpuMat out(1, 3 * kPlane, CV_32FC1);
        run_chain(s, cvGS::resize<CV_8UC3, cv::INTER_LINEAR, 1, cvGS::PRESERVE_AR>(one, DS, ok ? 1 : 0, bg), out);
        s.waitForCompletion();
        const std::vector<uint8_t> h = fetch(out.data, plane);
        std::memcpy(want.data() + (size_t)i * plane, h.data(), plane);
    }
    return want;
}

} // namespace

int main() {
    cv::cuda::Stream stream;
    const cv::Scalar bg(10.0, 20.0, 30.0);
    const size_t bytes = (size_t)N * 3 * kPlane * sizeof(float);
    cv::Mat h_a(H, W, CV_8UC3), h_b(H, W, CV_8UC3);
    fill_random(h_a, 0xC0FFEE);
    fill_random(h_b, 0xC0FFEF);
    cv::cuda::GpuMat frame_a, frame_b;
    frame_a.upload(h_a);
    frame_b.upload(h_b);
    void* d_boxes = nullptr;
    int32_t* d_count = nullptr;
    HIP_OK(hipMalloc(&d_boxes, sizeof(kBoxes)));
    HIP_OK(hipMalloc((void**)&d_count, 2 * sizeof(int32_t)));
    const int32_t counts[2] = {N - 2, N + 7};
    HIP_OK(hipMemcpy(d_boxes, kBoxes, sizeof(kBoxes), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_count, counts, sizeof(counts), hipMemcpyHostToDevice));

    // one camera: update, then the read like any other batched resize
    cvGS::DeviceCrops crops_a(N), crops_b(N);
    crops_a.update(stream, frame_a, d_boxes, d_count, CVGS_BOX_XYWH_I32, DS, cvGS::PRESERVE_AR);
    cv::cuda::GpuMat out_a(N, 3 * kPlane, CV_32FC1), out_b(N, 3 * kPlane, CV_32FC1);
    run_chain(stream, cvGS::resize<CV_8UC3, cv::INTER_LINEAR, cvGS::PRESERVE_AR>(crops_a, bg), out_a);
    stream.waitForCompletion();
    const std::vector<uint8_t> want_a = host_described(stream, frame_a, counts[0], bg), want_b = host_described(stream, frame_b, N, bg);
    CHECK(bit_equal(fetch(out_a.data, bytes).data(), want_a.data(), bytes), "executeOperations over DeviceCrops == host-described crops");
    // rects(): (x, y, w, h) of the clamped box, zeros for an invalid one
    const std::vector<uint8_t> rects = fetch(crops_a.rects(), (size_t)N * 16);
    for (int i = 0; i < N; ++i) {
        cv::Rect r;
        const bool ok = i < counts[0] && clamp_box(kBoxes[i], r);
        const int32_t want[4] = {ok ? r.x : 0, ok ? r.y : 0, ok ? r.width : 0, ok ? r.height : 0};
        CHECK(std::memcmp(rects.data() + (size_t)i * 16, want, 16) == 0, "rects() entry " << i);
    }

    // two cameras: ONE builder launch, ONE ChainBatch tick
    HIP_OK(hipMemset(out_a.data, 0, bytes));
    cvGS::DeviceCrops::update(stream, {{&crops_a, frame_a, d_boxes, d_count}, {&crops_b, frame_b, d_boxes, d_count + 1}}, CVGS_BOX_XYWH_I32, DS, cvGS::PRESERVE_AR);
    cvGS::ChainBatch tick;
    tick.add(cvGS::resize<CV_8UC3, cv::INTER_LINEAR, cvGS::PRESERVE_AR>(crops_a, bg), cvGS::cvtColor<cv::COLOR_RGB2BGR, CV_32FC3>(),
             cvGS::multiply<CV_32FC3>(cv::Scalar(0.3, 0.3, 0.3)), cvGS::subtract<CV_32FC3>(cv::Scalar(1.0, 4.0, 3.2)),
             cvGS::divide<CV_32FC3>(cv::Scalar(3.2, 0.6, 11.8)), cvGS::split<CV_32FC3>(out_a, DS));
    tick.add(cvGS::resize<CV_8UC3, cv::INTER_LINEAR, cvGS::PRESERVE_AR>(crops_b, bg), cvGS::cvtColor<cv::COLOR_RGB2BGR, CV_32FC3>(),
             cvGS::multiply<CV_32FC3>(cv::Scalar(0.3, 0.3, 0.3)), cvGS::subtract<CV_32FC3>(cv::Scalar(1.0, 4.0, 3.2)),
             cvGS::divide<CV_32FC3>(cv::Scalar(3.2, 0.6, 11.8)), cvGS::split<CV_32FC3>(out_b, DS));
    tick.execute(stream);
    stream.waitForCompletion();
    CHECK(bit_equal(fetch(out_a.data, bytes).data(), want_a.data(), bytes), "ChainBatch tick, camera 0");
    CHECK(bit_equal(fetch(out_b.data, bytes).data(), want_b.data(), bytes), "ChainBatch tick, camera 1");

    // the loop unchanged on a stream that records ticks
    HIP_OK(hipMemset(out_a.data, 0, bytes));
    HIP_OK(hipMemset(out_b.data, 0, bytes));
    cvGS::recordTicks(stream, 2);
    run_chain(stream, cvGS::resize<CV_8UC3, cv::INTER_LINEAR, cvGS::PRESERVE_AR>(crops_a, bg), out_a);
    run_chain(stream, cvGS::resize<CV_8UC3, cv::INTER_LINEAR, cvGS::PRESERVE_AR>(crops_b, bg), out_b);
    cvGS::stopRecording(stream);
    stream.waitForCompletion();
    CHECK(bit_equal(fetch(out_a.data, bytes).data(), want_a.data(), bytes), "recorded tick, camera 0");
    CHECK(bit_equal(fetch(out_b.data, bytes).data(), want_b.data(), bytes), "recorded tick, camera 1");

    // the read refuses a mode the table was not built with
    bool threw = false;
    try { (void)cvGS::resize<CV_8UC3, cv::INTER_LINEAR, cvGS::IGNORE_AR>(crops_a, bg); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw, "resize(DeviceCrops) with another aspect-ratio mode throws");
    HIP_OK(hipFree(d_boxes));
    HIP_OK(hipFree(d_count));
    return report("test_devicecrops");
}
