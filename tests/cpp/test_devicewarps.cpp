// test_devicewarps.cpp -- cvGS::DeviceWarps: aligned crops from device-side landmarks (cvgs_warp_tables_from_points) on the facade.
// The landmarks reach the device once; DeviceWarps::update fits the transforms there and warp<WT, T>(warps) reads the device table through
// executeOperations.  Checked bit for bit against the host-described warp (fk::WarpRead) whose matrices are the nine floats of each table
// entry -- valid items, a NaN landmark, coincident landmarks and items beyond the device-side count alike.
#include "common.h"

namespace {

constexpr int N = 12, K = 5, W = 97, H = 61;
const cv::Size DS(16, 8);
constexpr int kPlane = 16 * 8;
const std::vector<cv::Point2f> kTmpl = {{4.f, 2.f}, {11.f, 2.f}, {7.5f, 4.f}, {5.f, 6.f}, {10.f, 6.f}};

template <typename Read>
void run_chain(const cv::cuda::Stream& s, const Read& rd, cv::cuda::GpuMat& out) {
    cvGS::executeOperations(s, rd, cvGS::cvtColor<cv::COLOR_RGB2BGR, CV_32FC3>(), cvGS::multiply<CV_32FC3>(cv::Scalar(0.3, 0.3, 0.3)),
                            cvGS::subtract<CV_32FC3>(cv::Scalar(1.0, 4.0, 3.2)), cvGS::divide<CV_32FC3>(cv::Scalar(3.2, 0.6, 11.8)),
                            cvGS::split<CV_32FC3>(out, DS));
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
    cv::Mat h_frame(H, W, CV_8UC3);
    fill_random(h_frame, 0xFACE);
    cv::cuda::GpuMat frame;
    frame.upload(h_frame);

    // item i: the template scaled, rotated by a multiple of 30 degrees and moved (some partly or wholly outside the frame)
    std::vector<float> pts((size_t)N * K * 2);
    for (int i = 0; i < N; ++i) {
        const double ang = 0.5235987755982988 * i, sc = 0.6 + 0.35 * i, cx = -10.0 + 11.0 * i, cy = 5.0 + 5.0 * i;
        for (int j = 0; j < K; ++j) {
            const double x = kTmpl[(size_t)j].x - 7.5, y = kTmpl[(size_t)j].y - 4.0;
            pts[((size_t)i * K + j) * 2] = (float)(cx + sc * (std::cos(ang) * x - std::sin(ang) * y));
            pts[((size_t)i * K + j) * 2 + 1] = (float)(cy + sc * (std::sin(ang) * x + std::cos(ang) * y));
        }
    }
    pts[(size_t)3 * K * 2 + 4] = std::nanf("");                                            // item 3: a NaN coordinate
    for (int j = 0; j < K; ++j) { pts[((size_t)6 * K + j) * 2] = 40.f; pts[((size_t)6 * K + j) * 2 + 1] = 30.f; } // item 6: coincident
    const int32_t count = N - 2;                                                            // items 10, 11: beyond the count
    float* d_pts = nullptr;
    int32_t* d_count = nullptr;
    HIP_OK(hipMalloc((void**)&d_pts, pts.size() * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_count, sizeof(int32_t)));
    HIP_OK(hipMemcpy(d_pts, pts.data(), pts.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_count, &count, sizeof(count), hipMemcpyHostToDevice));

    cvGS::DeviceWarps warps(N);
    warps.update(stream, frame, d_pts, d_count, CVGS_WARP_FIT_SIMILARITY, kTmpl, DS);
    cv::cuda::GpuMat out(N, 3 * kPlane, CV_32FC1), want(N, 3 * kPlane, CV_32FC1);
    HIP_OK(hipMemset(out.data, 0xff, bytes));
    run_chain(stream, cvGS::warp<fk::WarpType::Affine, CV_8UC3>(warps), out);
    stream.waitForCompletion();

    // the table and the validity flags
    const std::vector<uint8_t> tab = fetch(warps.table(), (size_t)N * sizeof(Entry)), val = fetch(warps.valid(), (size_t)N * sizeof(int32_t));
    const float kInvalid[9] = {0.f, 0.f, -1.f, 0.f, 0.f, -1.f, 0.f, 0.f, 1.f};
    fk::WarpRead<fk::WarpType::Affine, CUDA_T(CV_8UC3)> host_rd;
    host_rd.planes.resize(N, cvgs_image2d{nullptr, 0, 0, 0, 0});
    host_rd.params.resize(N);
    host_rd.used = N;
    for (int i = 0; i < N; ++i) {
        Entry e;
        std::memcpy(&e, tab.data() + (size_t)i * sizeof(Entry), sizeof(Entry));
        int32_t v;
        std::memcpy(&v, val.data() + (size_t)i * 4, 4);
        const bool expect_valid = i != 3 && i != 6 && i < count;
        CHECK(v == (expect_valid ? 1 : 0), "valid() entry " << i);
        CHECK((std::memcmp(e.m, kInvalid, sizeof(kInvalid)) == 0) == !expect_valid, "invalid entries, and only they, hold the documented matrix: " << i);
        CHECK(e.data == frame.data && e.w == W && e.h == H && e.step == (int32_t)frame.step && e.dw == DS.width && e.dh == DS.height,
              "entry " << i << " names the frame and the target");
        host_rd.planes[(size_t)i] = cvgs_image2d{frame.data, frame.cols, frame.rows, (int32_t)frame.step, 0};
        for (int y = 0; y < 3; ++y)
            for (int x = 0; x < 3; ++x) host_rd.params[(size_t)i].transformMatrix[y][x] = e.m[3 * y + x];
        host_rd.params[(size_t)i].dstSize = fk::Size(DS.width, DS.height);
    }
    run_chain(stream, host_rd, want);
    stream.waitForCompletion();
    CHECK(bit_equal(fetch(out.data, bytes).data(), fetch(want.data, bytes).data(), bytes), "executeOperations over DeviceWarps == host-described warps");

    // the perspective kind over the same table (row 2 is 0 0 1)
    fk::WarpRead<fk::WarpType::Perspective, CUDA_T(CV_8UC3)> host_p;
    host_p.planes = host_rd.planes;
    host_p.params.resize(N);
    for (int i = 0; i < N; ++i) {
        std::memcpy(host_p.params[(size_t)i].transformMatrix, host_rd.params[(size_t)i].transformMatrix, 9 * sizeof(float));
        host_p.params[(size_t)i].dstSize = fk::Size(DS.width, DS.height);
    }
    host_p.used = N;
    HIP_OK(hipMemset(out.data, 0xff, bytes));
    run_chain(stream, cvGS::warp<fk::WarpType::Perspective, CV_8UC3>(warps), out);
    run_chain(stream, host_p, want);
    stream.waitForCompletion();
    CHECK(bit_equal(fetch(out.data, bytes).data(), fetch(want.data, bytes).data(), bytes), "perspective warp over DeviceWarps == host-described");

    // the read refuses another input type
    bool threw = false;
    try { (void)cvGS::warp<fk::WarpType::Affine, CV_8UC4>(warps); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw, "warp(DeviceWarps) with another input type throws");
    HIP_OK(hipFree(d_pts));
    HIP_OK(hipFree(d_count));
    return report("test_devicewarps");
}
