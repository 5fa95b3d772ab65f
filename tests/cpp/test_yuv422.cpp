// test_yuv422.cpp -- packed 4:2:2 surfaces (YUYV / UYVY) on the cvGS facade: cvtColorYUY2 / cvtColorUYVY -> resize -> normalize -> split.
// The checker is the CPU oracle's NV12 chain: a 4:2:2 surface whose chroma rows 2k and 2k + 1 are equal holds the picture of an NV12
// surface, so the same crops (even x, y, width, height) of both must give the same tensor, bit for bit.
#include "common.h"

// (H, W) packed surface of the NV12 picture h_nv12 ((H * 3 / 2, W), CV_8UC1); uyvy: bytes U Y0 V Y1, else Y0 U Y1 V
static cv::Mat pack422(const cv::Mat& h_nv12, int W, int H, bool uyvy) {
    cv::Mat s(H, W, CV_8UC2);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const uchar luma = h_nv12.ptr<uchar>(y)[x];
            const uchar chroma = h_nv12.ptr<uchar>(H + y / 2)[(x & ~1) + (x & 1)]; // even x: U of the pair, odd x: V
            uchar* px = s.ptr<uchar>(y) + 2 * x;
            px[uyvy ? 1 : 0] = luma;
            px[uyvy ? 0 : 1] = chroma;
        }
    return s;
}

template <bool UYVY, bool BGR>
static void test_crops(cv::cuda::Stream& stream) {
    const int W = 1280, H = 720;
    const cv::Size down(64, 128);
    constexpr size_t N = 5;
    const std::array<cv::Rect, N> crops = {cv::Rect(0, 0, W, H), cv::Rect(10, 20, 100, 200), cv::Rect(300, 100, 64, 128), cv::Rect(1200, 600, 80, 120), cv::Rect(2, 2, 6, 4)};
    cv::Mat h_nv12(H + H / 2, W, CV_8UC1);
    fill_random(h_nv12, 4220 + UYVY * 2 + BGR);
    cv::Mat h_422 = pack422(h_nv12, W, H, UYVY);
    cv::cuda::GpuMat d_422(h_422), hv_nv12 = host_view(h_nv12);
    const size_t n = N * (size_t)down.width * down.height * 3;
    cv::cuda::GpuMat d_out((int)N, down.width * down.height * 3, CV_32F);
    cv::Mat h_ref((int)N, down.width * down.height * 3, CV_32F);
    cv::cuda::GpuMat hv_ref = host_view(h_ref);
    const cv::Scalar a(0.3, 0.3, 0.3), s(1.f, 4.f, 3.2f), d(3.2f, 0.6f, 11.8f);
    auto go = [&](auto read) {
        cvGS::executeOperations(stream, cvGS::resize<cv::INTER_LINEAR>(read, down), cvGS::multiply<CV_32FC3>(a), cvGS::subtract<CV_32FC3>(s),
                                cvGS::divide<CV_32FC3>(d), cvGS::split<CV_32FC3>(d_out, down));
    };
    constexpr auto NV = BGR ? cv::COLOR_YUV2BGR_NV12 : cv::COLOR_YUV2RGB_NV12;
    if constexpr (UYVY) go(cvGS::cvtColorUYVY<BGR ? cv::COLOR_YUV2BGR_UYVY : cv::COLOR_YUV2RGB_UYVY, fk::Limited>(d_422, crops));
    else go(cvGS::cvtColorYUY2<BGR ? cv::COLOR_YUV2BGR_YUY2 : cv::COLOR_YUV2RGB_YUY2, fk::Limited>(d_422, crops));
    run_oracle(cvGS::resize<cv::INTER_LINEAR>(cvGS::cvtColorNV12<NV, fk::Limited>(hv_nv12, crops), down), cvGS::multiply<CV_32FC3>(a),
               cvGS::subtract<CV_32FC3>(s), cvGS::divide<CV_32FC3>(d), cvGS::split<CV_32FC3>(hv_ref, down));
    stream.waitForCompletion();
    const auto h = fetch(d_out.data, n * 4);
    CHECK(bit_equal(h.data(), h_ref.data, h.size()), (UYVY ? "cvtColorUYVY" : "cvtColorYUY2") << (BGR ? "<BGR>" : "<RGB>") << " crops -> resize -> normalize -> split, bit-exact vs the NV12 picture through the oracle");
}

static void test_refusals() {
    cv::cuda::GpuMat surf(16, 32, CV_8UC2), gray(16, 32, CV_8UC1);
    bool odd_x = false, wrong_type = false;
    try {
        (void)cvGS::cvtColorYUY2<cv::COLOR_YUV2RGB_YUY2>(surf, std::array<cv::Rect, 1>{cv::Rect(3, 0, 4, 4)});
    } catch (const std::runtime_error&) { odd_x = true; }
    try {
        (void)cvGS::cvtColorUYVY<cv::COLOR_YUV2RGB_UYVY>(gray);
    } catch (const std::runtime_error&) { wrong_type = true; }
    CHECK(odd_x, "a crop at an odd x is refused");
    CHECK(wrong_type, "a surface that is not CV_8UC2 is refused");
}

int main() {
    cv::cuda::Stream stream;
    test_crops<false, false>(stream);
    test_crops<false, true>(stream);
    test_crops<true, false>(stream);
    test_crops<true, true>(stream);
    test_refusals();
    return report("test_yuv422 (cvtColorYUY2 / cvtColorUYVY)");
}
