// test_yuv444.cpp -- planar 4:4:4 surfaces (I444) on the cvGS facade: cvtColorYUV444 -> resize -> normalize -> split.
// The checker is the CPU oracle's NV12 chain: a 4:4:4 surface whose chroma is constant in 2 x 2 blocks holds the picture of an NV12
// surface, so the same crops (even x, y, width, height) of both must give the same tensor, bit for bit.
#include "common.h"

// (3 * H, W) stacked planes Y, U, V of the NV12 picture h_nv12 ((H * 3 / 2, W), CV_8UC1)
static cv::Mat planes444(const cv::Mat& h_nv12, int W, int H) {
    cv::Mat s(3 * H, W, CV_8UC1);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            s.ptr<uchar>(y)[x] = h_nv12.ptr<uchar>(y)[x];
            s.ptr<uchar>(H + y)[x] = h_nv12.ptr<uchar>(H + y / 2)[x & ~1];
            s.ptr<uchar>(2 * H + y)[x] = h_nv12.ptr<uchar>(H + y / 2)[(x & ~1) + 1];
        }
    return s;
}

template <bool BGR>
static void test_crops(cv::cuda::Stream& stream) {
    const int W = 1280, H = 720;
    const cv::Size down(64, 128);
    constexpr size_t N = 5;
    const std::array<cv::Rect, N> crops = {cv::Rect(0, 0, W, H), cv::Rect(10, 20, 100, 200), cv::Rect(300, 100, 64, 128), cv::Rect(1200, 600, 80, 120), cv::Rect(2, 2, 6, 4)};
    cv::Mat h_nv12(H + H / 2, W, CV_8UC1);
    fill_random(h_nv12, 4440 + BGR);
    cv::Mat h_444 = planes444(h_nv12, W, H);
    cv::cuda::GpuMat d_444(h_444), hv_nv12 = host_view(h_nv12);
    const size_t n = N * (size_t)down.width * down.height * 3;
    cv::cuda::GpuMat d_out((int)N, down.width * down.height * 3, CV_32F);
    cv::Mat h_ref((int)N, down.width * down.height * 3, CV_32F);
    cv::cuda::GpuMat hv_ref = host_view(h_ref);
    const cv::Scalar a(0.3, 0.3, 0.3), s(1.f, 4.f, 3.2f), d(3.2f, 0.6f, 11.8f);
    constexpr auto NV = BGR ? cv::COLOR_YUV2BGR_NV12 : cv::COLOR_YUV2RGB_NV12;
    cvGS::executeOperations(stream, cvGS::resize<cv::INTER_LINEAR>(cvGS::cvtColorYUV444<BGR ? cv::COLOR_YUV2BGR : cv::COLOR_YUV2RGB, fk::Limited>(d_444, crops), down),
                            cvGS::multiply<CV_32FC3>(a), cvGS::subtract<CV_32FC3>(s), cvGS::divide<CV_32FC3>(d), cvGS::split<CV_32FC3>(d_out, down));
    run_oracle(cvGS::resize<cv::INTER_LINEAR>(cvGS::cvtColorNV12<NV, fk::Limited>(hv_nv12, crops), down), cvGS::multiply<CV_32FC3>(a),
               cvGS::subtract<CV_32FC3>(s), cvGS::divide<CV_32FC3>(d), cvGS::split<CV_32FC3>(hv_ref, down));
    stream.waitForCompletion();
    const auto h = fetch(d_out.data, n * 4);
    CHECK(bit_equal(h.data(), h_ref.data, h.size()), "cvtColorYUV444" << (BGR ? "<BGR>" : "<RGB>") << " crops -> resize -> normalize -> split, bit-exact vs the NV12 picture through the oracle");
}

// the whole surface, with alpha, through the resize: equal to the full-surface crop of the crops overload, and alpha = 255 everywhere
static void test_whole_surface_with_alpha(cv::cuda::Stream& stream) {
    const int W = 322, H = 198;
    const cv::Size down(65, 33);
    cv::Mat h_444(3 * H, W, CV_8UC1);
    fill_random(h_444, 4450);
    cv::cuda::GpuMat d_444(h_444);
    const size_t n = (size_t)down.width * down.height * 4;
    cv::cuda::GpuMat d_a(1, (int)n, CV_32F), d_b(1, (int)n, CV_32F);
    cvGS::executeOperations(stream, cvGS::resize<cv::INTER_LINEAR>(cvGS::cvtColorYUV444<cv::COLOR_YUV2RGB, fk::Full, fk::bt601, true>(d_444), down),
                            cvGS::split<CV_32FC4>(d_a, down));
    cvGS::executeOperations(stream, cvGS::resize<cv::INTER_LINEAR>(cvGS::cvtColorYUV444<cv::COLOR_YUV2RGB, fk::Full, fk::bt601, true>(d_444, std::array<cv::Rect, 1>{cv::Rect(0, 0, W, H)}), down),
                            cvGS::split<CV_32FC4>(d_b, down));
    stream.waitForCompletion();
    const auto ha = fetch(d_a.data, n * 4), hb = fetch(d_b.data, n * 4);
    CHECK(bit_equal(ha.data(), hb.data(), ha.size()), "cvtColorYUV444(surf) equals its full-surface crop");
    bool alpha = true;
    const float* fa = (const float*)ha.data();
    for (size_t i = 3 * n / 4; i < n; ++i) alpha = alpha && fa[i] == 255.f;
    CHECK(alpha, "the alpha plane holds 255");
}

static void test_refusals() {
    cv::cuda::GpuMat surf(48, 32, CV_8UC1), pairs(48, 32, CV_8UC2), ragged(50, 32, CV_8UC1);
    bool outside = false, wrong_type = false, wrong_rows = false, odd_ok = true;
    try {
        (void)cvGS::cvtColorYUV444<cv::COLOR_YUV2RGB>(surf, std::array<cv::Rect, 1>{cv::Rect(30, 0, 4, 4)});
    } catch (const std::runtime_error&) { outside = true; }
    try {
        (void)cvGS::cvtColorYUV444<cv::COLOR_YUV2RGB>(pairs);
    } catch (const std::runtime_error&) { wrong_type = true; }
    try {
        (void)cvGS::cvtColorYUV444<cv::COLOR_YUV2BGR>(ragged);
    } catch (const std::runtime_error&) { wrong_rows = true; }
    try {
        (void)cvGS::cvtColorYUV444<cv::COLOR_YUV2RGB>(surf, std::array<cv::Rect, 2>{cv::Rect(3, 5, 7, 9), cv::Rect(31, 15, 1, 1)});
    } catch (const std::runtime_error&) { odd_ok = false; }
    CHECK(outside, "a crop outside the surface is refused");
    CHECK(wrong_type, "a surface that is not CV_8UC1 is refused");
    CHECK(wrong_rows, "a surface whose rows are no multiple of 3 is refused");
    CHECK(odd_ok, "crops at odd origins and of odd sizes are taken");
}

int main() {
    cv::cuda::Stream stream;
    test_crops<false>(stream);
    test_crops<true>(stream);
    test_whole_surface_with_alpha(stream);
    test_refusals();
    return report("test_yuv444 (cvtColorYUV444)");
}
