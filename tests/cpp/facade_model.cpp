// facade_model.cpp -- the C++ facade's chains for the float64 model (tests/f64_model.py).
//
//   facade_model --list            prints the case names, in table order
//   facade_model <dir> oracle      host-backed GpuMats, fk::lowerChain + cvgs_validate + oracle_execute; makes no HIP runtime call
//   facade_model <dir> gpu         uploads the inputs, cvGS::executeOperations on a stream, prints the kernel's name per case
//
// For every case of its table the program reads the raw inputs <dir>/<case>.in<k> that tests/facade_cases.py wrote, builds the chain in
// the facade's own spelling (the cvGS:: templates, cv::Size, cv::Scalar, cv::Rect, cv::Mat, std::array<GpuMat, N>), runs it and writes
// <dir>/<case>.out: four int64 (guard, rows, row bytes, pitch), then the whole output buffer -- a canary band, rows x pitch bytes, a canary
// band; every byte is pre-filled with the canary.  It generates no data and knows no expected value: tests/facade_cases.py owns both and
// spells every chain a second time, for the model.  The two tables must hold the same names in the same order.
// The first failure (a HIP error, a refused chain, a missing file) ends the program with a non-zero status; nothing is started after it.
#include <cvGPUSpeedup.h>

#include <array>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../oracle/cvgs_oracle.h" // the oracle leg's executor; the product never uses it

using cv::cuda::GpuMat;

namespace {

constexpr size_t kGuard = 4096;
constexpr int kCanary = 0xA5;
constexpr size_t kPad = 64; // padding of a pitched output row

struct Ctx {
    std::string dir, name;
    bool gpu = false, oracle_ok = true, ran = false;
    std::unique_ptr<cv::cuda::Stream> stream; // gpu mode only
    std::vector<std::shared_ptr<std::vector<uint8_t>>> host_in;
    std::vector<GpuMat> dev_in;
    std::vector<uint8_t> host_out;
    std::shared_ptr<void> dev_out;
    size_t rows = 0, row_bytes = 0, pitch = 0;

    std::shared_ptr<std::vector<uint8_t>> load(int idx, size_t bytes) {
        const std::string path = dir + "/" + name + ".in" + std::to_string(idx);
        std::ifstream f(path, std::ios::binary);
        auto buf = std::make_shared<std::vector<uint8_t>>(bytes);
        if (!f || !f.read((char*)buf->data(), (std::streamsize)bytes) || f.peek() != EOF)
            throw std::runtime_error(path + ": missing, or not " + std::to_string(bytes) + " bytes");
        host_in.push_back(buf);
        return buf;
    }
    // input k as a rows x cols matrix of `type`: a host view (oracle) or an uploaded, pitched GpuMat (gpu)
    GpuMat src(int idx, int r, int c, int type) {
        auto buf = load(idx, (size_t)r * c * cv::cvgs_elem_size(type));
        cv::Mat m(r, c, type, buf->data());
        if (!gpu) return GpuMat(m.rows, m.cols, m.type(), m.data, m.step);
        GpuMat g;
        g.upload(m);
        dev_in.push_back(g);
        return g;
    }
    // input k as a CV_64FC1 host matrix (warp transforms)
    cv::Mat mat64(int idx, int r, int c) {
        auto buf = load(idx, (size_t)r * c * sizeof(double));
        cv::Mat m(r, c, CV_64FC1);
        std::memcpy(m.data, buf->data(), buf->size());
        return m;
    }
    // the case's output buffer: r rows of rb bytes, `pad` bytes of padding behind each; returns the first row
    uint8_t* out(size_t r, size_t rb, size_t pad) {
        if (rows) throw std::runtime_error(name + ": one output per case");
        rows = r; row_bytes = rb; pitch = rb + pad;
        const size_t total = 2 * kGuard + rows * pitch;
        if (!gpu) {
            host_out.assign(total, (uint8_t)kCanary);
            return host_out.data() + kGuard;
        }
        void* p = nullptr;
        fk::hip_check(hipMalloc(&p, total), "hipMalloc(output)");
        dev_out = std::shared_ptr<void>(p, [](void* q) { (void)hipFree(q); });
        fk::hip_check(hipMemset(p, kCanary, total), "hipMemset(output)");
        return (uint8_t*)p + kGuard;
    }
    GpuMat out2d(int r, int c, int type, bool pitched) {
        const size_t rb = (size_t)c * cv::cvgs_elem_size(type);
        uint8_t* p = out((size_t)r, rb, pitched ? kPad : 0);
        return GpuMat(r, c, type, p, pitch);
    }
    template <typename... IOps> void run(const IOps&... iops) {
        fk::ChainBuilder b;
        fk::lowerChain(b, iops...);
        if (cvgs_validate(&b.d) != CVGS_OK) throw std::runtime_error(name + ": cvgs_validate refused the chain: " + cvgs_last_error());
        ran = true;
        if (!gpu) {
            if (!oracle_ok) return; // a chain the CPU oracle does not know (packed 4:2:2, planar 4:4:4, bfloat16): lowered and validated only
            const int rc = oracle_execute(&b.d);
            if (rc != 0) throw std::runtime_error(name + ": oracle_execute failed: " + std::to_string(rc));
            return;
        }
        char kernel[128] = "";
        if (cvgs_kernel_name(&b.d, kernel, sizeof(kernel)) != CVGS_OK) throw std::runtime_error(name + ": cvgs_kernel_name failed");
        std::printf("KERNEL %s %s\n", name.c_str(), kernel);
        cvGS::executeOperations(*stream, iops...);
        stream->waitForCompletion();
        fk::hip_check(hipGetLastError(), "after the chain");
    }
    void finish() {
        if (!ran || !rows) throw std::runtime_error(name + ": the case ran no chain");
        if (!gpu && !oracle_ok) return;
        const size_t total = 2 * kGuard + rows * pitch;
        if (gpu) {
            host_out.resize(total);
            fk::hip_check(hipMemcpy(host_out.data(), dev_out.get(), total, hipMemcpyDeviceToHost), "hipMemcpy(output)");
        }
        const int64_t head[4] = {(int64_t)kGuard, (int64_t)rows, (int64_t)row_bytes, (int64_t)pitch};
        std::ofstream f(dir + "/" + name + ".out", std::ios::binary);
        f.write((const char*)head, sizeof(head));
        f.write((const char*)host_out.data(), (std::streamsize)total);
        if (!f) throw std::runtime_error(name + ": cannot write the output file");
    }
};

struct CaseDef {
    std::string name;
    bool oracle_ok;
    std::function<void(Ctx&)> fn;
};
std::vector<CaseDef> g_cases;
void add(const char* name, bool oracle_ok, std::function<void(Ctx&)> fn) { g_cases.push_back({name, oracle_ok, std::move(fn)}); }

// ---- the constants of tests/facade_cases.py -----------------------------------------------------------------------------------------
constexpr int FRAME_W = 97, FRAME_H = 61, PX_W = 67, PX_H = 45, YUV_W = 48, YUV_H = 32;
const cv::Scalar BG(17.25, 99.5, 3.0, 200.0);
const cv::Scalar MULV(0.00392156862745098, 0.0078125, 0.015625, 0.0625);
const cv::Scalar SUBV(0.485, 0.456, 0.406, 0.3);
const cv::Scalar DIVV(0.229, 0.224, 0.225, 0.25);
const cv::Scalar ADDV(1.5, -2.25, 3.125, -0.75);
const int AR_CROPS[5][4] = {{3, 5, 30, 20}, {4, 7, 13, 41}, {5, 6, 21, 40}, {10, 11, 1, 1}, {2, 2, 90, 11}};
const int ROI_CROPS[4][4] = {{3, 5, 30, 20}, {4, 7, 31, 21}, {60, 30, 37, 31}, {8, 8, 80, 50}};
const int USED_CROPS[5][4] = {{3, 5, 30, 20}, {4, 7, 31, 21}, {5, 6, 21, 40}, {10, 11, 1, 1}, {11, 2, 1, 33}};

template <size_t N> std::array<GpuMat, N> rois(const GpuMat& frame, const int (*r)[4]) {
    std::array<GpuMat, N> out;
    for (size_t i = 0; i < N; ++i) out[i] = frame(cv::Rect(r[i][0], r[i][1], r[i][2], r[i][3])); // GpuMat::operator()(Rect)
    return out;
}
template <typename T> auto px_read(const GpuMat& m) { return fk::Read<fk::PerThreadRead<fk::_2D, T>>{cvGS::gpuMat2RawPtr2D<T>(m)}; }
// an N x (cn * w * h) tensor living in a GpuMat with one image per row
GpuMat tensor(Ctx& c, int n, int cn, const cv::Size& s, int type1 = CV_32FC1) { return c.out2d(n, cn * s.width * s.height, type1, false); }
// n x cn pitched planes of h x w, [image][channel] behind one another in ONE output buffer
std::vector<GpuMat> planes(Ctx& c, int count, const cv::Size& s) {
    GpuMat all = c.out2d(count * s.height, s.width, CV_32FC1, true);
    std::vector<GpuMat> p;
    for (int i = 0; i < count; ++i) p.push_back(all(cv::Rect(0, i * s.height, s.width, s.height)));
    return p;
}

// ---- resize ---------------------------------------------------------------------------------------------------------------------------
template <cvGS::AspectRatio AR> void resize_ar(Ctx& c) {
    const GpuMat frame = c.src(0, FRAME_H, FRAME_W, CV_8UC3);
    const cv::Size dst(40, 24);
    c.run(cvGS::resize<CV_8UC3, cv::INTER_LINEAR, 5, AR>(rois<5>(frame, AR_CROPS), dst, 5, BG), cvGS::split<CV_32FC3>(tensor(c, 5, 3, dst), dst));
}
template <int T> void resize_c1(Ctx& c) {
    const GpuMat frame = c.src(0, FRAME_H, FRAME_W, T);
    const cv::Size dst(24, 16);
    c.run(cvGS::resize<T, cv::INTER_LINEAR, 3>(rois<3>(frame, ROI_CROPS), dst, 3), cvGS::write<CV_32FC1>(c.out2d(3, dst.width * dst.height, CV_32FC1, false), dst));
}

// ---- per-pixel chains -----------------------------------------------------------------------------------------------------------------
template <int O, typename Stage> void convert(Ctx& c, const Stage& stage) {
    const GpuMat in = c.src(0, PX_H, PX_W, CV_8UC3);
    c.run(px_read<uchar3>(in), stage, cvGS::write<O>(c.out2d(PX_H, PX_W, O, true)));
}
template <cv::ColorConversionCodes CODE, int I, int O> void cvt(Ctx& c) {
    const GpuMat in = c.src(0, PX_H, PX_W, I);
    c.run(px_read<CUDA_T(I)>(in), cvGS::cvtColor<CODE, I, O>(), cvGS::write<O>(c.out2d(PX_H, PX_W, O, true)));
}
template <int CN> void cvt_both(const char* name, void (*u8)(Ctx&), void (*f32)(Ctx&)) {
    add((std::string("cvt_") + name + "_8u").c_str(), true, u8);
    add((std::string("cvt_") + name + "_32f").c_str(), true, f32);
}
#define CVT(NAME, CODE, ICN, OCN) \
    cvt_both<ICN>(NAME, cvt<CODE, CV_MAKETYPE(CV_8U, ICN), CV_MAKETYPE(CV_8U, OCN)>, cvt<CODE, CV_MAKETYPE(CV_32F, ICN), CV_MAKETYPE(CV_32F, OCN)>)

// ---- YUV surfaces: one trait per cvGS::cvtColor* family -------------------------------------------------------------------------------
struct NV12 {
    static constexpr int type = CV_8UC1, rows = YUV_H * 3 / 2;
    template <bool SWAP, bool ALPHA, fk::ColorRange CR, fk::ColorPrimitives CP, typename... A> static auto read(const GpuMat& s, const A&... a) {
        constexpr cv::ColorConversionCodes code = ALPHA ? (SWAP ? cv::COLOR_YUV2BGRA_NV12 : cv::COLOR_YUV2RGBA_NV12) : (SWAP ? cv::COLOR_YUV2BGR_NV12 : cv::COLOR_YUV2RGB_NV12);
        return cvGS::cvtColorNV12<code, CR, CP>(s, a...);
    }
    static std::array<cv::Rect, 2> crops() { return {cv::Rect(6, 12, 30, 18), cv::Rect(10, 4, 22, 10)}; }
    static std::array<cv::Rect, 2> crops_px() { return {cv::Rect(6, 12, 22, 10), cv::Rect(10, 4, 22, 10)}; }
};
struct P010 : NV12 {
    static constexpr int type = CV_16UC1;
    template <bool SWAP, bool ALPHA, fk::ColorRange CR, fk::ColorPrimitives CP, typename... A> static auto read(const GpuMat& s, const A&... a) {
        constexpr cv::ColorConversionCodes code = ALPHA ? (SWAP ? cv::COLOR_YUV2BGRA_NV12 : cv::COLOR_YUV2RGBA_NV12) : (SWAP ? cv::COLOR_YUV2BGR_NV12 : cv::COLOR_YUV2RGB_NV12);
        return cvGS::cvtColorP010<code, CR, CP>(s, a...);
    }
};
struct YUY2 {
    static constexpr int type = CV_8UC2, rows = YUV_H;
    template <bool SWAP, bool ALPHA, fk::ColorRange CR, fk::ColorPrimitives CP, typename... A> static auto read(const GpuMat& s, const A&... a) {
        constexpr cv::ColorConversionCodes code = ALPHA ? (SWAP ? cv::COLOR_YUV2BGRA_YUY2 : cv::COLOR_YUV2RGBA_YUY2) : (SWAP ? cv::COLOR_YUV2BGR_YUY2 : cv::COLOR_YUV2RGB_YUY2);
        return cvGS::cvtColorYUY2<code, CR, CP>(s, a...);
    }
    static std::array<cv::Rect, 2> crops() { return {cv::Rect(6, 13, 31, 17), cv::Rect(10, 3, 21, 9)}; }
    static std::array<cv::Rect, 2> crops_px() { return {cv::Rect(6, 13, 21, 9), cv::Rect(10, 3, 21, 9)}; }
};
struct UYVY : YUY2 {
    template <bool SWAP, bool ALPHA, fk::ColorRange CR, fk::ColorPrimitives CP, typename... A> static auto read(const GpuMat& s, const A&... a) {
        constexpr cv::ColorConversionCodes code = ALPHA ? (SWAP ? cv::COLOR_YUV2BGRA_UYVY : cv::COLOR_YUV2RGBA_UYVY) : (SWAP ? cv::COLOR_YUV2BGR_UYVY : cv::COLOR_YUV2RGB_UYVY);
        return cvGS::cvtColorUYVY<code, CR, CP>(s, a...);
    }
};
struct YUV444 {
    static constexpr int type = CV_8UC1, rows = YUV_H * 3;
    template <bool SWAP, bool ALPHA, fk::ColorRange CR, fk::ColorPrimitives CP, typename... A> static auto read(const GpuMat& s, const A&... a) {
        return cvGS::cvtColorYUV444<SWAP ? cv::COLOR_YUV2BGR : cv::COLOR_YUV2RGB, CR, CP, ALPHA>(s, a...);
    }
    static std::array<cv::Rect, 2> crops() { return {cv::Rect(5, 3, 31, 17), cv::Rect(11, 3, 21, 9)}; }
    static std::array<cv::Rect, 2> crops_px() { return {cv::Rect(5, 3, 21, 9), cv::Rect(11, 4, 21, 9)}; }
};

template <typename L> void yuv_px(Ctx& c) { // the whole surface, per pixel: RGB, full range, BT.601
    const GpuMat s = c.src(0, L::rows, YUV_W, L::type);
    c.run(L::template read<false, false, fk::Full, fk::bt601>(s), cvGS::write<CV_32FC3>(c.out2d(YUV_H, YUV_W, CV_32FC3, true)));
}
template <typename L> void yuv_rs(Ctx& c) { // the whole surface behind a resize: BGR, limited range, BT.709
    const GpuMat s = c.src(0, L::rows, YUV_W, L::type);
    const cv::Size dst(29, 19);
    c.run(cvGS::resize<cv::INTER_LINEAR>(L::template read<true, false, fk::Limited, fk::bt709>(s), dst), cvGS::split<CV_32FC3>(tensor(c, 1, 3, dst), dst));
}
template <typename L> void yuv_crops_letterbox(Ctx& c) { // std::array<cv::Rect, 2> crops, letterboxed: BGRA, limited range, BT.2020, a background
    const GpuMat s = c.src(0, L::rows, YUV_W, L::type);
    const cv::Size dst(40, 24);
    c.run(cvGS::resize<cv::INTER_LINEAR, cvGS::PRESERVE_AR>(L::template read<true, true, fk::Limited, fk::bt2020>(s, L::crops()), dst, BG),
          cvGS::split<CV_32FC4>(tensor(c, 2, 4, dst), dst));
}
template <typename L> void yuv_crops_px(Ctx& c) { // crops per pixel: RGBA, full range, BT.2020
    const GpuMat s = c.src(0, L::rows, YUV_W, L::type);
    const auto crops = L::crops_px();
    const cv::Size plane(crops[0].width, crops[0].height);
    c.run(L::template read<false, true, fk::Full, fk::bt2020>(s, crops), cvGS::write<CV_32FC4>(c.out2d(2, plane.width * plane.height, CV_32FC4, false), plane));
}
template <typename L> void yuv_family(const std::string& ln, bool oracle_ok) {
    add(("yuv_" + ln + "_px").c_str(), oracle_ok, yuv_px<L>);
    add(("yuv_" + ln + "_rs").c_str(), oracle_ok, yuv_rs<L>);
    add(("yuv_" + ln + "_crops_letterbox").c_str(), oracle_ok, yuv_crops_letterbox<L>);
    add(("yuv_" + ln + "_crops_px").c_str(), oracle_ok, yuv_crops_px<L>);
}

// ---- the table (the order and the names of tests/facade_cases.py) -------------------------------------------------------------------
void build_table() {
    // resize<T, INTER>(GpuMat, dsize, fx, fy) -> write<O>(GpuMat), pitched
    add("resize_single_dsize_8uc3", true, [](Ctx& c) {
        const GpuMat frame = c.src(0, FRAME_H, FRAME_W, CV_8UC3);
        c.run(cvGS::resize<CV_8UC3, cv::INTER_LINEAR>(frame, cv::Size(29, 19), 0., 0.), cvGS::write<CV_32FC3>(c.out2d(19, 29, CV_32FC3, true)));
    });
    add("resize_single_fxfy_8uc1", true, [](Ctx& c) {
        const GpuMat frame = c.src(0, FRAME_H, FRAME_W, CV_8UC1);
        c.run(cvGS::resize<CV_8UC1, cv::INTER_LINEAR>(frame, cv::Size(), 0.4, 0.3), cvGS::write<CV_32FC1>(c.out2d(18, 39, CV_32FC1, true)));
    });
    // std::array of GpuMat::operator()(Rect) crops -> the headline chain -> split<O>(GpuMat, Size)
    add("resize_batch_roi_8uc3", true, [](Ctx& c) {
        const GpuMat frame = c.src(0, FRAME_H, FRAME_W, CV_8UC3);
        const cv::Size dst(24, 16);
        c.run(cvGS::resize<CV_8UC3, cv::INTER_LINEAR, 4>(rois<4>(frame, ROI_CROPS), dst, 4), cvGS::cvtColor<cv::COLOR_RGB2BGR, CV_32FC3>(),
              cvGS::multiply<CV_32FC3>(MULV), cvGS::subtract<CV_32FC3>(SUBV), cvGS::divide<CV_32FC3>(DIVV), cvGS::split<CV_32FC3>(tensor(c, 4, 3, dst), dst));
    });
    // cvGS::crop(GpuMat, Rect2d): the doubles truncate
    add("resize_batch_crop2d_16uc3", true, [](Ctx& c) {
        const GpuMat frame = c.src(0, FRAME_H, FRAME_W, CV_16UC3);
        const cv::Size dst(24, 16);
        const std::array<GpuMat, 3> crops = {cvGS::crop(frame, cv::Rect2d(3.7, 5.2, 30.9, 20.5)), cvGS::crop(frame, cv::Rect2d(60.99, 30.5, 36.2, 30.9)),
                                             cvGS::crop(frame, cv::Rect2d(8.5, 8.5, 80.5, 50.5))};
        c.run(cvGS::resize<CV_16UC3, cv::INTER_LINEAR, 3>(crops, dst, 3), cvGS::split<CV_32FC3>(tensor(c, 3, 3, dst), dst));
    });
    // usedPlanes < N with a background Scalar -> splitT<O>(RawPtr<T3D>)
    add("resize_batch_used_bg_8uc4", true, [](Ctx& c) {
        const GpuMat frame = c.src(0, FRAME_H, FRAME_W, CV_8UC4);
        const cv::Size dst(24, 16);
        const GpuMat t = tensor(c, 5, 4, dst);
        fk::RawPtr<fk::T3D, float> out((float*)t.data, fk::Dims3D{24, 16, 5, 4, 24 * sizeof(float), 24 * 16 * sizeof(float)});
        c.run(cvGS::resize<CV_8UC4, cv::INTER_LINEAR, 5>(rois<5>(frame, USED_CROPS), dst, 3, BG), cvGS::splitT<CV_32FC4>(out));
    });
    add("resize_ar_preserve_8uc3", true, resize_ar<cvGS::PRESERVE_AR>);
    add("resize_ar_ignore_8uc3", true, resize_ar<cvGS::IGNORE_AR>);
    add("resize_ar_rn_even_8uc3", true, resize_ar<cvGS::PRESERVE_AR_RN_EVEN>);
    add("resize_ar_left_8uc3", true, resize_ar<cvGS::PRESERVE_AR_LEFT>);
    // one-channel sources -> write<O>(GpuMat, Size)
    add("resize_batch_8uc1", true, resize_c1<CV_8UC1>);
    add("resize_batch_16sc1", true, resize_c1<CV_16SC1>);
    add("resize_batch_32fc1", true, resize_c1<CV_32FC1>);

    add("convert_plain_8u_32f", true, [](Ctx& c) { convert<CV_32FC3>(c, cvGS::convertTo<CV_8UC3, CV_32FC3>()); });
    add("convert_alpha_8u_32f", true, [](Ctx& c) { convert<CV_32FC3>(c, cvGS::convertTo<CV_8UC3, CV_32FC3>(0.25f)); });
    add("convert_alpha_beta_8u_32f", true, [](Ctx& c) { convert<CV_32FC3>(c, cvGS::convertTo<CV_8UC3, CV_32FC3>((float)(1.0 / 255.0), -0.25f)); });
    add("convert_saturates_8u_8u", true, [](Ctx& c) { convert<CV_8UC3>(c, cvGS::convertTo<CV_8UC3, CV_8UC3>((float)3.1, -260.0f)); });
    add("convert_8u_16u", true, [](Ctx& c) { convert<CV_16UC3>(c, cvGS::convertTo<CV_8UC3, CV_16UC3>(700.5f, -70000.25f)); });
    add("convert_8u_16f", true, [](Ctx& c) { convert<CV_16FC3>(c, cvGS::convertTo<CV_8UC3, CV_16FC3>((float)(1.0 / 255.0), -0.25f)); });
    add("convert_8u_16bf", false, [](Ctx& c) { convert<CV_16BFC3>(c, cvGS::convertTo<CV_8UC3, CV_16BFC3>((float)(1.0 / 255.0), -0.25f)); });
    // the reference README's call: the redundant convertTo<CV_8UC3, CV_32FC3>() behind the batched resize, `substract`
    add("convert_readme_redundant_cast", true, [](Ctx& c) {
        const GpuMat frame = c.src(0, FRAME_H, FRAME_W, CV_8UC3);
        const cv::Size dst(29, 19);
        c.run(cvGS::resize<CV_8UC3, cv::INTER_LINEAR, 4>(rois<4>(frame, ROI_CROPS), dst, 4), cvGS::convertTo<CV_8UC3, CV_32FC3>(),
              cvGS::cvtColor<cv::COLOR_RGB2BGR, CV_32FC3>(), cvGS::multiply<CV_32FC3>(MULV), cvGS::substract<CV_32FC3>(SUBV), cvGS::divide<CV_32FC3>(DIVV),
              cvGS::split<CV_32FC3>(tensor(c, 4, 3, dst), dst));
    });

    // / + x - on one, three and four channels
    add("arith_32fc1", true, [](Ctx& c) {
        const GpuMat in = c.src(0, PX_H, PX_W, CV_32FC1);
        c.run(px_read<float>(in), cvGS::divide<CV_32FC1>(DIVV), cvGS::add<CV_32FC1>(ADDV), cvGS::multiply<CV_32FC1>(MULV), cvGS::subtract<CV_32FC1>(SUBV),
              cvGS::write<CV_32FC1>(c.out2d(PX_H, PX_W, CV_32FC1, true)));
    });
    add("arith_32fc3", true, [](Ctx& c) {
        const GpuMat in = c.src(0, PX_H, PX_W, CV_32FC3);
        c.run(px_read<float3>(in), cvGS::divide<CV_32FC3>(DIVV), cvGS::add<CV_32FC3>(ADDV), cvGS::multiply<CV_32FC3>(MULV), cvGS::substract<CV_32FC3>(SUBV),
              cvGS::write<CV_32FC3>(c.out2d(PX_H, PX_W, CV_32FC3, true)));
    });
    add("arith_32fc4", true, [](Ctx& c) {
        const GpuMat in = c.src(0, PX_H, PX_W, CV_32FC4);
        c.run(px_read<float4>(in), cvGS::divide<CV_32FC4>(DIVV), cvGS::add<CV_32FC4>(ADDV), cvGS::multiply<CV_32FC4>(MULV), cvGS::subtract<CV_32FC4>(SUBV),
              cvGS::write<CV_32FC4>(c.out2d(PX_H, PX_W, CV_32FC4, true)));
    });

    CVT("bgr2bgra", cv::COLOR_BGR2BGRA, 3, 4);
    CVT("bgra2bgr", cv::COLOR_BGRA2BGR, 4, 3);
    CVT("bgr2rgba", cv::COLOR_BGR2RGBA, 3, 4);
    CVT("bgra2rgb", cv::COLOR_BGRA2RGB, 4, 3);
    CVT("bgr2rgb", cv::COLOR_BGR2RGB, 3, 3);
    CVT("bgra2rgba", cv::COLOR_BGRA2RGBA, 4, 4);
    CVT("bgr2gray", cv::COLOR_BGR2GRAY, 3, 1);
    CVT("rgb2gray", cv::COLOR_RGB2GRAY, 3, 1);
    CVT("bgra2gray", cv::COLOR_BGRA2GRAY, 4, 1);
    CVT("rgba2gray", cv::COLOR_RGBA2GRAY, 4, 1);

    // split<O>(vector<GpuMat>): three pitched planes
    add("write_split_vector", true, [](Ctx& c) {
        const GpuMat frame = c.src(0, FRAME_H, FRAME_W, CV_8UC3);
        const cv::Size dst(29, 19);
        c.run(cvGS::resize<CV_8UC3, cv::INTER_LINEAR>(frame, dst, 0., 0.), cvGS::split<CV_32FC3>(planes(c, 3, dst)));
    });
    // split<O>(array<vector<GpuMat>, N>): four pitched planes per image
    add("write_split_array_of_vectors", true, [](Ctx& c) {
        const GpuMat frame = c.src(0, FRAME_H, FRAME_W, CV_8UC4);
        const cv::Size dst(24, 16);
        const std::vector<GpuMat> all = planes(c, 8, dst);
        const std::array<std::vector<GpuMat>, 2> out = {std::vector<GpuMat>(all.begin(), all.begin() + 4), std::vector<GpuMat>(all.begin() + 4, all.end())};
        c.run(cvGS::resize<CV_8UC4, cv::INTER_LINEAR, 2>(rois<2>(frame, ROI_CROPS), dst, 2), cvGS::split<CV_32FC4>(out));
    });
    // split<O>(RawPtr<_3D>)
    add("write_split_rawptr3d", true, [](Ctx& c) {
        const GpuMat frame = c.src(0, FRAME_H, FRAME_W, CV_8UC3);
        const cv::Size dst(24, 16);
        const GpuMat t = tensor(c, 3, 3, dst);
        fk::RawPtr<fk::_3D, float> out((float*)t.data, fk::Dims3D{24, 16, 3, 3, 24 * sizeof(float), 24 * 16 * sizeof(float)});
        c.run(cvGS::resize<CV_8UC3, cv::INTER_LINEAR, 3>(rois<3>(frame, ROI_CROPS), dst, 3), cvGS::split<CV_32FC3>(out));
    });
    // write(Tensor)
    add("write_tensor", true, [](Ctx& c) {
        const GpuMat frame = c.src(0, FRAME_H, FRAME_W, CV_8UC3);
        const cv::Size dst(29, 19);
        const GpuMat t = c.out2d(3, dst.width * dst.height, CV_32FC3, false);
        c.run(cvGS::resize<CV_8UC3, cv::INTER_LINEAR, 3>(rois<3>(frame, ROI_CROPS), dst, 3), cvGS::write(fk::Tensor<float3>((float3*)t.data, 29, 19, 3)));
    });

    // warps: FORWARD transforms as CV_64FC1 cv::Mat (inputs n .. 2n - 1), written with write<O>(GpuMat, Size)
    add("warp_affine_single", true, [](Ctx& c) {
        const GpuMat src = c.src(0, 90, 120, CV_8UC3);
        const cv::Size dst(110, 100);
        c.run(cvGS::warp<fk::WarpType::Affine, CV_8UC3>(src, c.mat64(1, 2, 3), dst), cvGS::write<CV_32FC3>(c.out2d(1, dst.width * dst.height, CV_32FC3, false), dst));
    });
    add("warp_perspective_single", true, [](Ctx& c) {
        const GpuMat src = c.src(0, 60, 80, CV_8UC3);
        const cv::Size dst(80, 60);
        c.run(cvGS::warp<fk::WarpType::Perspective, CV_8UC3>(src, c.mat64(1, 3, 3), dst), cvGS::write<CV_32FC3>(c.out2d(1, dst.width * dst.height, CV_32FC3, false), dst));
    });
    add("warp_affine_batch", true, [](Ctx& c) {
        const std::array<GpuMat, 3> src = {c.src(0, 90, 120, CV_8UC3), c.src(1, 90, 120, CV_8UC3), c.src(2, 90, 120, CV_8UC3)};
        const std::array<cv::Mat, 3> tm = {c.mat64(3, 2, 3), c.mat64(4, 2, 3), c.mat64(5, 2, 3)};
        const cv::Size dst(64, 48);
        c.run(cvGS::warp<fk::WarpType::Affine, CV_8UC3>(src, tm, dst), cvGS::cvtColor<cv::COLOR_RGB2BGR, CV_32FC3>(), cvGS::multiply<CV_32FC3>(MULV),
              cvGS::subtract<CV_32FC3>(SUBV), cvGS::divide<CV_32FC3>(DIVV), cvGS::write<CV_32FC3>(c.out2d(3, dst.width * dst.height, CV_32FC3, false), dst));
    });
    add("warp_perspective_batch_used_default", true, [](Ctx& c) {
        const std::array<GpuMat, 4> src = {c.src(0, 60, 80, CV_8UC3), c.src(1, 60, 80, CV_8UC3), c.src(2, 60, 80, CV_8UC3), c.src(3, 60, 80, CV_8UC3)};
        const std::array<cv::Mat, 4> tm = {c.mat64(4, 3, 3), c.mat64(5, 3, 3), c.mat64(6, 3, 3), c.mat64(7, 3, 3)};
        const cv::Size dst(80, 60);
        c.run(cvGS::warp<fk::WarpType::Perspective, CV_8UC3>(src, tm, dst, 2, cv::Scalar(7.0, 8.0, 9.0)), cvGS::cvtColor<cv::COLOR_RGB2BGR, CV_32FC3>(),
              cvGS::multiply<CV_32FC3>(MULV), cvGS::subtract<CV_32FC3>(SUBV), cvGS::divide<CV_32FC3>(DIVV),
              cvGS::write<CV_32FC3>(c.out2d(4, dst.width * dst.height, CV_32FC3, false), dst));
    });

    yuv_family<NV12>("nv12", true);
    yuv_family<P010>("p010", true);
    yuv_family<YUY2>("yuy2", false);
    yuv_family<UYVY>("uyvy", false);
    yuv_family<YUV444>("yuv444", false);

    // the fk:: spellings of the facade tests: Read<PerThreadRead>, Unary<SaturateCast>, Binary<Mul>, Write<PerThreadWrite>
    add("fk_read_mul_saturate", true, [](Ctx& c) {
        const GpuMat in = c.src(0, PX_H, PX_W, CV_8UC3);
        const GpuMat out = c.out2d(PX_H, PX_W, CV_8UC3, true);
        c.run(fk::Read<fk::PerThreadRead<fk::_2D, uchar3>>{cvGS::gpuMat2RawPtr2D<uchar3>(in)}, fk::Unary<fk::SaturateCast<uchar3, float3>>{},
              fk::Binary<fk::Mul<float3>>{fk::make_<float3>(1.25f, 0.5f, 2.75f)}, fk::Unary<fk::SaturateCast<float3, uchar3>>{},
              fk::Write<fk::PerThreadWrite<fk::_2D, uchar3>>{cvGS::gpuMat2RawPtr2D<uchar3>(out)});
    });
    // ... fk::fuse(Read<ReadYUV>, Unary<ConvertYUVToRGB>) behind fk::Resize::build(backOp, size), VectorReorder
    add("fk_resize_over_fused_nv12", true, [](Ctx& c) {
        const GpuMat s = c.src(0, YUV_H * 3 / 2, YUV_W, CV_8UC1);
        const GpuMat out = c.out2d(19, 29, CV_8UC4, true);
        fk::RawPtr<fk::_2D, uchar> luma;
        luma.data = s.data;
        luma.dims = {(uint)YUV_W, (uint)YUV_H, (uint)s.step};
        const auto back = fk::fuse(fk::Read<fk::ReadYUV<fk::NV12>>{luma}, fk::Unary<fk::ConvertYUVToRGB<fk::NV12, fk::Full, fk::bt709, true, float4>>{});
        c.run(fk::Resize<fk::INTER_LINEAR>::build(back, fk::Size(29, 19)), fk::Unary<fk::SaturateCast<float4, uchar4>>{},
              fk::Unary<fk::VectorReorder<uchar4, 2, 1, 0, 3>>{}, fk::Write<fk::PerThreadWrite<fk::_2D, uchar4>>{cvGS::gpuMat2RawPtr2D<uchar4>(out)});
    });
}

} // namespace

int main(int argc, char** argv) {
    build_table();
    if (argc == 2 && std::string(argv[1]) == "--list") {
        for (const CaseDef& d : g_cases) std::printf("%s\n", d.name.c_str());
        return 0;
    }
    const std::string mode = argc == 3 ? argv[2] : "";
    if (mode != "oracle" && mode != "gpu") {
        std::fprintf(stderr, "usage: facade_model --list | facade_model <dir> oracle|gpu\n");
        return 2;
    }
    std::unique_ptr<cv::cuda::Stream> stream;
    try {
        if (mode == "gpu") stream = std::make_unique<cv::cuda::Stream>();
        for (const CaseDef& d : g_cases) {
            Ctx c;
            c.dir = argv[1]; c.name = d.name; c.gpu = mode == "gpu"; c.oracle_ok = d.oracle_ok;
            if (c.gpu) c.stream = std::make_unique<cv::cuda::Stream>(*stream);
            d.fn(c);
            c.finish();
        }
    } catch (const std::exception& e) {
        std::fflush(stdout);
        std::fprintf(stderr, "facade_model: %s\n", e.what());
        return 1;
    }
    std::printf("facade_model: %zu cases done (%s)\n", g_cases.size(), mode.c_str());
    return 0;
}
