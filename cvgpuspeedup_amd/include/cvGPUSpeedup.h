// cvGPUSpeedup.h -- the cvGS:: facade for the hot path, source-compatible with the reference's
// include/cvGPUSpeedup.cuh call shapes, on the MI355X engine.
//
//   cvGS::executeOperations(stream, cvGS::resize<CV_8UC3, cv::INTER_LINEAR, N>(crops, size, used),
//                           cvGS::cvtColor<cv::COLOR_RGB2BGR, CV_32FC3>(), cvGS::multiply<CV_32FC3>(a),
//                           cvGS::subtract<CV_32FC3>(s), cvGS::divide<CV_32FC3>(d),
//                           cvGS::split<CV_32FC3>(tensor, size));
//
// Each builder returns a typed IOp value (fk_compat.h); executeOperations checks the type chain at compile time,
// lowers the list to ONE cvgs_chain_desc and calls cvgs_execute() (include/cvgs_hip.h) -> ONE HIP kernel.  All
// calls are asynchronous on the given stream and never synchronise; device memory stays caller-owned.
// Not provided (outside the hot path): fk::StaticLoop.
#pragma once

#include <array>
#include <cassert>
#include <vector>

#include "cvGPUSpeedupHelpers.h"

namespace cvGS {

enum AspectRatio { PRESERVE_AR = 0, IGNORE_AR = 1, PRESERVE_AR_RN_EVEN = 2, PRESERVE_AR_LEFT = 3 };

// ---- GpuMat -> fk pointer adapters ------------------------------------------------------------------------
template <typename T>
inline fk::Ptr2D<T> gpuMat2Ptr2D(const cv::cuda::GpuMat& m) {
    return fk::Ptr2D<T>(reinterpret_cast<T*>(m.data), (uint)m.cols, (uint)m.rows, (uint)m.step);
}
template <typename T>
inline fk::RawPtr<fk::_2D, T> gpuMat2RawPtr2D(const cv::cuda::GpuMat& m) {
    fk::RawPtr<fk::_2D, T> p;
    p.data = reinterpret_cast<T*>(m.data);
    p.dims = {(uint)m.cols, (uint)m.rows, (uint)m.step};
    return p;
}
// reference include/cvGPUSpeedup.cuh:46-52
template <typename T, int Batch>
inline std::array<fk::Ptr2D<T>, Batch> gpuMat2Ptr2D_arr(const std::array<cv::cuda::GpuMat, Batch>& src) {
    std::array<fk::Ptr2D<T>, Batch> out;
    for (int i = 0; i < Batch; ++i) out[(size_t)i] = gpuMat2Ptr2D<T>(src[(size_t)i]);
    return out;
}
template <typename T, size_t N>
inline std::array<fk::RawPtr<fk::_2D, T>, N> gpuMat2RawPtr2D_arr(const std::array<cv::cuda::GpuMat, N>& src, int used = (int)N) {
    std::array<fk::RawPtr<fk::_2D, T>, N> out{};
    for (int i = 0; i < used && i < (int)N; ++i) out[(size_t)i] = gpuMat2RawPtr2D<T>(src[(size_t)i]);
    return out;
}
template <typename T>
inline fk::Tensor<T> gpuMat2Tensor(const cv::cuda::GpuMat& m, const cv::Size& plane, int colorPlanes) {
    return fk::Tensor<T>(reinterpret_cast<T*>(m.data), (uint)plane.width, (uint)plane.height, (uint)m.rows, (uint)colorPlanes);
}

// ---- pointwise builders ------------------------------------------------------------------------------------
template <int I, int O>
inline auto convertTo() {
    static_assert(CV_MAT_CN(I) == CV_MAT_CN(O), "convertTo does not support changing the number of channels, neither in cvGS nor in OpenCV. Please, use cvGS::cvtColor instead.");
    return fk::Unary<fk::SaturateCast<CUDA_T(I), CUDA_T(O)>>{};
}

namespace internal {
// integral outputs go through float: cast -> mul -> (add) -> saturate; float outputs: cast -> mul -> (add)
template <int I, int O>
inline auto convertToScaled(float alpha, const float* beta) {
    static_assert(CV_MAT_CN(I) == CV_MAT_CN(O), "convertTo does not support changing the number of channels, neither in cvGS nor in OpenCV. Please, use cvGS::cvtColor instead.");
    constexpr bool integral = CV_MAT_DEPTH(O) <= CV_32S || CV_MAT_DEPTH(O) == CV_16F; // CV_16F / CV_16BF: storage only, rounded once
    constexpr int mid = integral ? CV_32F : CV_MAT_DEPTH(O);
    fk::PointwiseSeq<CUDA_T(I), CUDA_T(O)> seq;
    fk::ChainBuilder b;
    b.op(CVGS_OP_CAST, mid);
    const float a[4] = {alpha, alpha, alpha, alpha};
    b.op(CVGS_OP_MUL, 0, a); // operand_d follows as (double)alpha: fk::make_set<FloatType>(alpha) on CV_64F outputs
    if (beta) {
        const float bb[4] = {*beta, *beta, *beta, *beta};
        b.op(CVGS_OP_ADD, 0, bb);
    }
    if (integral) b.op(CVGS_OP_CAST, CV_MAT_DEPTH(O) | (O & 0x1000)); // (CV_16BF: CVGS_DEPTH_16BF)
    seq.ops.assign(b.d.ops, b.d.ops + b.d.n_ops);
    return seq;
}
} // namespace internal

template <int I, int O> inline auto convertTo(float alpha) { return internal::convertToScaled<I, O>(alpha, nullptr); }
template <int I, int O> inline auto convertTo(float alpha, float beta) { return internal::convertToScaled<I, O>(alpha, &beta); }

template <int I> inline auto multiply(const cv::Scalar& s) { return fk::Binary<fk::Mul<CUDA_T(I)>>{cvScalar2CUDAV<I>::get(s)}; }
template <int I> inline auto subtract(const cv::Scalar& s) { return fk::Binary<fk::Sub<CUDA_T(I)>>{cvScalar2CUDAV<I>::get(s)}; }
// (the reference README's example spells it `substract`, README.md:127: the snippet users copy compiles)
template <int I> inline auto substract(const cv::Scalar& s) { return subtract<I>(s); }
template <int I> inline auto divide(const cv::Scalar& s) { return fk::Binary<fk::Div<CUDA_T(I)>>{cvScalar2CUDAV<I>::get(s)}; }
template <int I> inline auto add(const cv::Scalar& s) { return fk::Binary<fk::Add<CUDA_T(I)>>{cvScalar2CUDAV<I>::get(s)}; }

template <cv::ColorConversionCodes CODE, int I, int O = I>
inline auto cvtColor() {
    static_assert((CV_MAT_DEPTH(I) == CV_8U || CV_MAT_DEPTH(I) == CV_16U || CV_MAT_DEPTH(I) == CV_32F) &&
                  (CV_MAT_DEPTH(O) == CV_8U || CV_MAT_DEPTH(O) == CV_16U || CV_MAT_DEPTH(O) == CV_32F),
                  "Wrong CV_TYPE_DEPTH, it has to be CV_8U, or CV_16U or CV_32F");
    static_assert(isSupportedColorConversion<CODE>, "Color conversion type not supported yet.");
    return fk::Unary<fk::ColorConversion<(fk::ColorConversionCodes)CODE, CUDA_T(I), CUDA_T(O)>>{};
}

// ---- write builders ------------------------------------------------------------------------------------------
template <int O>
inline auto split(const std::vector<cv::cuda::GpuMat>& output) {
    std::vector<fk::Ptr2D<BASE_CUDA_T(O)>> planes;
    for (const auto& m : output) planes.push_back(gpuMat2Ptr2D<BASE_CUDA_T(O)>(m));
    return fk::SplitWrite<fk::_2D, CUDA_T(O)>::build(planes);
}
template <int O, size_t N>
inline auto split(const std::array<std::vector<cv::cuda::GpuMat>, N>& output) {
    std::array<std::vector<fk::Ptr2D<BASE_CUDA_T(O)>>, N> planes{};
    for (size_t i = 0; i < N; ++i)
        for (const auto& m : output[i]) planes[i].push_back(gpuMat2Ptr2D<BASE_CUDA_T(O)>(m));
    return fk::SplitWrite<fk::_2D, CUDA_T(O)>::build(planes);
}
// NCHW tensor living in a GpuMat with one image per row
template <int O>
inline auto split(const cv::cuda::GpuMat& output, const cv::Size& plane) {
    assert(output.cols % (plane.width * plane.height) == 0 && output.cols / (plane.width * plane.height) == CV_MAT_CN(O) &&
           "Each row of the GpuMat should contain as many planes as width / (planeDims.width * planeDims.height)");
    return fk::Write<fk::TensorSplit<CUDA_T(O)>>{gpuMat2Tensor<BASE_CUDA_T(O)>(output, plane, CV_MAT_CN(O)).ptr()};
}
template <int O>
inline auto split(const fk::RawPtr<fk::_3D, typename fk::VectorTraits<CUDA_T(O)>::base>& output) {
    return fk::Write<fk::TensorSplit<CUDA_T(O)>>{output};
}
template <int O>
inline auto splitT(const fk::RawPtr<fk::T3D, typename fk::VectorTraits<CUDA_T(O)>::base>& output) {
    return fk::Write<fk::TensorTSplit<CUDA_T(O)>>{output};
}
template <int O>
inline auto write(const cv::cuda::GpuMat& output) {
    return fk::Write<fk::PerThreadWrite<fk::_2D, CUDA_T(O)>>{gpuMat2RawPtr2D<CUDA_T(O)>(output)};
}
template <int O>
inline auto write(const cv::cuda::GpuMat& output, const cv::Size& plane) {
    return fk::Write<fk::PerThreadWrite<fk::_3D, CUDA_T(O)>>{gpuMat2Tensor<CUDA_T(O)>(output, plane, 1).ptr()};
}
template <typename T>
inline auto write(const fk::Tensor<T>& output) {
    return fk::Write<fk::PerThreadWrite<fk::_3D, T>>{output.ptr()};
}

// writeNV12<range, primaries>(surface) / writeNV21<...>: the chain ENDS in an 8-bit 4:2:0 encoder surface (NEW: CVGS_WRITE_NV12, an engine
// extension) -- the float3 R, G, B value is converted to Y'CbCr, the chroma of every 2 x 2 block averaged, and the surface stored by the
// same kernel that read and resized the picture.  `surface` is a CV_8UC1 GpuMat of H * 3 / 2 rows (H luma rows, then H / 2 interleaved
// chroma rows), as cvtColorNV12 takes it; the std::array overload writes one surface per batch element.  A BGR chain puts
// cvtColor<cv::COLOR_BGR2RGB, CV_32FC3>() in front.
namespace internal {
template <size_t N>
inline fk::Nv12SurfaceWrite nv12_surface_write(const std::array<cv::cuda::GpuMat, N>& surfaces, int range, int primaries, int layout, const char* what) {
    fk::Nv12SurfaceWrite w;
    w.params = CVGS_WRITE_YUV_PARAMS(range, primaries, layout);
    for (const auto& s : surfaces) {
        if (s.type() != CV_8UC1 || s.rows % 3 != 0 || ((s.rows / 3 * 2) & 1) || (s.cols & 1))
            throw std::runtime_error(std::string(what) + " needs CV_8UC1 surfaces with rows = H * 3 / 2, H and the width even");
        w.planes.push_back(cvgs_image2d{s.data, s.cols, s.rows / 3 * 2, (int32_t)s.step, 0});
    }
    return w;
}
} // namespace internal
template <fk::ColorRange CR = fk::Full, fk::ColorPrimitives CP = fk::bt709, size_t N>
inline auto writeNV12(const std::array<cv::cuda::GpuMat, N>& surfaces) {
    return internal::nv12_surface_write(surfaces, (int)CR, (int)CP, CVGS_YUV_NV12, "writeNV12");
}
template <fk::ColorRange CR = fk::Full, fk::ColorPrimitives CP = fk::bt709>
inline auto writeNV12(const cv::cuda::GpuMat& surface) {
    return writeNV12<CR, CP>(std::array<cv::cuda::GpuMat, 1>{surface});
}
template <fk::ColorRange CR = fk::Full, fk::ColorPrimitives CP = fk::bt709, size_t N>
inline auto writeNV21(const std::array<cv::cuda::GpuMat, N>& surfaces) {
    return internal::nv12_surface_write(surfaces, (int)CR, (int)CP, CVGS_YUV_NV21, "writeNV21");
}
template <fk::ColorRange CR = fk::Full, fk::ColorPrimitives CP = fk::bt709>
inline auto writeNV21(const cv::cuda::GpuMat& surface) {
    return writeNV21<CR, CP>(std::array<cv::cuda::GpuMat, 1>{surface});
}

// ---- read builders ---------------------------------------------------------------------------------------------
// resize<INTER>(dsize): a resize still waiting for its source -- complete it with readIOp.then(...)
template <int INTER_F>
inline auto resize(const cv::Size& dsize) {
    static_assert(isSupportedInterpolation<INTER_F>, "Interpolation type not supported yet.");
    return fk::Resize<(fk::InterpolationType)INTER_F>::build(fk::Size(dsize.width, dsize.height));
}
// single image: resize<T, INTER>(GpuMat, dsize, fx, fy); the output type is CV_32F of the same channels
template <int T, int INTER_F>
inline auto resize(const cv::cuda::GpuMat& input, const cv::Size& dsize, double fx, double fy) {
    static_assert(isSupportedInterpolation<INTER_F>, "Interpolation type not supported yet.");
    return fk::Resize<(fk::InterpolationType)INTER_F>::build(gpuMat2RawPtr2D<CUDA_T(T)>(input), fk::Size(dsize.width, dsize.height), fx, fy);
}

// batch: N crops -> dsize, planes >= usedPlanes (and the AR padding) take backgroundValue
template <int T, int INTER_F, int NPtr, AspectRatio AR_ = IGNORE_AR>
inline auto resize(const std::array<cv::cuda::GpuMat, NPtr>& input, const cv::Size& dsize, const int& usedPlanes,
                   const cv::Scalar& backgroundValue_ = cvScalar_set<CV_MAKETYPE(CV_32F, CV_MAT_CN(T))>(0)) {
    static_assert(isSupportedInterpolation<INTER_F>, "Interpolation type not supported yet.");
    fk::BatchResizeRead<CUDA_T(T)> rd;
    rd.kind = fk::resize_read_kind<(fk::InterpolationType)INTER_F>; // cv::INTER_AREA: the box filter (CVGS_READ_RESIZE_AREA)
    rd.planes.resize((size_t)NPtr, cvgs_image2d{nullptr, 0, 0, 0, 0});
    for (int i = 0; i < usedPlanes && i < NPtr; ++i) rd.planes[(size_t)i] = fk::image2d(gpuMat2RawPtr2D<CUDA_T(T)>(input[(size_t)i]));
    rd.used = usedPlanes;
    rd.dsize = fk::Size(dsize.width, dsize.height);
    rd.ar = (int)AR_;
    for (int c = 0; c < CV_MAT_CN(T); ++c) rd.background[c] = static_cast<float>(backgroundValue_[c]);
    return rd;
}

// ---- NV12 sources (NEW: the reference has no cvGS:: wrapper for its fk::ReadYUV path) --------------
// cvtColorNV12<cv::COLOR_YUV2BGR_NV12 | RGB | BGRA | RGBA>(nv12): reads a decoder surface (CV_8UC1 GpuMat with
// H luma rows followed by H/2 interleaved UV rows, i.e. rows = H*3/2) as float BGR/RGB[A] pixels -- the first IOp of
// a chain.  resize<INTER>(thatIOp, dsize) fuses it as the read-back of the bilinear resize (one kernel).
namespace internal {
template <fk::PixelFormat PF, cv::ColorConversionCodes CODE, fk::ColorRange CR, fk::ColorPrimitives CP>
inline auto yuv_surface_read(const cv::cuda::GpuMat& surf, const char* what) {
    static_assert(CODE == cv::COLOR_YUV2RGB_NV12 || CODE == cv::COLOR_YUV2BGR_NV12 || CODE == cv::COLOR_YUV2RGBA_NV12 ||
                  CODE == cv::COLOR_YUV2BGRA_NV12, "Color conversion type not supported yet.");
    if (surf.type() != (PF == fk::P010 ? CV_16UC1 : CV_8UC1) || surf.rows % 3 != 0)
        throw std::runtime_error(std::string(what) + " needs a single-channel surface (CV_8UC1; CV_16UC1 for P010) with rows = H * 3 / 2");
    constexpr bool alpha = CODE == cv::COLOR_YUV2RGBA_NV12 || CODE == cv::COLOR_YUV2BGRA_NV12;
    constexpr bool swap = CODE == cv::COLOR_YUV2BGR_NV12 || CODE == cv::COLOR_YUV2BGRA_NV12;
    using O = std::conditional_t<alpha, float4, float3>;
    fk::RawPtr<fk::_2D, fk::YuvSample<PF>> luma;
    luma.data = (fk::YuvSample<PF>*)surf.data;
    luma.dims = {(uint)surf.cols, (uint)(surf.rows / 3 * 2), (uint)surf.step};
    return fk::YuvRead<PF, CR, CP, alpha, O, swap>{luma};
}
template <typename Read, size_t N>
inline void yuv_surface_crops(Read& rd, const cv::cuda::GpuMat& surf, const std::array<cv::Rect, N>& crops) {
    const int H = surf.rows / 3 * 2, step = (int)surf.step, esz = (int)surf.elemSize();
    for (const cv::Rect& r : crops) {
        if ((r.x | r.y | r.width | r.height) & 1) throw std::runtime_error("NV12 crops need even x, y, width and height");
        if (r.x < 0 || r.y < 0 || r.width < 2 || r.height < 2 || r.x + r.width > surf.cols || r.y + r.height > H)
            throw std::runtime_error("NV12 crop outside the surface");
        rd.crops.push_back(cvgs_image2d{surf.data + (size_t)r.y * step + (size_t)r.x * esz, r.width, r.height, step, (H - r.y + r.y / 2) * step});
    }
}
} // namespace internal
template <cv::ColorConversionCodes CODE, fk::ColorRange CR = fk::Full, fk::ColorPrimitives CP = fk::bt709>
inline auto cvtColorNV12(const cv::cuda::GpuMat& nv12) {
    return internal::yuv_surface_read<fk::NV12, CODE, CR, CP>(nv12, "cvtColorNV12");
}
// cvtColorNV12<CODE>(nv12, crops): N crops of the surface (even x, y, width, height) as a batch of N planes -- with
// resize<INTER>(thatIOp, dsize) the decode-side version of the headline path: N detections of a decoder surface ->
// colour conversion -> bilinear resize -> normalize -> NCHW tensor, ONE kernel, no intermediate BGR frame.
template <cv::ColorConversionCodes CODE, fk::ColorRange CR = fk::Full, fk::ColorPrimitives CP = fk::bt709, size_t N>
inline auto cvtColorNV12(const cv::cuda::GpuMat& nv12, const std::array<cv::Rect, N>& crops) {
    auto rd = cvtColorNV12<CODE, CR, CP>(nv12);
    internal::yuv_surface_crops(rd, nv12, crops);
    return rd;
}
// cvtColorP010<CODE[, range, primaries]>(p010[, crops]): the same for a 10-bit decoder surface (CV_16UC1, rows = H * 3 / 2,
// 10-bit codes in the high bits of every sample); R, G, B[, A] arrive on the 0..1023 scale (A = 1023).  The codes reuse
// OpenCV's *_NV12 names for the channel order.
template <cv::ColorConversionCodes CODE, fk::ColorRange CR = fk::Limited, fk::ColorPrimitives CP = fk::bt2020>
inline auto cvtColorP010(const cv::cuda::GpuMat& p010) {
    return internal::yuv_surface_read<fk::P010, CODE, CR, CP>(p010, "cvtColorP010");
}
template <cv::ColorConversionCodes CODE, fk::ColorRange CR = fk::Limited, fk::ColorPrimitives CP = fk::bt2020, size_t N>
inline auto cvtColorP010(const cv::cuda::GpuMat& p010, const std::array<cv::Rect, N>& crops) {
    auto rd = cvtColorP010<CODE, CR, CP>(p010);
    internal::yuv_surface_crops(rd, p010, crops);
    return rd;
}
// cvtColorYUY2<cv::COLOR_YUV2RGB_YUY2 | BGR | RGBA | BGRA[, range, primaries]>(surf[, crops]) and cvtColorUYVY<cv::COLOR_YUV2*_UYVY ...>:
// the same IOp for packed 4:2:2 surfaces of cameras, capture cards and 4:2:2 JPEG decoders (CV_8UC2 GpuMat, rows = H; bytes Y0 U Y1 V /
// U Y0 V Y1 per pixel pair).  Crops are plain views at an even x (any y, width, height).
namespace internal {
template <fk::PixelFormat PF, cv::ColorConversionCodes RGB, cv::ColorConversionCodes BGR, cv::ColorConversionCodes RGBA, cv::ColorConversionCodes BGRA,
          cv::ColorConversionCodes CODE, fk::ColorRange CR, fk::ColorPrimitives CP>
inline auto yuv422_surface_read(const cv::cuda::GpuMat& surf, const char* what) {
    static_assert(CODE == RGB || CODE == BGR || CODE == RGBA || CODE == BGRA, "Color conversion type not supported yet.");
    if (surf.type() != CV_8UC2) throw std::runtime_error(std::string(what) + " needs a packed 4:2:2 surface (CV_8UC2)");
    constexpr bool alpha = CODE == RGBA || CODE == BGRA;
    constexpr bool swap = CODE == BGR || CODE == BGRA;
    using O = std::conditional_t<alpha, float4, float3>;
    fk::RawPtr<fk::_2D, uchar> view;
    view.data = (uchar*)surf.data;
    view.dims = {(uint)surf.cols, (uint)surf.rows, (uint)surf.step};
    return fk::YuvRead<PF, CR, CP, alpha, O, swap>{view};
}
template <typename Read, size_t N>
inline void yuv422_surface_crops(Read& rd, const cv::cuda::GpuMat& surf, const std::array<cv::Rect, N>& crops) {
    const int step = (int)surf.step;
    for (const cv::Rect& r : crops) {
        if (r.x & 1) throw std::runtime_error("crops of packed 4:2:2 surfaces need an even x");
        if (r.x < 0 || r.y < 0 || r.width < 1 || r.height < 1 || r.x + r.width > surf.cols || r.y + r.height > surf.rows)
            throw std::runtime_error("packed 4:2:2 crop outside the surface");
        rd.crops.push_back(cvgs_image2d{surf.data + (size_t)r.y * step + (size_t)r.x * 2, r.width, r.height, step, 0});
    }
}
} // namespace internal
template <cv::ColorConversionCodes CODE, fk::ColorRange CR = fk::Full, fk::ColorPrimitives CP = fk::bt709>
inline auto cvtColorYUY2(const cv::cuda::GpuMat& surf) {
    return internal::yuv422_surface_read<fk::YUYV, cv::COLOR_YUV2RGB_YUY2, cv::COLOR_YUV2BGR_YUY2, cv::COLOR_YUV2RGBA_YUY2, cv::COLOR_YUV2BGRA_YUY2, CODE, CR, CP>(surf, "cvtColorYUY2");
}
template <cv::ColorConversionCodes CODE, fk::ColorRange CR = fk::Full, fk::ColorPrimitives CP = fk::bt709, size_t N>
inline auto cvtColorYUY2(const cv::cuda::GpuMat& surf, const std::array<cv::Rect, N>& crops) {
    auto rd = cvtColorYUY2<CODE, CR, CP>(surf);
    internal::yuv422_surface_crops(rd, surf, crops);
    return rd;
}
template <cv::ColorConversionCodes CODE, fk::ColorRange CR = fk::Full, fk::ColorPrimitives CP = fk::bt709>
inline auto cvtColorUYVY(const cv::cuda::GpuMat& surf) {
    return internal::yuv422_surface_read<fk::UYVY, cv::COLOR_YUV2RGB_UYVY, cv::COLOR_YUV2BGR_UYVY, cv::COLOR_YUV2RGBA_UYVY, cv::COLOR_YUV2BGRA_UYVY, CODE, CR, CP>(surf, "cvtColorUYVY");
}
template <cv::ColorConversionCodes CODE, fk::ColorRange CR = fk::Full, fk::ColorPrimitives CP = fk::bt709, size_t N>
inline auto cvtColorUYVY(const cv::cuda::GpuMat& surf, const std::array<cv::Rect, N>& crops) {
    auto rd = cvtColorUYVY<CODE, CR, CP>(surf);
    internal::yuv422_surface_crops(rd, surf, crops);
    return rd;
}
// cvtColorYUV444<cv::COLOR_YUV2RGB | cv::COLOR_YUV2BGR[, range, primaries, ALPHA]>(surf[, crops]): the same IOp for planar 4:4:4 surfaces
// (I444: rocDecode's YUV444 output, rocJPEG's output for non-subsampled JPEGs).  `surf` is a CV_8UC1 GpuMat of 3 * H rows, the planes Y, U,
// V stacked (as cvtColorNV12 takes H * 3 / 2 rows).  OpenCV has no RGBA code for this family, so alpha is a template bool.  Crops are
// cv::Rects at ANY origin and of any size >= 1, odd values included.
namespace internal {
inline cvgs_image2d yuv444_view(const cv::cuda::GpuMat& surf, const cv::Rect& r) {
    const int H = surf.rows / 3, step = (int)surf.step;
    if (r.x < 0 || r.y < 0 || r.width < 1 || r.height < 1 || r.x + r.width > surf.cols || r.y + r.height > H)
        throw std::runtime_error("planar 4:4:4 crop outside the surface");
    return cvgs_image2d{surf.data + (size_t)r.y * step + (size_t)r.x, r.width, r.height, step, H * step};
}
} // namespace internal
template <cv::ColorConversionCodes CODE, fk::ColorRange CR = fk::Full, fk::ColorPrimitives CP = fk::bt709, bool ALPHA = false, size_t N>
inline auto cvtColorYUV444(const cv::cuda::GpuMat& surf, const std::array<cv::Rect, N>& crops) {
    static_assert(CODE == cv::COLOR_YUV2RGB || CODE == cv::COLOR_YUV2BGR, "Color conversion type not supported yet.");
    if (surf.type() != CV_8UC1 || surf.rows < 3 || surf.rows % 3 != 0)
        throw std::runtime_error("cvtColorYUV444 needs a planar 4:4:4 surface (CV_8UC1 with rows = 3 * H: the planes Y, U, V stacked)");
    using O = std::conditional_t<ALPHA, float4, float3>;
    fk::RawPtr<fk::_2D, uchar> luma;
    luma.data = (uchar*)surf.data;
    luma.dims = {(uint)surf.cols, (uint)(surf.rows / 3), (uint)surf.step};
    fk::YuvRead<fk::I444, CR, CP, ALPHA, O, CODE == cv::COLOR_YUV2BGR> rd{luma};
    for (const cv::Rect& r : crops) rd.crops.push_back(internal::yuv444_view(surf, r)); // every view states its uv_offset, the whole surface too
    return rd;
}
template <cv::ColorConversionCodes CODE, fk::ColorRange CR = fk::Full, fk::ColorPrimitives CP = fk::bt709, bool ALPHA = false>
inline auto cvtColorYUV444(const cv::cuda::GpuMat& surf) {
    return cvtColorYUV444<CODE, CR, CP, ALPHA>(surf, std::array<cv::Rect, 1>{cv::Rect(0, 0, surf.cols, surf.rows / 3)});
}
template <int INTER_F, fk::PixelFormat PF, fk::ColorRange CR, fk::ColorPrimitives CP, bool ALPHA, typename O, bool SW>
inline auto resize(const fk::YuvRead<PF, CR, CP, ALPHA, O, SW>& nv12Read, const cv::Size& dsize) {
    static_assert(isSupportedInterpolation<INTER_F>, "Interpolation type not supported yet.");
    return fk::Resize<(fk::InterpolationType)INTER_F>::build(nv12Read, fk::Size(dsize.width, dsize.height));
}
// resize<INTER, AR>(thatIOp, dsize, backgroundValue): the decoder surface letterboxed into dsize (the AspectRatio modes of the
// batched resize, reference :218-245, on the NV12 read-back); the padding takes backgroundValue (in the IOp's channel order) and
// runs through the rest of the chain like a pixel.  One K4 launch: surface -> detector input tensor.
template <int INTER_F, AspectRatio AR, fk::PixelFormat PF, fk::ColorRange CR, fk::ColorPrimitives CP, bool ALPHA, typename O, bool SW>
inline auto resize(const fk::YuvRead<PF, CR, CP, ALPHA, O, SW>& nv12Read, const cv::Size& dsize, const cv::Scalar& backgroundValue = cv::Scalar()) {
    static_assert(isSupportedInterpolation<INTER_F>, "Interpolation type not supported yet.");
    const float bg[4] = {(float)backgroundValue[0], (float)backgroundValue[1], (float)backgroundValue[2], (float)backgroundValue[3]};
    return fk::Resize<(fk::InterpolationType)INTER_F, (fk::AspectRatio)AR>::build(nv12Read, fk::Size(dsize.width, dsize.height), bg);
}

// resizeArea(thatIOp, dsize) / resizeArea<AR>(thatIOp, dsize, backgroundValue): the same fusion through the BOX FILTER (cv::INTER_AREA's
// antialiasing; CVGS_READ_NV12_RESIZE_AREA, an engine extension) for surfaces and crops that shrink by large factors -- a 6K surface into a
// 720p network input, detections of a 4K surface into 64 x 128.  Over the IOp of cvtColorNV12 (NV12), cvtColorP010 and the fk::NV21 reader;
// the other layouts are refused when the chain is validated (CVGS_ERR_UNSUPPORTED).  A name of its own: resize<cv::INTER_AREA>(thatIOp, ...)
// keeps failing to compile, as it always has.
template <AspectRatio AR, fk::PixelFormat PF, fk::ColorRange CR, fk::ColorPrimitives CP, bool ALPHA, typename O, bool SW>
inline auto resizeArea(const fk::YuvRead<PF, CR, CP, ALPHA, O, SW>& nv12Read, const cv::Size& dsize, const cv::Scalar& backgroundValue = cv::Scalar()) {
    static_assert(PF == fk::NV12 || PF == fk::NV21 || PF == fk::P010, "resizeArea reads NV12, NV21 and P010 surfaces.");
    const float bg[4] = {(float)backgroundValue[0], (float)backgroundValue[1], (float)backgroundValue[2], (float)backgroundValue[3]};
    auto rd = fk::Resize<fk::INTER_LINEAR, (fk::AspectRatio)AR>::build(nv12Read, fk::Size(dsize.width, dsize.height), bg);
    rd.kind = CVGS_READ_NV12_RESIZE_AREA; // the bilinear spelling's fields, unchanged
    return rd;
}
template <fk::PixelFormat PF, fk::ColorRange CR, fk::ColorPrimitives CP, bool ALPHA, typename O, bool SW>
inline auto resizeArea(const fk::YuvRead<PF, CR, CP, ALPHA, O, SW>& nv12Read, const cv::Size& dsize) {
    return resizeArea<IGNORE_AR>(nv12Read, dsize);
}

// ---- warp (reference include/cvGPUSpeedup.cuh:267-442) --------------------------------------------------------------
// warp<WT, InputType[, BATCH]>(input(s), FORWARD transform(s) as CV_64FC1 cv::Mat, dstSize(s)[, usedPlanes, defaultValue]):
// the first IOp of a chain; its output is CV_32F of the input's channels.  The matrices are inverted on the host in
// double (cv::invertAffineTransform / cv::Mat::inv) and narrowed to float, like the reference.
namespace internal {
template <fk::WarpType WT>
inline fk::WarpingParameters<WT> warp_parameters(const cv::Mat& transform_matrix, const cv::Size& dstSize) {
    if (transform_matrix.type() != CV_64FC1) throw std::runtime_error("Transform matrix type should be CV_64FC1.");
    fk::WarpingParameters<WT> p;
    p.dstSize = fk::Size(dstSize.width, dstSize.height);
    if constexpr (WT == fk::WarpType::Affine) {
        cv::Mat inverse_transform_matrix;
        cv::invertAffineTransform(transform_matrix, inverse_transform_matrix);
        for (int y = 0; y < 2; ++y)
            for (int x = 0; x < 3; ++x) p.transformMatrix[y][x] = static_cast<float>(inverse_transform_matrix.ptr<double>(y)[x]);
    } else {
        const cv::Mat inverse_transform_matrix(transform_matrix.inv());
        for (int y = 0; y < 3; ++y)
            for (int x = 0; x < 3; ++x) p.transformMatrix[y][x] = static_cast<float>(inverse_transform_matrix.ptr<double>(y)[x]);
    }
    return p;
}
// the reference's public spellings (include/cvGPUSpeedup.cuh:269-284): the 6 / 9 doubles of an ALREADY INVERTED transform, row-major,
// narrowed to float, plus the target size
inline fk::WarpingParameters<fk::WarpType::Affine> warp_getWarpingAffineParameters(const double* const tm_raw, const cv::Size& dstSize) {
    fk::WarpingParameters<fk::WarpType::Affine> p;
    for (int i = 0; i < 6; ++i) p.transformMatrix[i / 3][i % 3] = static_cast<float>(tm_raw[i]);
    p.dstSize = fk::Size(dstSize.width, dstSize.height);
    return p;
}
inline fk::WarpingParameters<fk::WarpType::Perspective> warp_getWarpingPerspectiveParameters(const double* const tm_raw, const cv::Size& dstSize) {
    fk::WarpingParameters<fk::WarpType::Perspective> p;
    for (int i = 0; i < 9; ++i) p.transformMatrix[i / 3][i % 3] = static_cast<float>(tm_raw[i]);
    p.dstSize = fk::Size(dstSize.width, dstSize.height);
    return p;
}
// the batch spellings (include/cvGPUSpeedup.cuh:311-377): FORWARD transforms in, the device's (inverted, float) parameters out; entries at
// and beyond usedPlanes stay value-initialised
template <fk::WarpType WT, size_t BATCH>
inline std::array<fk::WarpingParameters<WT>, BATCH> warp_batchParameters(const std::array<cv::Mat, BATCH>& transform_matrices,
                                                                         const std::array<cv::Size, BATCH>& dstSize, const int& usedPlanes = BATCH) {
    std::array<fk::WarpingParameters<WT>, BATCH> out{};
    for (int i = 0; i < usedPlanes && i < (int)BATCH; ++i) out[(size_t)i] = warp_parameters<WT>(transform_matrices[(size_t)i], dstSize[(size_t)i]);
    return out;
}
} // namespace internal

template <fk::WarpType WT, int InputType = CV_8UC3>
inline auto warp(const cv::cuda::GpuMat& input, const cv::Mat& transform_matrix, const cv::Size& dstSize) {
    if (InputType != input.type()) throw std::runtime_error("Input type does not match the input type of the operation.");
    fk::WarpRead<WT, CUDA_T(InputType)> rd;
    rd.planes.assign(1, fk::image2d(gpuMat2RawPtr2D<CUDA_T(InputType)>(input)));
    rd.params.assign(1, internal::warp_parameters<WT>(transform_matrix, dstSize));
    rd.used = 1;
    return rd;
}
template <fk::WarpType WT, int InputType, size_t BATCH>
inline auto warp(const std::array<cv::cuda::GpuMat, BATCH>& inputs, const std::array<cv::Mat, BATCH>& transform_matrices,
                 const std::array<cv::Size, BATCH>& dstSize, const int& usedPlanes, const cv::Scalar& defaultValue) {
    fk::WarpRead<WT, CUDA_T(InputType)> rd;
    rd.planes.resize(BATCH, cvgs_image2d{nullptr, 0, 0, 0, 0});
    rd.params.resize(BATCH);
    for (size_t i = 0; i < BATCH; ++i) rd.params[i].dstSize = fk::Size(dstSize[i].width, dstSize[i].height); // also of unused planes
    for (int i = 0; i < usedPlanes && i < (int)BATCH; ++i) {
        if (InputType != inputs[(size_t)i].type()) throw std::runtime_error("Input type does not match the input type of the operation.");
        rd.planes[(size_t)i] = fk::image2d(gpuMat2RawPtr2D<CUDA_T(InputType)>(inputs[(size_t)i]));
        rd.params[(size_t)i] = internal::warp_parameters<WT>(transform_matrices[(size_t)i], dstSize[(size_t)i]);
    }
    rd.used = usedPlanes;
    for (int c = 0; c < CV_MAT_CN(InputType); ++c) rd.background[c] = static_cast<float>(defaultValue[c]); // Scalar() = zeros
    return rd;
}
template <fk::WarpType WT, int InputType, size_t BATCH>
inline auto warp(const std::array<cv::cuda::GpuMat, BATCH>& inputs, const std::array<cv::Mat, BATCH>& transform_matrices,
                 const std::array<cv::Size, BATCH>& dstSize) {
    return warp<WT, InputType>(inputs, transform_matrices, dstSize, (int)BATCH, cv::Scalar());
}
template <fk::WarpType WT, int InputType, size_t BATCH>
inline auto warp(const std::array<cv::cuda::GpuMat, BATCH>& inputs, const std::array<cv::Mat, BATCH>& transform_matrices,
                 const cv::Size& dstSize) {
    std::array<cv::Size, BATCH> sizes;
    sizes.fill(dstSize);
    return warp<WT, InputType>(inputs, transform_matrices, sizes, (int)BATCH, cv::Scalar());
}
template <fk::WarpType WT, int InputType, size_t BATCH>
inline auto warp(const std::array<cv::cuda::GpuMat, BATCH>& inputs, const std::array<cv::Mat, BATCH>& transform_matrices,
                 const cv::Size& dstSize, const int& usedPlanes, const cv::Scalar& defaultValue) {
    std::array<cv::Size, BATCH> sizes;
    sizes.fill(dstSize);
    return warp<WT, InputType>(inputs, transform_matrices, sizes, usedPlanes, defaultValue);
}

// crop == an ROI view (zero cost): same pointer arithmetic as GpuMat::operator()(Rect); Rect2d doubles truncate
// (reference :247-265,444-447: uint x/y, int width/height)
namespace internal {
inline fk::Rect fk_rect(const cv::Rect2d& r) { return fk::Rect(static_cast<uint>(r.x), static_cast<uint>(r.y), static_cast<int>(r.width), static_cast<int>(r.height)); }
} // namespace internal
inline auto crop(const cv::Rect2d& rect) { return fk::CropSpec{internal::fk_rect(rect)}; }
template <size_t BATCH>
inline auto crop(const std::array<cv::Rect2d, BATCH>& rects) {
    fk::BatchCropSpec<BATCH> spec;
    for (size_t i = 0; i < BATCH; ++i) spec.rects[i] = internal::fk_rect(rects[i]);
    return spec;
}
template <typename BackIOp> inline auto crop(const BackIOp& backIOp, const cv::Rect2d& rect) { return backIOp.then(crop(rect)); }
template <typename BackIOp, size_t BATCH>
inline auto crop(const BackIOp& backIOp, const std::array<cv::Rect2d, BATCH>& rects) { return backIOp.then(crop(rects)); }
inline cv::cuda::GpuMat crop(const cv::cuda::GpuMat& input, const cv::Rect2d& rect) { return input(cv::Rect(rect)); }
template <size_t BATCH>
inline std::array<cv::cuda::GpuMat, BATCH> crop(const cv::cuda::GpuMat& input, const std::array<cv::Rect2d, BATCH>& rects) {
    std::array<cv::cuda::GpuMat, BATCH> out;
    for (size_t i = 0; i < BATCH; ++i) out[i] = input(cv::Rect(rects[i]));
    return out;
}

// ---- executeOperations ---------------------------------------------------------------------------------------------
template <bool ENABLE_THREAD_FUSION, typename... IOpTypes>
inline void executeOperations(const cv::cuda::Stream& stream, const IOpTypes&... iops) {
    fk::executeOperations<ENABLE_THREAD_FUSION>(cv::cuda::StreamAccessor::getStream(stream), iops...);
}
template <typename... IOpTypes>
inline void executeOperations(const cv::cuda::Stream& stream, const IOpTypes&... iops) {
    executeOperations<true>(stream, iops...);
}

namespace internal {
template <typename First, typename... Rest> struct first_of { using type = First; };
template <typename... T> using first_input_t = typename first_of<T...>::type::InputType;
template <typename... T> struct last_of;
template <typename T> struct last_of<T> { using type = T; };
template <typename T, typename... R> struct last_of<T, R...> : last_of<R...> {};
template <typename... T> using last_output_t = typename last_of<T...>::type::OutputType;

template <typename T, size_t N>
inline fk::BatchPixelRead<T> batchRead(const std::array<cv::cuda::GpuMat, N>& in, size_t active, const cv::Scalar& def) {
    fk::BatchPixelRead<T> rd;
    rd.planes.resize(N, cvgs_image2d{nullptr, 0, 0, 0, 0});
    for (size_t i = 0; i < active && i < N; ++i) rd.planes[i] = fk::image2d(gpuMat2RawPtr2D<T>(in[i]));
    rd.used = (int)active;
    const T d = cvScalar2CUDAV_t<T>::get(def); // narrowed to the INPUT type, as the reference does
    fk::vec_to_floats(d, rd.background);
    return rd;
}
} // namespace internal

// input GpuMat given: a per-pixel read of it is prepended
template <bool TF, typename... IOpTypes>
inline void executeOperations(const cv::cuda::GpuMat& input, const cv::cuda::Stream& stream, const IOpTypes&... iops) {
    using In = internal::first_input_t<IOpTypes...>;
    const fk::Read<fk::PerThreadRead<fk::_2D, In>> read{gpuMat2RawPtr2D<In>(input)};
    fk::executeOperations<TF>(cv::cuda::StreamAccessor::getStream(stream), read, iops...);
}
template <typename... IOpTypes>
inline void executeOperations(const cv::cuda::GpuMat& input, const cv::cuda::Stream& stream, const IOpTypes&... iops) {
    executeOperations<true>(input, stream, iops...);
}
// input and output GpuMat given: read prepended, per-pixel write appended
template <bool TF, typename... IOpTypes>
inline void executeOperations(const cv::cuda::GpuMat& input, cv::cuda::GpuMat& output, cv::cuda::Stream& stream, const IOpTypes&... iops) {
    using In = internal::first_input_t<IOpTypes...>;
    using Out = internal::last_output_t<IOpTypes...>;
    const fk::Read<fk::PerThreadRead<fk::_2D, In>> read{gpuMat2RawPtr2D<In>(input)};
    const fk::Write<fk::PerThreadWrite<fk::_2D, Out>> wr{gpuMat2RawPtr2D<Out>(output)};
    fk::executeOperations<TF>(cv::cuda::StreamAccessor::getStream(stream), read, iops..., wr);
}
template <typename... IOpTypes>
inline void executeOperations(const cv::cuda::GpuMat& input, cv::cuda::GpuMat& output, cv::cuda::Stream& stream, const IOpTypes&... iops) {
    executeOperations<true>(input, output, stream, iops...);
}
// batch reads
template <bool TF, size_t Batch, typename... IOpTypes>
inline void executeOperations(const std::array<cv::cuda::GpuMat, Batch>& input, const size_t& activeBatch, const cv::Scalar& defaultValue,
                              const cv::cuda::Stream& stream, const IOpTypes&... iops) {
    using In = internal::first_input_t<IOpTypes...>;
    fk::executeOperations<TF>(cv::cuda::StreamAccessor::getStream(stream), internal::batchRead<In>(input, activeBatch, defaultValue), iops...);
}
template <bool TF, size_t Batch, typename... IOpTypes>
inline void executeOperations(const std::array<cv::cuda::GpuMat, Batch>& input, const cv::cuda::Stream& stream, const IOpTypes&... iops) {
    using In = internal::first_input_t<IOpTypes...>;
    fk::executeOperations<TF>(cv::cuda::StreamAccessor::getStream(stream), internal::batchRead<In>(input, Batch, cv::Scalar()), iops...);
}
template <size_t Batch, typename... IOpTypes>
inline void executeOperations(const std::array<cv::cuda::GpuMat, Batch>& input, const size_t& activeBatch, const cv::Scalar& defaultValue,
                              const cv::cuda::Stream& stream, const IOpTypes&... iops) {
    executeOperations<true>(input, activeBatch, defaultValue, stream, iops...);
}
template <size_t Batch, typename... IOpTypes>
inline void executeOperations(const std::array<cv::cuda::GpuMat, Batch>& input, const cv::cuda::Stream& stream, const IOpTypes&... iops) {
    executeOperations<true>(input, stream, iops...);
}
// batch reads with a tensor output (one packed image per row of `output`)
template <bool TF, size_t Batch, typename... IOpTypes>
inline void executeOperations(const std::array<cv::cuda::GpuMat, Batch>& input, const size_t& activeBatch, const cv::Scalar& defaultValue,
                              const cv::cuda::GpuMat& output, const cv::Size& outputPlane, const cv::cuda::Stream& stream, const IOpTypes&... iops) {
    using In = internal::first_input_t<IOpTypes...>;
    using Out = internal::last_output_t<IOpTypes...>;
    const fk::Write<fk::PerThreadWrite<fk::_3D, Out>> wr{gpuMat2Tensor<Out>(output, outputPlane, 1).ptr()};
    fk::executeOperations<TF>(cv::cuda::StreamAccessor::getStream(stream), internal::batchRead<In>(input, activeBatch, defaultValue), iops..., wr);
}
template <bool TF, size_t Batch, typename... IOpTypes>
inline void executeOperations(const std::array<cv::cuda::GpuMat, Batch>& input, const cv::cuda::GpuMat& output, const cv::Size& outputPlane,
                              const cv::cuda::Stream& stream, const IOpTypes&... iops) {
    executeOperations<TF>(input, Batch, cv::Scalar(), output, outputPlane, stream, iops...);
}
template <size_t Batch, typename... IOpTypes>
inline void executeOperations(const std::array<cv::cuda::GpuMat, Batch>& input, const size_t& activeBatch, const cv::Scalar& defaultValue,
                              const cv::cuda::GpuMat& output, const cv::Size& outputPlane, const cv::cuda::Stream& stream, const IOpTypes&... iops) {
    executeOperations<true>(input, activeBatch, defaultValue, output, outputPlane, stream, iops...);
}
template <size_t Batch, typename... IOpTypes>
inline void executeOperations(const std::array<cv::cuda::GpuMat, Batch>& input, const cv::cuda::GpuMat& output, const cv::Size& outputPlane,
                              const cv::cuda::Stream& stream, const IOpTypes&... iops) {
    executeOperations<true>(input, output, outputPlane, stream, iops...);
}

// ---- CircularTensor --------------------------------------------------------------------------------------------------
// MIRRORED = true selects the opt-in mirrored-ring layout (engine extension; see include/cvgs_hip.h): data() then moves
// with every update instead of being stable, and an update costs one pass over the new frame only.  CAPTURABLE = true makes
// update() capturable into a HIP graph (engine extension: the update count lives on the device).
template <int I, int O, int COLOR_PLANES, int BATCH, fk::CircularTensorOrder CT_ORDER, fk::ColorPlanes CP_MODE = fk::ColorPlanes::Standard,
          bool MIRRORED = false, bool CAPTURABLE = false>
class CircularTensor : public fk::CircularTensor<CUDA_T(O), COLOR_PLANES, BATCH, CT_ORDER, CP_MODE, MIRRORED, CAPTURABLE> {
    using Base = fk::CircularTensor<CUDA_T(O), COLOR_PLANES, BATCH, CT_ORDER, CP_MODE, MIRRORED, CAPTURABLE>;
public:
    CircularTensor() = default;
    CircularTensor(const uint& width_, const uint& height_, const int& deviceID_ = 0) : Base(width_, height_, deviceID_) {}

    // new frame read per pixel from a GpuMat of type I
    template <typename... IOpTypes>
    void update(const cv::cuda::Stream& stream, const cv::cuda::GpuMat& input, const IOpTypes&... iops) {
        const fk::Read<fk::PerThreadRead<fk::_2D, CUDA_T(I)>> read{gpuMat2RawPtr2D<CUDA_T(I)>(input)};
        Base::update(cv::cuda::StreamAccessor::getStream(stream), read, iops...);
    }
    // first IOp is already a read (e.g. cvGS::resize(...)): "push with resize+normalize"
    template <typename... IOpTypes>
    void update(const cv::cuda::Stream& stream, const IOpTypes&... iops) {
        Base::update(cv::cuda::StreamAccessor::getStream(stream), iops...);
    }
    CUDA_T(O)* data() { return this->ptr_a.data; }
};

// ---- crops from a detector's device-side boxes (engine extension: cvgs_plane_tables_from_boxes, include/cvgs_hip_ext.h) ----------
// The second stage of a detection pipeline without the host in the loop: the boxes a network has just written on this GPU become a
// device plane table in ONE small kernel on the stream, and resize<T, INTER_LINEAR, AR>(deviceCrops, bg) reads that table like any other
// batched resize -- executeOperations, ChainBatch, recordTicks, graph capture.  update() copies nothing to the host and never synchronises.
//   cvGS::DeviceCrops crops(50);                                          // owns the table (and the rectangle buffer) of up to 50 boxes
//   crops.update(stream, frame, d_boxes, d_count, CVGS_BOX_XYXY_F32, cv::Size(64, 128));
//   cvGS::executeOperations(stream, cvGS::resize<CV_8UC3, cv::INTER_LINEAR>(crops), ..., cvGS::split<CV_32FC3>(tensor, cv::Size(64, 128)));
// Boxes are clamped into the frame; invalid boxes (NaN, empty, outside, at or beyond *d_count) give planes of the background value;
// rects() (device int32[maxBoxes][4]: x, y, w, h; zeros for an invalid box) maps results back to frame coordinates.
class DeviceCrops {
public:
    explicit DeviceCrops(int maxBoxes, bool withRects = true) : max_(maxBoxes) {
        if (maxBoxes < 1 || maxBoxes > 65535) throw std::runtime_error("cvGS::DeviceCrops: maxBoxes must be in [1, 65535]");
        void* p = nullptr;
        fk::hip_check(hipMalloc(&p, cvgs_plane_table_bytes(maxBoxes)), "hipMalloc(plane table)");
        table_ = std::shared_ptr<void>(p, [](void* q) { (void)hipFree(q); });
        if (withRects) {
            fk::hip_check(hipMalloc(&p, (size_t)maxBoxes * 4 * sizeof(int32_t)), "hipMalloc(rects)");
            rects_ = std::shared_ptr<void>(p, [](void* q) { (void)hipFree(q); });
        }
    }
    // enqueue the builder for ONE frame: `boxes` = device, maxBoxes x 4 floats (CVGS_BOX_XYXY_F32) or int32 (CVGS_BOX_XYWH_I32); `count` =
    // device int32 or nullptr (= maxBoxes).  The frame's type is taken from the GpuMat; dsize / ar must be those of the resize that reads it.
    void update(const cv::cuda::Stream& stream, const cv::cuda::GpuMat& frame, const void* boxes, const int32_t* count, cvgs_box_format format,
                const cv::Size& dsize, AspectRatio ar = IGNORE_AR) {
        const cvgs_box_table_desc d = describe(frame, boxes, count, format, dsize, ar);
        fk::detail::check_status(cvgs_plane_tables_from_boxes(&d, 1, cv::cuda::StreamAccessor::getStream(stream)));
    }
    // one frame's part of a several-camera update
    struct Job {
        DeviceCrops* crops;
        cv::cuda::GpuMat frame;
        const void* boxes;
        const int32_t* count;
    };
    // several DeviceCrops (the cameras of a tick) in ONE launch
    static void update(const cv::cuda::Stream& stream, const std::vector<Job>& jobs, cvgs_box_format format, const cv::Size& dsize,
                       AspectRatio ar = IGNORE_AR) {
        std::vector<cvgs_box_table_desc> d;
        d.reserve(jobs.size());
        for (const Job& j : jobs) {
            if (!j.crops) throw std::runtime_error("cvGS::DeviceCrops::update: null DeviceCrops");
            d.push_back(j.crops->describe(j.frame, j.boxes, j.count, format, dsize, ar));
        }
        fk::detail::check_status(cvgs_plane_tables_from_boxes(d.data(), (int32_t)d.size(), cv::cuda::StreamAccessor::getStream(stream)));
    }
    int maxBoxes() const { return max_; }
    const void* table() const { return table_.get(); }
    const int32_t* rects() const { return static_cast<const int32_t*>(rects_.get()); } // nullptr when built without
    // what the last update() described (the read built from it must agree)
    const cv::cuda::GpuMat& frame() const { return frame_; }
    cv::Size dsize() const { return dsize_; }
    AspectRatio aspectRatio() const { return ar_; }
private:
    cvgs_box_table_desc describe(const cv::cuda::GpuMat& frame, const void* boxes, const int32_t* count, cvgs_box_format format, const cv::Size& dsize,
                                 AspectRatio ar) {
        cvgs_box_table_desc d;
        std::memset(&d, 0, sizeof(d));
        d.struct_size = sizeof(d);
        d.frame = cvgs_image2d{frame.data, frame.cols, frame.rows, (int32_t)frame.step, 0};
        d.read_kind = CVGS_READ_RESIZE_LINEAR;
        d.src_type = frame.type();
        d.dst_width = dsize.width; d.dst_height = dsize.height; d.aspect_ratio = (int)ar;
        d.box_format = (int32_t)format; d.max_boxes = max_;
        d.boxes = boxes; d.count = count;
        d.table_out = table_.get(); d.rects_out = static_cast<int32_t*>(rects_.get());
        frame_ = frame; dsize_ = dsize; ar_ = ar;
        return d;
    }
    int max_;
    std::shared_ptr<void> table_, rects_;
    cv::cuda::GpuMat frame_;
    cv::Size dsize_;
    AspectRatio ar_ = IGNORE_AR;
};

// ---- the detector's raw candidates -> the boxes DeviceCrops reads (engine extension: cvgs_boxes_select, include/cvgs_hip_ext.h) --------
// Score threshold, top-K and greedy NMS on the device, in frame coordinates: two small kernels on the stream, nothing copied to the host.
//   cvGS::DeviceBoxSelect select(cv::Size(1920, 1080), 8400, 1024, 50);     // owns scratch and outputs for 8400 candidates, 50 boxes
//   select.candidates(d_head, 6, d_head + 4, 6);                            // a [8400, 6] head read in place: boxes, then scores
//   select.thresholds(0.25f, 0.45f).transform(sx, sy, ox, oy);              // detector input -> frame pixels
//   select.enqueue(stream);
//   crops.update(stream, frame, select.boxes(), select.count(), CVGS_BOX_XYXY_F32, cv::Size(64, 128));   // crops: DeviceCrops(50)
// The second constructor takes caller-owned buffers (scratch: cvgs_boxes_select_scratch_bytes) and allocates nothing.
class DeviceBoxSelect {
public:
    DeviceBoxSelect(const cv::Size& frameSize, int maxCandidates, int preNmsK, int maxOut, bool withScoresAndIndices = true) {
        init(frameSize, maxCandidates, preNmsK, maxOut);
        const size_t sb = cvgs_boxes_select_scratch_bytes(maxCandidates, preNmsK);
        if (!sb || maxOut < 1 || maxOut > preNmsK) throw std::runtime_error("cvGS::DeviceBoxSelect: maxCandidates in [1, 65535], preNmsK in [1, 1024], maxOut in [1, preNmsK]");
        d_.scratch = own(sb);
        d_.boxes_out = static_cast<float*>(own((size_t)maxOut * 4 * sizeof(float)));
        d_.count_out = static_cast<int32_t*>(own(sizeof(int32_t)));
        if (withScoresAndIndices) {
            d_.scores_out = static_cast<float*>(own((size_t)maxOut * sizeof(float)));
            d_.index_out = static_cast<int32_t*>(own((size_t)maxOut * sizeof(int32_t)));
        }
    }
    DeviceBoxSelect(const cv::Size& frameSize, int maxCandidates, int preNmsK, int maxOut, void* scratch, float* boxesOut, int32_t* countOut,
                    float* scoresOut = nullptr, int32_t* indexOut = nullptr) {
        init(frameSize, maxCandidates, preNmsK, maxOut);
        d_.scratch = scratch; d_.boxes_out = boxesOut; d_.count_out = countOut; d_.scores_out = scoresOut; d_.index_out = indexOut;
    }
    // where the candidates are (device pointers, strides in elements); classes == nullptr: class-agnostic suppression; count == nullptr: all
    DeviceBoxSelect& candidates(const float* boxes, int boxStride, const float* scores, int scoreStride, cvgs_cand_format format = CVGS_CAND_XYXY_F32,
                                const int32_t* classes = nullptr, int classStride = 1, const int32_t* count = nullptr) {
        d_.boxes = boxes; d_.box_stride = boxStride; d_.scores = scores; d_.score_stride = scoreStride; d_.box_format = (int32_t)format;
        d_.classes = classes; d_.class_stride = classStride; d_.count = count;
        return *this;
    }
    DeviceBoxSelect& thresholds(float score, float iou) { d_.score_threshold = score; d_.iou_threshold = iou; return *this; }
    DeviceBoxSelect& transform(float sx, float sy, float ox, float oy) { d_.xform[0] = sx; d_.xform[1] = sy; d_.xform[2] = ox; d_.xform[3] = oy; return *this; }
    void enqueue(const cv::cuda::Stream& stream) const { fk::detail::check_status(cvgs_boxes_select(&d_, 1, cv::cuda::StreamAccessor::getStream(stream))); }
    // several frames (the cameras of a tick, at most 16) in ONE call
    static void enqueue(const cv::cuda::Stream& stream, const std::vector<const DeviceBoxSelect*>& jobs) {
        std::vector<cvgs_box_select_desc> d;
        d.reserve(jobs.size());
        for (const DeviceBoxSelect* j : jobs) {
            if (!j) throw std::runtime_error("cvGS::DeviceBoxSelect::enqueue: null DeviceBoxSelect");
            d.push_back(j->d_);
        }
        fk::detail::check_status(cvgs_boxes_select(d.data(), (int32_t)d.size(), cv::cuda::StreamAccessor::getStream(stream)));
    }
    // what DeviceCrops::update accepts: maxOut x 4 floats (CVGS_BOX_XYXY_F32) and the count
    const void* boxes() const { return d_.boxes_out; }
    const int32_t* count() const { return d_.count_out; }
    const float* scores() const { return d_.scores_out; }   // nullptr when built without
    const int32_t* indices() const { return d_.index_out; } // nullptr when built without
    int maxOut() const { return d_.max_out; }
    const cvgs_box_select_desc& desc() const { return d_; }
private:
    void init(const cv::Size& frameSize, int maxCandidates, int preNmsK, int maxOut) {
        std::memset(&d_, 0, sizeof(d_));
        d_.struct_size = sizeof(d_);
        d_.frame_width = frameSize.width; d_.frame_height = frameSize.height;
        d_.max_candidates = maxCandidates; d_.pre_nms_k = preNmsK; d_.max_out = maxOut;
        d_.box_format = CVGS_CAND_XYXY_F32; d_.box_stride = 4; d_.score_stride = 1;
        d_.xform[0] = 1.f; d_.xform[1] = 1.f;
    }
    void* own(size_t bytes) {
        void* p = nullptr;
        fk::hip_check(hipMalloc(&p, bytes), "hipMalloc(box selection)");
        owned_.push_back(std::shared_ptr<void>(p, [](void* q) { (void)hipFree(q); }));
        return p;
    }
    cvgs_box_select_desc d_;
    std::vector<std::shared_ptr<void>> owned_;
};

// ---- the network's raw head -> the candidates DeviceBoxSelect reads (engine extension: cvgs_head_decode, include/cvgs_hip_ext.h) --------
// Best class, score, threshold and compaction on the device: two small kernels on the stream, the head read in place in fp32 / fp16 / bf16.
//   cvGS::DeviceHeadDecode decode(8400);                                    // owns scratch and outputs for 8400 candidates
//   decode.layout(d_head, CVGS_HEAD_BF16, 1, 8400, 80).threshold(0.25f);    // a [4 + 80, 8400] head: box 0..3, classes 4..83
//   decode.feed(select);                                                    // select.candidates(...) and its count from the outputs
//   decode.enqueue(stream); select.enqueue(stream);
// The second constructor takes caller-owned buffers (scratch: cvgs_head_decode_scratch_bytes) and allocates nothing.
class DeviceHeadDecode {
public:
    explicit DeviceHeadDecode(int maxCandidates, bool withIndices = true) {
        init(maxCandidates);
        const size_t sb = cvgs_head_decode_scratch_bytes(maxCandidates);
        if (!sb) throw std::runtime_error("cvGS::DeviceHeadDecode: maxCandidates in [1, 65535]");
        const size_t n = (size_t)maxCandidates;
        d_.scratch = own(sb);
        d_.boxes_out = static_cast<float*>(own(n * 4 * sizeof(float)));
        d_.scores_out = static_cast<float*>(own(n * sizeof(float)));
        d_.classes_out = static_cast<int32_t*>(own(n * sizeof(int32_t)));
        d_.count_out = static_cast<int32_t*>(own(sizeof(int32_t)));
        if (withIndices) d_.index_out = static_cast<int32_t*>(own(n * sizeof(int32_t)));
    }
    DeviceHeadDecode(int maxCandidates, void* scratch, float* boxesOut, float* scoresOut, int32_t* classesOut, int32_t* countOut, int32_t* indexOut = nullptr) {
        init(maxCandidates);
        d_.scratch = scratch; d_.boxes_out = boxesOut; d_.scores_out = scoresOut; d_.classes_out = classesOut; d_.count_out = countOut; d_.index_out = indexOut;
    }
    // where the head is (device pointer) and how it is laid out: attribute a of candidate i at element i * candStride + a * attrStride;
    // [N, A]: (A, 1), [A, N]: (1, N).  objAttr == -1: no objectness value
    DeviceHeadDecode& layout(const void* head, cvgs_head_elem elemType, int candStride, int attrStride, int numClasses, int boxAttr = 0, int classAttr = 4,
                             int objAttr = -1) {
        d_.head = head; d_.elem_type = (int32_t)elemType; d_.cand_stride = candStride; d_.attr_stride = attrStride; d_.num_classes = numClasses;
        d_.box_attr = boxAttr; d_.class_attr = classAttr; d_.obj_attr = objAttr;
        return *this;
    }
    DeviceHeadDecode& threshold(float score) { d_.score_threshold = score; return *this; }
    void enqueue(const cv::cuda::Stream& stream) const { fk::detail::check_status(cvgs_head_decode(&d_, 1, cv::cuda::StreamAccessor::getStream(stream))); }
    // several frames (the cameras of a tick, at most 16) in ONE call
    static void enqueue(const cv::cuda::Stream& stream, const std::vector<const DeviceHeadDecode*>& jobs) {
        std::vector<cvgs_head_desc> d;
        d.reserve(jobs.size());
        for (const DeviceHeadDecode* j : jobs) {
            if (!j) throw std::runtime_error("cvGS::DeviceHeadDecode::enqueue: null DeviceHeadDecode");
            d.push_back(j->d_);
        }
        fk::detail::check_status(cvgs_head_decode(d.data(), (int32_t)d.size(), cv::cuda::StreamAccessor::getStream(stream)));
    }
    // the selector reads this decoder's outputs: dense boxes (stride 4), scores, classes and the device count.  `format` is the head's
    // box format; the selector's maxCandidates must be this decoder's
    void feed(DeviceBoxSelect& select, cvgs_cand_format format = CVGS_CAND_XYXY_F32, bool classAware = true) const {
        if (select.desc().max_candidates != d_.max_candidates) throw std::runtime_error("cvGS::DeviceHeadDecode::feed: the selector's maxCandidates differs");
        select.candidates(d_.boxes_out, 4, d_.scores_out, 1, format, classAware ? d_.classes_out : nullptr, 1, d_.count_out);
    }
    const float* boxes() const { return d_.boxes_out; }
    const float* scores() const { return d_.scores_out; }
    const int32_t* classes() const { return d_.classes_out; }
    const int32_t* indices() const { return d_.index_out; } // nullptr when built without
    const int32_t* count() const { return d_.count_out; }
    int maxCandidates() const { return d_.max_candidates; }
    const cvgs_head_desc& desc() const { return d_; }
private:
    void init(int maxCandidates) {
        std::memset(&d_, 0, sizeof(d_));
        d_.struct_size = sizeof(d_);
        d_.max_candidates = maxCandidates;
        d_.elem_type = CVGS_HEAD_F32; d_.cand_stride = 1; d_.attr_stride = 1; d_.num_classes = 1; d_.class_attr = 4; d_.obj_attr = -1;
    }
    void* own(size_t bytes) {
        void* p = nullptr;
        fk::hip_check(hipMalloc(&p, bytes), "hipMalloc(head decode)");
        owned_.push_back(std::shared_ptr<void>(p, [](void* q) { (void)hipFree(q); }));
        return p;
    }
    cvgs_head_desc d_;
    std::vector<std::shared_ptr<void>> owned_;
};

// resize<T, INTER_LINEAR | INTER_AREA, AR>(deviceCrops, backgroundValue): the batched read over the device-built table -- maxBoxes planes of the size and
// aspect-ratio mode of the last update() (AR must be that mode), invalid boxes and the AR padding take backgroundValue.  fk::executeDivergentBatch
// keeps refusing device tables (it selects planes on the host).
template <int T, int INTER_F, AspectRatio AR_ = IGNORE_AR>
inline auto resize(const DeviceCrops& crops, const cv::Scalar& backgroundValue_ = cvScalar_set<CV_MAKETYPE(CV_32F, CV_MAT_CN(T))>(0)) {
    static_assert(isSupportedInterpolation<INTER_F>, "Interpolation type not supported yet.");
    const cv::cuda::GpuMat& f = crops.frame();
    if (!f.data) throw std::runtime_error("cvGS::resize(DeviceCrops): update() has not described a frame yet");
    if (f.type() != T) throw std::runtime_error("cvGS::resize(DeviceCrops): the frame of the last update() is not of type T");
    if (crops.aspectRatio() != AR_) throw std::runtime_error("cvGS::resize(DeviceCrops): AR differs from the mode the table was built with");
    fk::DeviceTableResizeRead<CUDA_T(T)> rd;
    rd.kind = fk::resize_read_kind<(fk::InterpolationType)INTER_F>; // cv::INTER_AREA reads the same table (built as RESIZE_LINEAR: one layout)
    rd.table = crops.table();
    rd.batch = crops.maxBoxes();
    rd.dsize = fk::Size(crops.dsize().width, crops.dsize().height);
    rd.ar = (int)AR_;
    for (int c = 0; c < CV_MAT_CN(T); ++c) rd.background[c] = static_cast<float>(backgroundValue_[c]);
    // the whole frame's byte range: cvgs_plane_table_hull of the one whole-frame view
    rd.src_lo = f.data;
    rd.src_hi = (const unsigned char*)f.data + (size_t)f.step * (size_t)(f.rows - 1) + (size_t)f.cols * f.elemSize();
    return rd;
}

// ---- the landmarks of kept detections -> the points DeviceWarps reads (engine extension: cvgs_points_gather, include/cvgs_hip_ext.h) ----
// The link between DeviceBoxSelect and DeviceWarps: one small kernel on the stream follows the selector's indices (through the decoder's)
// to the raw candidates, reads their landmarks from the head in place and maps them to frame pixels; nothing is copied to the host.
//   cvGS::DevicePointGather gather(8400, 50, 5);                            // owns the points of up to 50 detections, 5 landmarks each
//   gather.layout(d_head, CVGS_HEAD_BF16, 1, 8400, 5, 3).transform(sx, sy, ox, oy);   // a [4 + 1 + 5 * 3, 8400] head: x, y, conf from attribute 5
//   gather.from(select, decode);                                            // select.indices() / count(), decode.indices()
//   decode.enqueue(stream); select.enqueue(stream); gather.enqueue(stream);
//   faces.update(stream, frame, gather.points(), gather.count(), CVGS_WARP_FIT_SIMILARITY, arcface5, cv::Size(112, 112));
// The transform is the caller's: the selector's for a detector that reports edge coordinates; a detector that reports pixel-centre
// coordinates needs ox + 0.5 * sx - 0.5 (oy + 0.5 * sy - 0.5), since the warp kernels take integer coordinates as pixel centres.
// The second constructor takes caller-owned buffers and allocates nothing.
class DevicePointGather {
public:
    DevicePointGather(int maxCandidates, int maxOut, int nPoints, bool withConf = false, bool withSource = false) {
        init(maxCandidates, maxOut, nPoints);
        if (maxCandidates < 1 || maxCandidates > 65535 || maxOut < 1 || maxOut > 65535 || nPoints < 1 || nPoints > CVGS_GATHER_MAX_POINTS)
            throw std::runtime_error("cvGS::DevicePointGather: maxCandidates and maxOut in [1, 65535], nPoints in [1, 64]");
        const size_t items = (size_t)maxOut * (size_t)nPoints;
        d_.points_out = static_cast<float*>(own(items * 2 * sizeof(float)));
        if (withConf) d_.conf_out = static_cast<float*>(own(items * sizeof(float)));
        if (withSource) d_.source_out = static_cast<int32_t*>(own((size_t)maxOut * sizeof(int32_t)));
    }
    DevicePointGather(int maxCandidates, int maxOut, int nPoints, float* pointsOut, float* confOut = nullptr, int32_t* sourceOut = nullptr) {
        init(maxCandidates, maxOut, nPoints);
        d_.points_out = pointsOut; d_.conf_out = confOut; d_.source_out = sourceOut;
    }
    // where the head is (device pointer) and where its landmarks are: attribute a of candidate i at element i * candStride + a * attrStride,
    // x of point p at attribute pointAttr + p * pointStep, y at the next one, its confidence at + confOffset (-1: none; given exactly when
    // the object holds a confidence buffer)
    DevicePointGather& layout(const void* head, cvgs_head_elem elemType, int candStride, int attrStride, int pointAttr, int pointStep, int confOffset = -1) {
        d_.head = head; d_.elem_type = (int32_t)elemType; d_.cand_stride = candStride; d_.attr_stride = attrStride;
        d_.point_attr = pointAttr; d_.point_step = pointStep; d_.conf_offset = confOffset;
        return *this;
    }
    DevicePointGather& transform(float sx, float sy, float ox, float oy) { d_.xform[0] = sx; d_.xform[1] = sy; d_.xform[2] = ox; d_.xform[3] = oy; return *this; }
    // the selector ran over the head's own candidates: its indices are raw candidate indices
    DevicePointGather& from(const DeviceBoxSelect& select) {
        if (select.maxOut() != d_.max_out) throw std::runtime_error("cvGS::DevicePointGather::from: the selector's maxOut differs");
        if (select.desc().max_candidates != d_.max_candidates) throw std::runtime_error("cvGS::DevicePointGather::from: the selector's maxCandidates differs");
        if (!select.indices()) throw std::runtime_error("cvGS::DevicePointGather::from: the selector was built without indices");
        d_.kept_index = select.indices(); d_.kept_count = select.count(); d_.cand_index = nullptr;
        return *this;
    }
    // the selector ran over the decoder's compacted list: its indices map to raw candidates through the decoder's
    DevicePointGather& from(const DeviceBoxSelect& select, const DeviceHeadDecode& decode) {
        if (decode.maxCandidates() != d_.max_candidates) throw std::runtime_error("cvGS::DevicePointGather::from: the decoder's maxCandidates differs");
        if (!decode.indices()) throw std::runtime_error("cvGS::DevicePointGather::from: the decoder was built without indices");
        from(select);
        d_.cand_index = decode.indices();
        return *this;
    }
    void enqueue(const cv::cuda::Stream& stream) const { fk::detail::check_status(cvgs_points_gather(&d_, 1, cv::cuda::StreamAccessor::getStream(stream))); }
    // several frames (the cameras of a tick, at most 16) in ONE launch
    static void enqueue(const cv::cuda::Stream& stream, const std::vector<const DevicePointGather*>& jobs) {
        std::vector<cvgs_point_gather_desc> d;
        d.reserve(jobs.size());
        for (const DevicePointGather* j : jobs) {
            if (!j) throw std::runtime_error("cvGS::DevicePointGather::enqueue: null DevicePointGather");
            d.push_back(j->d_);
        }
        fk::detail::check_status(cvgs_points_gather(d.data(), (int32_t)d.size(), cv::cuda::StreamAccessor::getStream(stream)));
    }
    // what DeviceWarps::update accepts: maxOut x nPoints x 2 floats in frame pixels and the selector's count
    const float* points() const { return d_.points_out; }
    const int32_t* count() const { return d_.kept_count; }
    const float* conf() const { return d_.conf_out; }       // nullptr when built without
    const int32_t* source() const { return d_.source_out; } // nullptr when built without
    int maxOut() const { return d_.max_out; }
    int nPoints() const { return d_.n_points; }
    const cvgs_point_gather_desc& desc() const { return d_; }
private:
    void init(int maxCandidates, int maxOut, int nPoints) {
        std::memset(&d_, 0, sizeof(d_));
        d_.struct_size = sizeof(d_);
        d_.max_candidates = maxCandidates; d_.max_out = maxOut; d_.n_points = nPoints;
        d_.elem_type = CVGS_HEAD_F32; d_.cand_stride = 1; d_.attr_stride = 1; d_.point_attr = 5; d_.point_step = 2; d_.conf_offset = -1;
        d_.xform[0] = 1.f; d_.xform[1] = 1.f;
    }
    void* own(size_t bytes) {
        void* p = nullptr;
        fk::hip_check(hipMalloc(&p, bytes), "hipMalloc(point gather)");
        owned_.push_back(std::shared_ptr<void>(p, [](void* q) { (void)hipFree(q); }));
        return p;
    }
    cvgs_point_gather_desc d_;
    std::vector<std::shared_ptr<void>> owned_;
};

// ---- aligned crops from a detector's device-side landmarks (engine extension: cvgs_warp_tables_from_points, include/cvgs_hip_ext.h) ----
// Face alignment / oriented-box rectification without the host in the loop: the landmarks a network has just written on this GPU are
// fitted to a template in ONE small kernel on the stream, and warp<WT, T>(deviceWarps) reads the resulting device warp table like any
// other batched warp.  update() copies nothing to the host and never synchronises.
//   cvGS::DeviceWarps faces(64);                                         // owns the table (and the validity buffer) of up to 64 items
//   faces.update(stream, frame, d_landmarks, d_count, CVGS_WARP_FIT_SIMILARITY, arcface5, cv::Size(112, 112));
//   cvGS::executeOperations(stream, cvGS::warp<fk::WarpType::Affine, CV_8UC3>(faces), ..., cvGS::split<CV_32FC3>(tensor, cv::Size(112, 112)));
// Invalid items (a non-finite coordinate, coincident landmarks, at or beyond *d_count) give planes of 0 followed by the chain's program;
// valid() (device int32[maxItems], 1 / 0) says which.
class DeviceWarps {
public:
    explicit DeviceWarps(int maxItems, bool withValid = true) : max_(maxItems) {
        if (maxItems < 1 || maxItems > 65535) throw std::runtime_error("cvGS::DeviceWarps: maxItems must be in [1, 65535]");
        void* p = nullptr;
        fk::hip_check(hipMalloc(&p, cvgs_warp_table_bytes(maxItems)), "hipMalloc(warp table)");
        table_ = std::shared_ptr<void>(p, [](void* q) { (void)hipFree(q); });
        if (withValid) {
            fk::hip_check(hipMalloc(&p, (size_t)maxItems * sizeof(int32_t)), "hipMalloc(valid)");
            valid_ = std::shared_ptr<void>(p, [](void* q) { (void)hipFree(q); });
        }
    }
    // enqueue the builder for ONE frame: `points` = device float32 [maxItems][tmpl.size()][2] (x, y) in frame pixels; `count` = device int32
    // or nullptr (= maxItems); `tmpl` = the template in destination pixels (SIMILARITY: 2..16 points, AFFINE3: 3).  The frame's type is taken
    // from the GpuMat; the warp that reads the table may be affine or perspective.
    void update(const cv::cuda::Stream& stream, const cv::cuda::GpuMat& frame, const float* points, const int32_t* count, cvgs_warp_fit fit,
                const std::vector<cv::Point2f>& tmpl, const cv::Size& dsize) {
        if (tmpl.size() > (size_t)CVGS_WARP_MAX_POINTS) throw std::runtime_error("cvGS::DeviceWarps::update: a template holds at most 16 points");
        cvgs_warp_table_desc d;
        std::memset(&d, 0, sizeof(d));
        d.struct_size = sizeof(d);
        d.frame = cvgs_image2d{frame.data, frame.cols, frame.rows, (int32_t)frame.step, 0};
        d.src_type = frame.type();
        d.read_kind = CVGS_READ_WARP_AFFINE;
        d.dst_width = dsize.width; d.dst_height = dsize.height;
        d.fit = (int32_t)fit; d.n_points = (int32_t)tmpl.size();
        for (size_t i = 0; i < tmpl.size(); ++i) { d.tmpl[i][0] = tmpl[i].x; d.tmpl[i][1] = tmpl[i].y; }
        d.max_items = max_;
        d.points = points; d.count = count;
        d.table_out = table_.get(); d.valid_out = static_cast<int32_t*>(valid_.get());
        fk::detail::check_status(cvgs_warp_tables_from_points(&d, 1, cv::cuda::StreamAccessor::getStream(stream)));
        frame_ = frame; dsize_ = dsize;
    }
    // enqueue the box builder for ONE frame (cvgs_warp_tables_from_boxes): `boxes` = device float32 [maxItems][4] (xa, ya, xb, yb), edge
    // coordinates in frame pixels (DeviceBoxSelect's boxes); `count` = device int32 or nullptr.  Each box grows by `scale` and `pad` per
    // axis, its shorter side to dsize's aspect ratio (CVGS_BOX_SHAPE_EXPAND), and is sampled to dsize even where it leaves the frame (0
    // there).  `boxesOut` (optional, device float32 [maxItems][4]) receives the shaped rectangles, unclamped.
    void updateFromBoxes(const cv::cuda::Stream& stream, const cv::cuda::GpuMat& frame, const float* boxes, const int32_t* count, const cv::Size& dsize,
                         cvgs_box_shape shape = CVGS_BOX_SHAPE_EXPAND, const cv::Point2f& scale = cv::Point2f(1.25f, 1.25f),
                         const cv::Point2f& pad = cv::Point2f(0.f, 0.f), float* boxesOut = nullptr) {
        cvgs_box_warp_desc d;
        std::memset(&d, 0, sizeof(d));
        d.struct_size = sizeof(d);
        d.frame = cvgs_image2d{frame.data, frame.cols, frame.rows, (int32_t)frame.step, 0};
        d.src_type = frame.type();
        d.read_kind = CVGS_READ_WARP_AFFINE;
        d.dst_width = dsize.width; d.dst_height = dsize.height;
        d.shape = (int32_t)shape; d.max_items = max_;
        d.scale[0] = scale.x; d.scale[1] = scale.y; d.pad[0] = pad.x; d.pad[1] = pad.y;
        d.boxes = boxes; d.count = count;
        d.table_out = table_.get(); d.boxes_out = boxesOut; d.valid_out = static_cast<int32_t*>(valid_.get());
        fk::detail::check_status(cvgs_warp_tables_from_boxes(&d, 1, cv::cuda::StreamAccessor::getStream(stream)));
        frame_ = frame; dsize_ = dsize;
    }
    int maxItems() const { return max_; }
    const void* table() const { return table_.get(); }
    const int32_t* valid() const { return static_cast<const int32_t*>(valid_.get()); } // nullptr when built without
    // what the last update() described
    const cv::cuda::GpuMat& frame() const { return frame_; }
    cv::Size dsize() const { return dsize_; }
private:
    int max_;
    std::shared_ptr<void> table_, valid_;
    cv::cuda::GpuMat frame_;
    cv::Size dsize_;
};

// warp<WT, T>(deviceWarps[, defaultValue]): the batched warp over the device-built table -- maxItems planes of the size of the last update().
// fk::executeDivergentBatch keeps refusing warps and device tables.
template <fk::WarpType WT, int InputType = CV_8UC3>
inline auto warp(const DeviceWarps& warps, const cv::Scalar& defaultValue = cv::Scalar()) {
    const cv::cuda::GpuMat& f = warps.frame();
    if (!f.data) throw std::runtime_error("cvGS::warp(DeviceWarps): update() has not described a frame yet");
    if (f.type() != InputType) throw std::runtime_error("Input type does not match the input type of the operation.");
    fk::DeviceTableWarpRead<WT, CUDA_T(InputType)> rd;
    rd.table = warps.table();
    rd.batch = rd.used = warps.maxItems();
    rd.dsize = fk::Size(warps.dsize().width, warps.dsize().height);
    for (int c = 0; c < CV_MAT_CN(InputType); ++c) rd.background[c] = static_cast<float>(defaultValue[c]);
    rd.src_lo = f.data;
    rd.src_hi = (const unsigned char*)f.data + (size_t)f.step * (size_t)(f.rows - 1) + (size_t)f.cols * f.elemSize();
    return rd;
}

// ---- launch batching (engine extension, see fk::ChainBatch): several independent chains, ONE kernel launch -------------
class ChainBatch {
public:
    template <typename... IOps> void add(const IOps&... iops) { batch_.add(iops...); }
    void execute(const cv::cuda::Stream& stream) { batch_.execute(cv::cuda::StreamAccessor::getStream(stream)); }
    void clear() { batch_.clear(); }
    size_t size() const { return batch_.size(); }
private:
    fk::ChainBatch batch_;
};

// ---- device-side descriptor queue (engine extension, see fk::Queue): executeOperations without a launch per call -------
class Queue {
public:
    explicit Queue(int device = -1 /* the current device */, int depth = 0, double idle_us = 0.0) : q_(device, depth, idle_us) {}
    template <typename... IOps> uint64_t submit(const IOps&... iops) { return q_.submit(iops...); }
    void wait(uint64_t ticket, double timeout_s = 10.0) { q_.wait(ticket, timeout_s); }
    void wait(uint64_t ticket, const cv::cuda::Stream& consumer) { q_.wait(ticket, cv::cuda::StreamAccessor::getStream(consumer)); }
    uint64_t recover() { return q_.recover(); }
    fk::Queue& fk() { return q_; }
private:
    fk::Queue q_;
};
// The reference's own call shape on the queue: after attachQueue(stream, queue) every cvGS::executeOperations(stream, iops...) whose
// chain the server takes is submitted stream-ordered (behind the stream's earlier work, in front of its later work; no host
// synchronisation -- include/cvGPUSpeedup.cuh:464-473's contract), everything else is the ordinary launch.  The latency policy decides per
// call: one gate kernel per call is the price of stream order, so the server takes ChainBatch::execute(stream) ticks of >= 8 chains (2.5 us
// per 50-crop frame at 16 frames per tick against 8.9 us as launches) and single calls stay launches -- an attached stream is never slower
// than an unattached one (minGroup overrides the 8; 1 = always the server).  deferWait: the stream is not held on each batch;
// cvGS::fence(stream) orders the consumer (several batches of one stream then overlap on the device).
inline void attachQueue(const cv::cuda::Stream& stream, Queue& queue, bool deferWait = false, int minGroup = 0) {
    queue.fk().attach(cv::cuda::StreamAccessor::getStream(stream), deferWait, minGroup);
}
// Recorded ticks: the reference's loop UNCHANGED -- one cvGS::executeOperations(stream, ...) per camera, one stream.waitForCompletion() (or
// cvGS::fence(stream)) per tick -- on a stream attached with attachQueueTicks: the calls are recorded (0.14 us each) and go to the queue's
// server `tick` at a time behind one gate; waitForCompletion / fence submit what is pending first.  Sources and tensors of recorded calls
// are in flight until then (the deferred-wait contract).
inline void attachQueueTicks(const cv::cuda::Stream& stream, Queue& queue, int tick = 16) {
    queue.fk().attachTicks(cv::cuda::StreamAccessor::getStream(stream), tick);
}
// The same with NO queue: the recorded calls are launched `tick` at a time as ONE multi-chain kernel (cvgs_execute_many), strictly
// stream-ordered, nothing resident on the GPU between ticks.  stopRecording (or detachQueue) launches what is pending and ends it.
inline void recordTicks(const cv::cuda::Stream& stream, int tick = 16) { fk::recordTicks(cv::cuda::StreamAccessor::getStream(stream), tick); }
inline void stopRecording(const cv::cuda::Stream& stream) { fk::stopRecording(cv::cuda::StreamAccessor::getStream(stream)); }
inline void detachQueue(const cv::cuda::Stream& stream) { fk::Queue::detach(cv::cuda::StreamAccessor::getStream(stream)); }
inline void fence(const cv::cuda::Stream& stream) { fk::Queue::fence(cv::cuda::StreamAccessor::getStream(stream)); }
inline bool lastTicket(const cv::cuda::Stream& stream, uint64_t* ticket) { return fk::Queue::lastTicket(cv::cuda::StreamAccessor::getStream(stream), ticket); }
// cvGS::executeOperations(queue, iops...): the stream form's IOps, a ticket instead of a stream position
template <typename... IOpTypes>
inline uint64_t executeOperations(Queue& queue, const IOpTypes&... iops) {
    return queue.submit(iops...);
}

} // namespace cvGS
