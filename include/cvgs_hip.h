/*
 * cvgs_hip.h -- C-ABI of the MI355X-native fused image-preprocessing engine.
 *
 * This is the drop-in boundary for the hot path
 *     crop -> resize(bilinear) -> convertTo/normalize -> cvtColor -> split -> (Circular)Tensor
 * of Libraries-Openly-Fused/cvGPUSpeedup.  The reference has no FFI layer of its own: its
 * host/device boundary is the single call
 *     fk::executeOperations<TF>(cu_stream, iops...)          (reference include/cvGPUSpeedup.cuh:467)
 * into the (un-vendored) FusedKernelLibrary, with every operation parameter passed by value as a
 * kernel argument.  The entry points below are what a binding for that call would bind: the C++
 * facade (cvgpuspeedup_amd/include/cvGPUSpeedup.h, same cvGS:: names as the reference) pattern-
 * matches the compile-time operation list and lowers it to ONE cvgs_chain_desc, and
 * cvgs_execute() launches ONE hand-written HIP kernel (gfx950) for it.
 *
 * Plain C: pointers, sizes and POD structs only.  Every call is asynchronous on the given HIP
 * stream, never synchronises, and is thread-safe (CircularTensor handles excepted: they carry a
 * ring index, as in the reference, include/cvGPUSpeedup.cuh:600-627).  Device memory is only
 * allocated by cvgs_circular_create and cvgs_comm_*, plus one case inside cvgs_execute(_many): a batch
 * with more host descriptors than fit the kernel-argument block (64 planes in a 4 KB block; up to
 * CVGS_KERNARG_PLANES_MAX = 320 planes in a 16 KB block for the batched resize -> planar tensor chain,
 * the reference's benchmark sweep; 52 for warps, 16 destination planes) is written into a slot of a
 * library-owned pool of pinned host buffers (grown on first use, recycled by HIP event, never freed
 * per call) that the kernel reads in place; that case is refused during stream capture -- pass a
 * resident table (cvgs_plane_table_build).  A call whose descriptors travel in the
 * kernel arguments allocates nothing, on the host or on the device, and can be captured.
 *
 * Return value: 0 (CVGS_OK) or a negative cvgs_status; cvgs_last_error() gives a thread-local
 * human-readable message.  After a SUCCESSFUL cvgs_execute_many it holds a note instead: how
 * the tick was launched ("tick: ...", "not fused: <reason>") and, for captured ticks, how many
 * this process has captured beside their predecessor / in order (and, for a tick that was merged
 * into the previous tick's launch or was tried for it, how many were merged).
 */
#ifndef CVGS_HIP_H
#define CVGS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVGS_ABI_VERSION 6
#define CVGS_MAX_OPS 12        /* pointwise stages between the read and the write            */
#define CVGS_MAX_CHANNELS 4
#define CVGS_KERNARG_PLANES 64 /* planes whose descriptors travel inside the kernel arguments */
#define CVGS_KERNARG_PLANES_MAX 320 /* ... and for the batched resize -> planar tensor chain (K1), in a 16 KB argument block */
#define CVGS_MAX_MIRRORS 7     /* extra tensors one chain can write (the 7 peers of an 8-GPU node)  */
#define CVGS_MAX_CHAINS 128    /* chains one cvgs_execute_many launch can fuse                     */
/* Size limits (CVGS_ERR_UNSUPPORTED beyond them; the kernels index inside a row with 32-bit arithmetic): source planes and
 * output planes are at most 2^24 pixels wide and tall; the chroma plane of a 4:2:0 surface starts less than 2 GiB after its
 * luma plane.  Row pitches, plane strides and tensor sizes are 64-bit: a 288 GB tensor is addressable.              */
#define CVGS_MAX_DIM (1 << 24)

typedef void* cvgs_stream_t; /* hipStream_t (0 = the null stream) */

typedef enum cvgs_status {
    CVGS_OK = 0,
    CVGS_ERR_INVALID = -1,     /* malformed descriptor (the reference static_asserts / asserts) */
    CVGS_ERR_UNSUPPORTED = -2, /* well-formed but not implemented on this build                 */
    CVGS_ERR_HIP = -3,         /* a HIP runtime call failed (reference: gpuErrchk)              */
    CVGS_ERR_NO_DEVICE = -4,
    CVGS_ERR_RCCL = -5
} cvgs_status;

/* Element types use OpenCV's numeric encoding so that the cv2cuda shims (reference
 * include/cv2cuda_types.cuh:34-61) need no translation table:
 *   type = depth + ((channels-1) << 3),  depth: 8U=0 8S=1 16U=2 16S=3 32S=4 32F=5 64F=6 16F=7
 * CV_16F (IEEE binary16) is this engine's half-precision hand-off option (the reference has no
 * half type): a storage format only -- per-pixel read source, CAST target (round-to-nearest-even, overflow to
 * +-inf, like cv::saturate_cast<cv::float16_t>) and write type; arithmetic stages need a CAST to CV_32F (or CV_64F) first;
 * a CV_64F value becomes CV_16F through float (two roundings, like the double -> float -> half conversion it spells).
 * CV_16BF (bfloat16) is the second 16-bit float hand-off, for networks that run in bf16.  OpenCV's 3-bit depth field is
 * full, so it is spelled as depth 16F plus CVGS_TYPE_FLAG_BF16 (bit 12: outside OpenCV 4's CV_MAT_TYPE_MASK 0xFFF and below
 * its CONT / SUBMAT flags).  CVGS_TYPE_DEPTH still reads 7 (2 bytes per element) and CVGS_TYPE_CN masks the bit away.  It is
 * a storage format with CV_16F's contract, wherever CV_16F is accepted: per-pixel / resize / warp read source (widened to
 * fp32 exactly), CAST / CAST_TRUNC target (aux = CVGS_DEPTH_16BF; computed in fp32 and rounded once to nearest even,
 * overflow to +-inf, +-0, subnormals and infinities kept; a NaN stays a NaN, its sign and payload are unspecified; integer,
 * CV_64F (through float: two roundings) and CV_16F values get there through float) and write type.  Arithmetic stages and
 * GRAY on CV_16BF values: CVGS_ERR_UNSUPPORTED.  Other bits above the channel field keep their meaning (none).            */
#define CVGS_DEPTH_8U 0
#define CVGS_DEPTH_8S 1
#define CVGS_DEPTH_16U 2
#define CVGS_DEPTH_16S 3
#define CVGS_DEPTH_32S 4
#define CVGS_DEPTH_32F 5
#define CVGS_DEPTH_64F 6
#define CVGS_DEPTH_16F 7
#define CVGS_MAKETYPE(depth, cn) ((depth) + (((cn) - 1) << 3))
#define CVGS_TYPE_DEPTH(t) ((t) & 7)
#define CVGS_TYPE_CN(t) ((((t) >> 3) & 63) + 1)
#define CVGS_TYPE_FLAG_BF16 0x1000                            /* with depth 16F: the 16-bit float is bfloat16 */
#define CVGS_DEPTH_16BF (CVGS_DEPTH_16F | CVGS_TYPE_FLAG_BF16) /* also a valid CAST / CAST_TRUNC aux            */
#define CVGS_TYPE_IS_BF16(t) (((t) & CVGS_TYPE_FLAG_BF16) != 0)

/* A pitched 2D image view: replaces fk::RawPtr<fk::_2D,T> / fk::Ptr2D<T> as produced by
 * gpuMat2RawPtr2D / gpuMat2Ptr2D (reference include/cvGPUSpeedup.cuh:34-44).  A crop is a view:
 * data = frame + y*step + x*elemSize, same step (reference GpuMat::operator()(Rect),
 * tests/batchresize/test_batchresize_x_split3D.cu:284; cvGS::crop, include/cvGPUSpeedup.cuh:247). */
typedef struct cvgs_image2d {
    const void* data; /* device pointer to pixel (0,0)            */
    int32_t width;    /* pixels                                   */
    int32_t height;   /* rows (NV12: luma rows; UV plane follows) */
    int32_t step;     /* bytes between rows                       */
    /* NV12 kinds only: bytes from `data` to the interleaved UV row that belongs to luma row 0 of this view.
     * 0 = height * step (a whole surface: the UV plane directly below the luma plane).  A CROP of a surface at an
     * even (x, y) is then a view like any other: data = Y + y*step + x, uv_offset = (UV + (y/2)*step + x) - data. */
    int32_t uv_offset;
} cvgs_image2d;

/* ---- read stage (first IOp of the chain) ------------------------------------------------- */
typedef enum cvgs_read_kind {
    /* fk::PerThreadRead<_2D,T>, batched by fk::BatchRead<N,...> (cvGPUSpeedup.cuh:475-583)   */
    CVGS_READ_PIXEL = 0,
    /* fk::Resize<INTER_LINEAR,AR,fk::Read<PerThreadRead<_2D,T>>> wrapped in
     * fk::BatchRead<N,CONDITIONAL_WITH_DEFAULT> (cvGPUSpeedup.cuh:204-245)                    */
    CVGS_READ_RESIZE_LINEAR = 1,
    /* fk::ReadYUV<NV12> + fk::ConvertYUVToRGB<NV12,range,primaries,alpha,floatN>
     * (reference tests/resize/test_fused_resize.cu:50-51)                                     */
    CVGS_READ_NV12 = 2,
    /* the same pair fused as the BackIOp of fk::Resize<INTER_LINEAR>
     * (reference tests/resize/test_fused_resize.cu:141-143)                                   */
    CVGS_READ_NV12_RESIZE_LINEAR = 3,
    /* fk::Warping<fk::WarpType::Affine | Perspective, fk::Read<PerThreadRead<_2D,T>>>, batched like the resize
     * (cvGS::warp, cvGPUSpeedup.cuh:288-442; tests/warping/test_warping_opencv.cu).  For output pixel (x,y) the
     * source position is M*(x,y,1) (perspective: divided by its third component) with M = read.warp_matrices[z],
     * the INVERSE (destination -> source) transform narrowed to float exactly as fk::WarpingParameters holds it
     * (cvGPUSpeedup.cuh:269-284); inside the source [0,w) x [0,h) the value is the INTER_LINEAR interpolation of
     * the resize kinds, outside it is 0; the output type is CV_32F of the source's channels.  Every plane warps into
     * dst_width x dst_height, unless read.warp_dst_sizes gives each plane its own size (the reference's
     * std::array<cv::Size, BATCH> overloads, :381-401): then the write stage must hold one destination image per plane
     * (CVGS_WRITE_PIXEL_2D_BATCH / CVGS_WRITE_SPLIT_2D) of exactly that plane's size; dense tensors need equal sizes.  */
    CVGS_READ_WARP_AFFINE = 4,
    CVGS_READ_WARP_PERSPECTIVE = 5,
    /* INTER_AREA (box filter) resize: an ENGINE EXTENSION, the reference has INTER_LINEAR only.  For decimating crops: every source
     * pixel of the view is weighted by the share of it the output pixel covers, where the bilinear kind reads 2 x 2 of them.  Uses the
     * fields of CVGS_READ_RESIZE_LINEAR unchanged (src views or a device plane table, batch, used_planes, dst_width / dst_height,
     * aspect_ratio, background, table_src_lo / _hi); the value is CV_32F of the source's channels.  The plane table of an AREA chain is
     * BYTE FOR BYTE the table of the same chain spelled RESIZE_LINEAR (PlaneParams: fx, fy and the window x1..y2 of the aspect-ratio
     * mode): cvgs_plane_table_build / _bytes accept the kind, and a device table written by cvgs_plane_tables_from_boxes with
     * read_kind = CVGS_READ_RESIZE_LINEAR may be handed to an AREA chain.  cvgs_plane_table_hull of an AREA read is, per plane, the
     * whole view (first byte of the top row to one past the last byte of the bottom row): every pixel of a shrunk view is read; for a
     * non-shrinking axis it is a safe upper bound.
     * The arithmetic (the contract: strict fp32, no contraction, every operation rounded once, in this order).  Output pixel (x, y) of
     * plane z inside the window: tx = x - x1, ty = y - y1.  Each axis builds its tap list on its own; x is given, y is the same with
     * fy, ty, h.
     *   fx <= 1.0f (not shrinking): the bilinear taps.  s = (float)tx * fx, i0 = (int)floorf(s); tap 0 = (i0, (float)(i0 + 1) - s),
     *     tap 1 = (min(i0 + 1, w - 1), s - (float)i0); Wx = 1.0f by definition, not summed.
     *   fx > 1.0f (shrinking): a = (float)tx * fx, b = fminf((float)(tx + 1) * fx, (float)w), i0 = min((int)floorf(a), w - 1),
     *     i1 = max(min((int)ceilf(b), w), i0 + 1) (exclusive); for i = i0 .. i1-1 ascending wx_i = fminf((float)(i + 1), b) -
     *     fmaxf((float)i, a); if b <= a the single tap (i0, 1.0f); Wx = the fp32 sum of the wx_i, ascending, from 0.0f.
     *   pixel, per channel k: acc = 0.0f; for rows j ascending { row = 0.0f; for columns i ascending row = row + v(j,i,k) * wx_i;
     *     acc = acc + row * wy_j }; the result is acc * (1.0f / (Wx * Wy)).  v = the source sample as a float (exact for 8U, 8S, 16U,
     *     16S, 16F, 16BF; 32F as it is; 32S converted).
     * Outside the window: background; planes z >= used_planes: the default value, then the chain's program -- as for the bilinear kind.
     * A view shrunk by exactly 2 on both axes gives the exact mean of each 2 x 2 block; a view as large as its target reproduces it.
     * Served by cvgs_execute and by cvgs_execute_many.  cvgs_execute_many fuses independent chains of one shape into ONE launch when
     * they are the fast kernel's: 8U sources of 3 / 4 channels, a program without casts (but a trailing cast to 16F / 16BF), a planar
     * CVGS_WRITE_TENSOR_SPLIT / _T_SPLIT target of 32F / 16F / 16BF -- over host descriptors or device plane tables (stated hull or
     * vouched), bit-identical to one cvgs_execute per chain; a captured AREA tick is one kernel node in stream order.  Every other AREA
     * chain (other depths or channel counts, packed or per-plane targets, CVGS_CHAIN_FORCE_GENERIC, differing shapes, dependent chains)
     * runs one by one, in order, and cvgs_last_error() says why ("not fused: ...").  CVGS_ERR_UNSUPPORTED: CV_64F sources or values, mirrors,
     * the descriptor queue, cvgs_circular_update.  Decoder surfaces have an AREA kind of their own, CVGS_READ_NV12_RESIZE_AREA below.    */
    CVGS_READ_RESIZE_AREA = 6,
    /* 7: reserved (CVGS_ERR_INVALID) */
    /* INTER_AREA (box filter) resize of 4:2:0 DECODER SURFACES: an ENGINE EXTENSION.  For surfaces and crops that shrink by large factors
     * (a 6K surface into 1280 x 720, detections of a 4K surface into 64 x 128), where the 2 x 2 taps of CVGS_READ_NV12_RESIZE_LINEAR alias.
     * Uses the fields of CVGS_READ_NV12_RESIZE_LINEAR unchanged (views with uv_offset -- crops at even (x, y) -- or a device plane table,
     * batch, used_planes, dst_width / dst_height, aspect_ratio, background, yuv_range / yuv_primaries / yuv_alpha / yuv_layout,
     * table_src_lo / _hi); the value is that kind's: CV_32F with 3 or 4 channels, P010 on the 0..1023 scale.  Layouts: CVGS_YUV_NV12,
     * CVGS_YUV_NV21, CVGS_YUV_P010; I420, YV12, YUYV, UYVY and I444 are CVGS_ERR_UNSUPPORTED.  Unlike the bilinear kind a view may have an
     * ODD width or height (the last chroma sample then lies under one luma column / row only).  The plane table is BYTE FOR BYTE the table of
     * the same chain spelled NV12_RESIZE_LINEAR: cvgs_plane_table_build / _bytes accept the kind, and a device table built for the bilinear
     * NV12 kind -- by cvgs_plane_tables_from_boxes with read_kind = CVGS_READ_NV12_RESIZE_LINEAR too -- may be handed to an AREA chain
     * (cvgs_plane_tables_from_boxes called with THIS kind is CVGS_ERR_UNSUPPORTED, as for CVGS_READ_RESIZE_AREA).  cvgs_plane_table_hull is,
     * per plane, every luma byte of the view plus every chroma byte under it: ceil(h / 2) chroma rows of 2 * ceil(w / 2) samples.
     * The arithmetic (the contract: strict fp32, no contraction, every operation rounded once, in this order).  Per axis, x given, y the same
     * with fy, ty, h:
     *   luma axis: exactly the axis rule of CVGS_READ_RESIZE_AREA with n = the view's luma extent w: the taps (i, wx_i), their sum Wx, and
     *     the values a, b (shrinking) or s, i0 and the two weights w0, w1 (not shrinking).
     *   chroma axis, over nc = (w + 1) >> 1 samples.  Shrinking (fx > 1.0f): ac = a * 0.5f, bc = b * 0.5f, c0 = min((int)floorf(ac), nc - 1),
     *     c1 = max(min((int)ceilf(bc), nc), c0 + 1); for c = c0 .. c1-1 ascending wc = fminf((float)(c + 1), bc) - fmaxf((float)c, ac); if
     *     bc <= ac the single tap (c0, 1.0f); Wcx = the fp32 sum of the weights, ascending, from 0.0f -- the same box seen from the chroma
     *     grid: a chroma sample weighs half the luma area it sits under, and the last sample of an odd view gets its half weight by itself.
     *     Not shrinking: the two taps (i0 >> 1, w0), (min(i0 + 1, w - 1) >> 1, w1) with the luma weights, both kept, in this order, even when
     *     they name one sample; Wcx = 1.0f.
     *   values: Ym = the AREA loop nest over the luma codes (rows ascending, row = row + v * wx over columns ascending, acc = acc + row * wy)
     *     times 1.0f / (Wx * Wy); Um and Vm the same nest over the chroma taps of both axes times 1.0f / (Wcx * Wcy).  P010 codes are
     *     sample >> 6, taken before any weighting.
     *   conversion: (Ym, Um, Vm) go ONCE through the bilinear kind's per-tap conversion (cb = U - 128, cr = V - 128 -- 512 for P010 --,
     *     yv = (Y - ysub) * yscale, R = yv + rv * cr, G = (yv + gu * cb) + gv * cr, B = yv + bu * cb), then alpha, the window / background /
     *     default-value rules of the bilinear kind, then the chain's program.  The conversion is affine with no clamp: this equals "convert
     *     every pixel, then box-filter" in exact arithmetic and differs from it by rounding only.
     * A view as large as its target reproduces CVGS_READ_NV12's value; a view shrunk by exactly 2 converts the mean of each 2 x 2 luma block
     * with its one chroma sample.  Served by cvgs_execute and by cvgs_execute_many.  cvgs_execute_many fuses independent chains of one
     * shape into ONE launch when they are the fast kernel's: 8-bit NV12 / NV21 views, a program that keeps the CV_32F value and its channel
     * count (MUL / ADD / SUB / DIV / REORDER, and a trailing cast to 16F / 16BF), a planar CVGS_WRITE_TENSOR_SPLIT / _T_SPLIT target of
     * 32F / 16F / 16BF -- over device plane tables (stated hull or vouched), host descriptors in the kernel arguments (at most 1024 planes
     * in all) or the staged host table, bit-identical to one cvgs_execute per chain; a captured tick of this kind is one kernel node in
     * stream order.  Every other chain of this kind (P010, packed, u8 or per-plane targets, CVGS_CHAIN_FORCE_GENERIC, differing shapes,
     * dependent chains -- a view's chroma rows count) runs one by one, in order, and cvgs_last_error() says why ("not fused: ...").
     * CVGS_ERR_UNSUPPORTED, before anything is enqueued: CV_64F values, mirrors, the descriptor queue, cvgs_circular_update,
     * CVGS_WRITE_NV12 behind it.                                                                                                          */
    CVGS_READ_NV12_RESIZE_AREA = 8
} cvgs_read_kind;

/* same numeric values as cvGS::AspectRatio (reference include/cvGPUSpeedup.cuh:32) */
typedef enum cvgs_aspect_ratio {
    CVGS_PRESERVE_AR = 0,
    CVGS_IGNORE_AR = 1,
    CVGS_PRESERVE_AR_RN_EVEN = 2,
    CVGS_PRESERVE_AR_LEFT = 3
} cvgs_aspect_ratio;

typedef enum cvgs_yuv_range { CVGS_YUV_FULL = 0, CVGS_YUV_LIMITED = 1 } cvgs_yuv_range;
typedef enum cvgs_yuv_primaries { CVGS_BT601 = 0, CVGS_BT709 = 1, CVGS_BT2020 = 2 /* non-constant luminance */ } cvgs_yuv_primaries;
/* 4:2:0 layouts of the NV12 read kinds (the reference spells the reader as a template on the pixel format,
 * fk::ReadYUV<fk::NV12>, tests/resize/test_fused_resize.cu:50; NV12 is the only format its tests instantiate):
 *   NV12: interleaved chroma plane, U first;  NV21: the same, V first;
 *   I420: planar chroma, a (W/2) x (H/2) U plane with rows of step/2 bytes directly followed by the V plane; YV12: V plane first.
 * The chroma of luma row 0 starts uv_offset bytes after `data` (0 = height * step, the whole surface).  Crops
 * (uv_offset != 0) exist for the interleaved layouts only: a crop of a planar-chroma surface cannot say where its second
 * chroma plane starts (CVGS_ERR_UNSUPPORTED).
 *   P010: the 10-bit decoder surface -- NV12's geometry with 16-bit little-endian samples whose 10 significant bits are the
 *         MOST significant ones (code = sample >> 6); src_type is CV_16UC1, width / height in samples, step and uv_offset in
 *         BYTES.  The conversion works on the 10-bit codes (chroma centre 512, limited range 64..940 / 64..960) and delivers
 *         R, G, B on the 10-bit scale, 0..1023 (alpha = 1023): convertTo CV_16U for a 10-bit image, or scale by 1/1023 in
 *         the chain for a network input.                                                                             */
/* Packed 4:2:2 layouts (capture cards, V4L2 cameras, 4:2:2 JPEG decoders), accepted by both NV12 read kinds:
 *   YUYV: bytes Y0 U Y1 V per pixel pair (YUY2);  UYVY: bytes U Y0 V Y1 per pixel pair.
 * src_type is CV_8UC2; width / height in pixels, step in bytes; ONE plane, so uv_offset must be 0, and a row is a sequence of
 * 4-byte pixel pairs: data and step are multiples of 4 (CVGS_ERR_INVALID otherwise).  Width and height may be odd.
 * Pixel (x, y) has luma Y[y][x] and the chroma of its pair, U[y][x >> 1], V[y][x >> 1] -- the nearest-sample rule of the 4:2:0
 * layouts with full vertical chroma resolution; conversion (range, primaries, alpha, fp32 operation order) and the bilinear blend
 * are those of the 4:2:0 layouts, unchanged.  A crop is a plain view at an even x: data = frame + y*step + 2*x, any y, any
 * width >= 1, any height >= 1.  A view of odd width reads the whole last pair: the bytes a plane may read are
 * [0, 4 * ceil(width / 2)) of each of its rows, and nothing outside them is read; cvgs_plane_table_hull and the independence
 * check of cvgs_execute_many use that range.  Device plane tables: CVGS_ERR_UNSUPPORTED (a table carries no layout tag).  */
/* Planar 4:4:4 (I444: rocDecode's YUV444 surfaces of 4:4:4 HEVC / AV1 streams, rocJPEG's output for non-subsampled JPEGs), accepted
 * by both NV12 read kinds: three full-resolution planes Y, U, V that share `step`.
 * src_type is CV_8UC1; width / height in pixels, any value >= 1, odd included; step >= width; NO alignment requirement on data,
 * step or uv_offset.  `data` points at Y(0,0) of the view, uv_offset is the byte distance from Y(0,0) to U(0,0) of the same view,
 * and V(0,0) lies the same distance behind U(0,0): V = data + 2 * uv_offset.  A whole rocDecode surface: uv_offset = pitch *
 * aligned_height; a [3, H, W] tensor: step = stride(1), uv_offset = stride(0).  uv_offset must ALWAYS be stated -- there is no
 * "0 = height * step" default, a crop and a whole surface are described the same way: uv_offset == 0 and
 * uv_offset < (height - 1) * step + width (the planes of the view would overlap) are CVGS_ERR_INVALID, uv_offset > 2^30 is
 * CVGS_ERR_UNSUPPORTED.  A crop is a plain view at ANY (x, y, w, h): data = Y + y*step + x, uv_offset unchanged.
 * Pixel (x, y) is Y[y][x], U[y][x], V[y][x]; conversion (range, primaries, alpha, fp32 operation order) and the bilinear blend are
 * those of the 8-bit 4:2:0 layouts, unchanged: each tap is converted, then the taps are blended.  A plane reads the bytes
 * [0, width) of each of its `height` rows in each of the three planes, and nothing else; cvgs_plane_table_hull and the
 * independence check of cvgs_execute_many use [data, data + 2 * uv_offset + (height - 1) * step + width).  Device plane tables:
 * CVGS_ERR_UNSUPPORTED (a table carries no layout tag).                                                                          */
typedef enum cvgs_yuv_layout {
    CVGS_YUV_NV12 = 0, CVGS_YUV_NV21 = 1, CVGS_YUV_I420 = 2, CVGS_YUV_YV12 = 3, CVGS_YUV_P010 = 4,
    CVGS_YUV_YUYV = 5, /* bytes Y0 U Y1 V per pixel pair (YUY2, V4L2 YUYV) */
    CVGS_YUV_UYVY = 6, /* bytes U Y0 V Y1 per pixel pair                   */
    CVGS_YUV_I444 = 7  /* planar 4:4:4: full-resolution planes Y, U, V     */
} cvgs_yuv_layout;

#define CVGS_READ_FLAG_TABLE_ON_DEVICE 1u /* `src` is a device table made by cvgs_plane_table_build */
/* Device tables in cvgs_execute_many (ABI 6): the caller VOUCHES that nothing this table's planes read lies inside the output of another
 * chain of the same call -- for callers that rewrite their tables in place and cannot state table_src_lo / table_src_hi (below).        */
#define CVGS_READ_FLAG_TABLE_SOURCES_VOUCHED 2u

typedef struct cvgs_read_desc {
    int32_t kind;         /* cvgs_read_kind                                                   */
    int32_t src_type;     /* CV type of the source pixels (NV12: CVGS_MAKETYPE(8U,1))         */
    int32_t batch;        /* planes = grid z (std::array<GpuMat,N>::size())                   */
    int32_t used_planes;  /* planes >= used_planes produce `background` (usedPlanes/activeBatch) */
    const void* src;      /* host: cvgs_image2d[batch]; or device table (flag above)          */
    int32_t dst_width;    /* resize target; PIXEL/NV12 reads: ignored (= source size)         */
    int32_t dst_height;
    int32_t aspect_ratio; /* cvgs_aspect_ratio                                                */
    uint32_t flags;
    float background[4];  /* default value, already in the float type of the read's output    */
    int32_t yuv_range;    /* NV12 kinds only                                                  */
    int32_t yuv_primaries;
    int32_t yuv_alpha;    /* 1: 4-channel output with alpha = 255                             */
    int32_t yuv_layout;   /* cvgs_yuv_layout (0 = NV12)                                       */
    const float* warp_matrices; /* WARP kinds: host, batch x 9 floats (3x3 row-major; affine ignores row 2) */
    /* WARP kinds: host, batch x 2 ints (width, height) = the destination size of every plane (also of planes >= used_planes),
     * or NULL = dst_width x dst_height for all of them.                                                              */
    const int32_t* warp_dst_sizes;
    /* Device tables only (ABI 6): the byte range [table_src_lo, table_src_hi) that holds every byte the table's planes read (chroma rows of
     * 4:2:0 surfaces included), as cvgs_plane_table_hull computes it from the host descriptors the table was built from; NULL / NULL = not
     * stated.  The host cannot see into a device table: cvgs_execute_many compares THIS range with the other chains' outputs before it lets
     * the chains run concurrently in one launch.  A wider range (the whole frame) is always safe.  Ignored by every other call.            */
    const void* table_src_lo;
    const void* table_src_hi;
} cvgs_read_desc;

/* ---- pointwise stages (Unary / Binary IOps) ---------------------------------------------- */
typedef enum cvgs_opcode {
    CVGS_OP_NOP = 0,
    /* fk::SaturateCast<I,O> (cvGS::convertTo, cvGPUSpeedup.cuh:74-129). aux = destination depth. */
    CVGS_OP_CAST = 1,
    /* fk::Binary<fk::Mul/Add/Sub/Div<T>> (cvGS::multiply/add/subtract/divide,
     * cvGPUSpeedup.cuh:131-149); operand[c] = static_cast<float>(cv::Scalar[c])
     * (cvGPUSpeedupHelpers.cuh:38-54), operand_d[c] = the cv::Scalar value itself for CV_64F
     * types.  IEEE fp32 (fp64 on CV_64F values), applied in call order, never merged.  On integer-typed values (since ABI 4;
     * an ENGINE EXTENSION: the reference instantiates fk::Mul<uchar3> etc., whose semantics live in the un-vendored FKL and no
     * reference test uses): the scalar truncated and saturated to the pixel's own type, 64-bit integer arithmetic, division
     * truncating toward zero with x / 0 = 0, the result saturated back to the type; interpreted kernels only.  CV_16F values:
     * CVGS_ERR_UNSUPPORTED.                                                                                              */
    CVGS_OP_MUL = 2,
    CVGS_OP_ADD = 3,
    CVGS_OP_SUB = 4,
    CVGS_OP_DIV = 5,
    /* fk::VectorReorder / the channel-permuting fk::ColorConversion codes
     * (cvGS::cvtColor, cvGPUSpeedup.cuh:151-161).  aux = packed source indices,
     * 2 bits per output channel: out[c] = in[(aux >> 2c) & 3]; channel count unchanged.       */
    CVGS_OP_REORDER = 6,
    /* RGB->RGBA style: out[0..2] = in[(aux>>2c)&3], out[3] = operand[0] (type max). 3 -> 4 ch. */
    CVGS_OP_ADD_ALPHA = 7,
    /* RGBA->RGB style: out[c] = in[(aux>>2c)&3] for c < 3. 4 -> 3 channels.                    */
    CVGS_OP_DROP_ALPHA = 8,
    /* *2GRAY: 0.299 R + 0.587 G + 0.114 B, R = in[aux & 3], B = in[(aux>>4)&3]; integer depths
     * round to nearest even.  3|4 -> 1 channel.                                                */
    CVGS_OP_GRAY = 9,
    /* fk::Cast<I,O> (the reference's warp tests end with fk::Cast<float3,uchar3>, tests/warping/
     * test_warping_opencv.cu:63): static_cast per channel -- float -> integer TRUNCATES toward zero (values outside
     * the destination range, undefined in C++, saturate; NaN -> 0).  aux = destination depth.                  */
    CVGS_OP_CAST_TRUNC = 10
} cvgs_opcode;

typedef struct cvgs_op {
    int32_t opcode;
    int32_t aux;
    float operand[4];    /* operand narrowed to float: used while the value is CV_32F (or an integer depth)   */
    double operand_d[4]; /* the same operand in double: used by arithmetic stages on CV_64F values           */
} cvgs_op;

/* ---- write stage (last IOp of the chain) -------------------------------------------------- */
typedef enum cvgs_write_kind {
    /* fk::PerThreadWrite<_2D,T>: packed pixels into ONE pitched image (cvGS::write(GpuMat),
     * cvGPUSpeedup.cuh:449-452; executeOperations(in,out,...) :489-503).                      */
    CVGS_WRITE_PIXEL_2D = 0,
    /* fk::PerThreadWrite<_3D,T>: packed pixels, dense [plane][y][x] (cvGS::write(GpuMat,Size)
     * :454-457, write(fk::Tensor) :459-462).                                                  */
    CVGS_WRITE_PIXEL_3D = 1,
    /* fk::TensorSplit<T>: dense NCHW  out[z][c][y][x]  (cvGS::split(GpuMat,Size) :185-197)     */
    CVGS_WRITE_TENSOR_SPLIT = 2,
    /* fk::TensorTSplit<T>: dense CNHW out[c][z][y][x]  (cvGS::splitT :199-202)                 */
    CVGS_WRITE_TENSOR_T_SPLIT = 3,
    /* fk::SplitWrite<_2D,T>: C independent pitched planes per batch element
     * (cvGS::split(vector<GpuMat>) / (array<vector<GpuMat>,N>) :163-183)                       */
    CVGS_WRITE_SPLIT_2D = 4,
    /* fk::PerThreadWrite<_2D,T> per batch element: array of pitched images                     */
    CVGS_WRITE_PIXEL_2D_BATCH = 5,
    /* An 8-bit 4:2:0 ENCODER surface per plane, NV12 or NV21: an ENGINE EXTENSION, the reference writes pixels and tensors only.  The
     * chain converts to Y'CbCr, subsamples the chroma and stores the surface in the same launch that read and resized the picture: what a
     * pipeline that ends in a video encoder otherwise does in a second pass over a packed CV_8UC3 image.
     * Value.  The value reaching the write must be CV_32FC3 (dst_type), channels in the order R, G, B; a chain that carries BGR puts a
     *   CVGS_OP_REORDER in front.  Any other type: CVGS_ERR_INVALID.
     * Target.  write.planes2d = host cvgs_image2d[read.batch], one surface per plane, as for PIXEL_2D_BATCH.  data = Y(0,0); step in bytes,
     *   >= width; uv_offset = bytes from data to the chroma row of luma row 0, 0 = height * step (the meaning it has on the read side: a
     *   crop of a larger surface at an even origin is a target like any other).  width and height must equal the size the read stage
     *   produces and must be even (CVGS_ERR_INVALID otherwise, like the NV12 read).
     * Colour parameters.  write.yuv_params (the int32 that was `reserved` until this kind existed; every other kind ignores it):
     *   bits 0-3 cvgs_yuv_range, bits 4-7 cvgs_yuv_primaries, bits 8-11 the layout, CVGS_YUV_NV12 or CVGS_YUV_NV21 only
     *   (CVGS_WRITE_YUV_PARAMS below); all other bits zero.
     * Arithmetic (the contract: strict fp32, no contraction, every operation rounded once, in this order).  Per pixel:
     *     y = (Kr*R + Kg*G) + Kb*B;   cb = (B - y) * cu;   cr = (R - y) * cv
     *   full range:    Y = y,            U = cb + 128,       V = cr + 128
     *   limited range: Y = y * sy + 16,  U = cb * sc + 128,  V = cr * sc + 128
     *   Kr, Kg, Kb = the luma weights of BT.601 (0.299, 0.587, 0.114), BT.709 (0.2126, 0.7152, 0.0722), BT.2020 NCL (0.2627, 0.678, 0.0593);
     *   cu = 0.5 / (1 - Kb), cv = 0.5 / (1 - Kr); sy = 219/255, sc = 224/255 -- all as 6-decimal fp32 literals:
     *     BT.601  cu 0.564334 cv 0.713267;  BT.709  cu 0.538909 cv 0.635001;  BT.2020  cu 0.531519 cv 0.678150;  sy 0.858824  sc 0.878431
     *   The luma byte of pixel (x, y) is Y under the CVGS_OP_CAST-to-8U rule: round to nearest even, saturate to 0..255 (NaN -> 0).
     *   The chroma pair of the 2 x 2 block (bx, by) comes from the four FLOAT U and V values of its pixels, nothing rounded in between:
     *     Ub = ((U(2bx,2by) + U(2bx+1,2by)) + (U(2bx,2by+1) + U(2bx+1,2by+1))) * 0.25f, Vb the same with V; each rounded by the same rule
     *   and stored at data + uv_offset + by*step + 2*bx as (Ub, Vb) for NV12, (Vb, Ub) for NV21.
     * Bytes written.  A plane writes the bytes [0, width) of each of its `height` luma rows and of its height/2 chroma rows, and nothing
     *   else: row padding stays untouched.  Planes z >= used_planes run the background value through the chain and are written like any other.
     * Served by cvgs_execute -- read kinds CVGS_READ_PIXEL, CVGS_READ_RESIZE_LINEAR, CVGS_READ_NV12, CVGS_READ_NV12_RESIZE_LINEAR with every
     *   source type and layout they take, host views or a device plane table, any fp32 program -- and one by one by cvgs_execute_many.
     *   CVGS_ERR_UNSUPPORTED: CV_64F values, mirrors, warp reads, CVGS_READ_RESIZE_AREA, CVGS_READ_NV12_RESIZE_AREA, the descriptor queue,
     *   cvgs_circular_update.
     * Transcoding a surface at its own size with the same range and primaries in and out returns it byte for byte.                       */
    CVGS_WRITE_NV12 = 6
} cvgs_write_kind;

/* cvgs_write_desc.yuv_params of a CVGS_WRITE_NV12 chain */
#define CVGS_WRITE_YUV_PARAMS(range, primaries, layout) (((range) & 15) | (((primaries) & 15) << 4) | (((layout) & 15) << 8))
#define CVGS_WRITE_YUV_RANGE(p) ((p) & 15)
#define CVGS_WRITE_YUV_PRIMARIES(p) (((p) >> 4) & 15)
#define CVGS_WRITE_YUV_LAYOUT(p) (((p) >> 8) & 15)

typedef struct cvgs_write_desc {
    int32_t kind;     /* cvgs_write_kind                                                       */
    int32_t dst_type; /* CV type of the value being written (depth + channels)                 */
    void* data;       /* tensor kinds and PIXEL_2D: device pointer                             */
    int32_t width;    /* plane width  (pixels)                                                 */
    int32_t height;   /* plane height (rows)                                                   */
    int32_t step;     /* PIXEL_2D: row pitch in bytes; tensor kinds: ignored (dense)           */
    int32_t planes;   /* tensor kinds: number of images N in the tensor (>= read.batch)        */
    /* SPLIT_2D: host array cvgs_image2d[batch*channels], index z*channels+c.
     * PIXEL_2D_BATCH: host array cvgs_image2d[batch].
     * NV12: host array cvgs_image2d[batch], the luma views with their uv_offset.              */
    const cvgs_image2d* planes2d;
    /* Tensor kinds (TENSOR_SPLIT / TENSOR_T_SPLIT / PIXEL_3D) only: n_mirrors (<= CVGS_MAX_MIRRORS) further device
     * tensors of the same shape that receive the SAME values at the same element offsets as `data`, in the same kernel
     * (host array of device pointers; NULL / 0 = none).  This is the exchange step of the sharded batched-crop path
     * (SURVEY.md 8e option 2, BASELINE cfg #5): rank r's kernel stores its rows of the [N,C,H,W] tensor into its own
     * copy AND into every peer's copy through P2P-mapped pointers (include/cvgs_rccl.h: cvgs_ipc_* /
     * cvgs_peer_enable), so no separate all-gather moves the data a second time.  No reference counterpart.        */
    void* const* mirrors;
    int32_t n_mirrors;
    int32_t yuv_params; /* CVGS_WRITE_NV12: CVGS_WRITE_YUV_PARAMS(range, primaries, layout); ignored by every other kind */
} cvgs_write_desc;

/* ---- the fused chain = one kernel launch --------------------------------------------------- */
typedef struct cvgs_chain_desc {
    uint32_t struct_size; /* sizeof(cvgs_chain_desc), for ABI checking */
    uint32_t flags;       /* cvgs_chain_flags                          */
    cvgs_read_desc read;
    int32_t n_ops;
    int32_t reserved;
    cvgs_op ops[CVGS_MAX_OPS];
    cvgs_write_desc write;
} cvgs_chain_desc;

typedef enum cvgs_chain_flags {
    CVGS_CHAIN_DEFAULT = 0,
    /* force the interpreted generic kernel even when a specialised kernel matches (testing)   */
    CVGS_CHAIN_FORCE_GENERIC = 1,
    /* ENABLE_THREAD_FUSION=false of the reference (cvGPUSpeedup.cuh:464): results identical,
     * only disables the multi-pixel-per-thread fast paths.  A tuning / testing knob: the C++
     * facade does not forward executeOperations<false> (the hint exists in the reference because
     * its thread-fused path does not cover every type; here it would only pick a slower kernel) */
    CVGS_CHAIN_NO_THREAD_FUSION = 2
    /* every other bit must be zero (CVGS_ERR_INVALID) */
} cvgs_chain_flags;

/* Library / device ------------------------------------------------------------------------- */
int cvgs_abi_version(void);
const char* cvgs_version_string(void);
const char* cvgs_last_error(void);
/* number of visible HIP devices, or a negative status */
int cvgs_device_count(void);

/* Replaces fk::executeOperations<TF>(stream, iops...) (reference include/cvGPUSpeedup.cuh:467,
 * 480,495,513,524,552,566): validates the chain and enqueues exactly one kernel on `stream`.   */
int cvgs_execute(const cvgs_chain_desc* chain, cvgs_stream_t stream);

/* n_chains INDEPENDENT chains -- distinct source frames, crop lists and output tensors -- in as few launches as
 * possible.  A 50-crop chain moves ~9 MB, about 1 us of HBM time behind a ~1.8 us launch/drain floor;
 * a serving loop with several cameras amortises that floor by submitting its frames together.  Chains whose read is
 * a bilinear resize of 8U/16U/16S/32F pixels, or of NV12 / NV21 surfaces or crops of them (host descriptors), into a planar
 * fp32 / fp16 tensor (the K1 / K4 shapes) -- or, since round 6, a per-pixel read of 8U planes of ONE size (host descriptors) through an fp32 program into a
 * dense fp32 tensor / packed pixels (the reference's batched pointwise chains, tests/batchread/test_batchread_x_write3D.cu:92-96), or an INTER_AREA
 * resize of 8U pixels with 3 / 4 channels, or of 8-bit NV12 / NV21 surfaces or crops of them, into a planar fp32 / fp16 / bf16 tensor
 * (CVGS_READ_RESIZE_AREA, CVGS_READ_NV12_RESIZE_AREA; host descriptors or device tables), or an affine / perspective warp of 8U pixels
 * with 3 / 4 channels into a planar fp32 / fp16 / bf16 tensor (CVGS_READ_WARP_AFFINE / _PERSPECTIVE with one target size, no
 * warp_dst_sizes; device warp tables, or host descriptors of at most 256 planes in all, which travel in the kernel arguments -- more run
 * one by one) --, and that agree in
 * everything except read.src / batch / used_planes and write.data / planes (same source type, target size,
 * aspect-ratio mode, background, YUV range / primaries / layout, pointwise stages and operands, write kind and type), are
 * fused into ONE launch of the K1 (or K4, pointwise, AREA, warp) kernel: grid z = chain, grid y = crop.  Results are bit-identical to n_chains separate cvgs_execute calls (same
 * kernel code; tests/test_gpu_many.py).  Any other set of chains is executed one by one, in order -- and so is a set whose
 * chains are NOT independent (two chains write overlapping bytes, or a source view of one -- chroma rows of a 4:2:0
 * surface included -- lies inside another's output: fused chains run concurrently; chains whose plane table lives on the device are checked
 * through the source range they state, read.table_src_lo / table_src_hi from cvgs_plane_table_hull, and a device-table chain that states
 * none runs one by one unless it carries CVGS_READ_FLAG_TABLE_SOURCES_VOUCHED -- ABI 6; until ABI 5 such chains were fused unchecked),
 * a set with a batch beyond 65535, and staged host descriptors under stream capture.  Host
 * descriptors of fused 8-bit chains -- pixels with 3 / 4 channels, or crops of NV12 / NV21 surfaces -- with at most 1024 planes in all (a tick of
 * 16 cameras x 50 crops is 800) travel
 * INSIDE the fused launch's kernel arguments (a 16 KB block up to 256 planes, 52 KB beyond): nothing is staged, nothing is recycled, the
 * call allocates nothing and can be captured as it is; the kernel reads them from device memory (the runtime's argument pool) instead of
 * fetching a pinned table over PCIe (eager tick of 16 x 50 crops: 40.9 -> 39.9 us; the host pays 1-5 us more per call for the larger
 * argument block).  Every other fused launch with host
 * descriptors writes them into a pinned buffer of the stream's own ring that the kernel reads in place (no copy; round 5:
 * the fused kernel itself stores the stream's progress into a pinned word when it starts, and a slot is recycled once that word has reached
 * its launch -- no HIP event behind the launch; a host 8 such launches ahead of ONE stream waits for the oldest of them, at most a few
 * milliseconds, then falls back to the event-tracked descriptor scratch; a stream handle the runtime hands out again after
 * hipStreamDestroy continues the old ring: destroy a stream only once its fused launches have finished); pass device plane tables to
 * make such a fused call capturable; at most
 * CVGS_MAX_CHAINS chains per call.  The reference's closest spelling is the batch sweep of
 * tests/batchresize/test_batchresize_x_split3D.cu:384-392 (one launch per BATCH value).
 * On a CAPTURING stream a K1 tick over device tables may add no kernel node at all: when it follows this library's previous tick of the
 * same capture directly, launches the same kernel over an equal argument block and is proven independent of it from the stated ranges, its
 * chains join that tick's node (gridDim.z grows; up to CVGS_MAX_CHAINS chains per node; CVGS_TICK_MERGE=0 keeps one node per tick).  The
 * node is then this library's: do not change its parameters.  DESIGN.md section 5.                                                       */
int cvgs_execute_many(const cvgs_chain_desc* chains, int32_t n_chains, cvgs_stream_t stream);

/* Call before destroying a stream that has carried cvgs_execute_many calls with host descriptors: waits for the stream's work
 * (hipStreamSynchronize -- the stream is about to go anyway) and retires the table ring and progress word the library keeps for that stream
 * HANDLE, so that a later stream the runtime creates with the same handle starts from a clean state and the pinned tables are freed
 * (hipStreamDestroy does not wait for pending work, and the ring is keyed by the handle).  A no-op (CVGS_OK) for streams the
 * library holds nothing for; the C++ facade's cv::cuda::Stream calls it from its destructor.  No reference counterpart.               */
int cvgs_stream_release(cvgs_stream_t stream);

/* Validation only (what the reference checks with static_assert / assert / runtime_error).    */
int cvgs_validate(const cvgs_chain_desc* chain);

/* Name of the kernel cvgs_execute would launch for this chain ("k1_u8c3_swap_mul_sub_div", "generic_inline8", ...)
 * written into buf (NUL terminated).  Introspection for tests and profiles.                    */
int cvgs_kernel_name(const cvgs_chain_desc* chain, char* buf, size_t buf_size);

/* Plane tables: for batches larger than CVGS_KERNARG_PLANES, or when the caller keeps the crop
 * list resident in HBM, the per-plane read parameters live in a device buffer instead of the
 * kernel arguments (the reference is limited to ~50 planes by the 4 KB kernel-parameter block,
 * tests/batchresize/test_batchresize_aspectratio_x_split3D.cu:21-23).  `read->src` must be a
 * host cvgs_image2d[batch]; the function writes cvgs_plane_table_bytes(batch) bytes of
 * position-independent table into host_out, which the caller copies to the device and passes
 * back as read.src with CVGS_READ_FLAG_TABLE_ON_DEVICE.                                         */
size_t cvgs_plane_table_bytes(int32_t batch);
/* A table is bound to the 4:2:0 layout it was built (and validated) with: executing it with another read.yuv_layout is
 * refused for the layouts whose per-plane preconditions differ (P010, I420, YV12: CVGS_ERR_UNSUPPORTED with device tables). */
int cvgs_plane_table_build(const cvgs_read_desc* read, void* host_out);
/* The byte range [*lo, *hi) that holds everything the planes of `read` (host cvgs_image2d[batch], as for cvgs_plane_table_build) read:
 * what a chain that passes the built table states in read.table_src_lo / table_src_hi so that cvgs_execute_many can check it (ABI 6).   */
int cvgs_plane_table_hull(const cvgs_read_desc* read, const void** lo, const void** hi);

/* ---- CircularTensor ------------------------------------------------------------------------
 * Replaces fk::CircularTensor<T,COLOR_PLANES,BATCH,ORDER,CP_MODE> as wrapped by
 * cvGS::CircularTensor (reference include/cvGPUSpeedup.cuh:600-627).                            */
typedef struct cvgs_circular_s* cvgs_circular_t;

typedef enum cvgs_circular_order { CVGS_NEWEST_FIRST = 0, CVGS_OLDEST_FIRST = 1 } cvgs_circular_order;
typedef enum cvgs_color_planes_mode { CVGS_PLANES_STANDARD = 0, CVGS_PLANES_TRANSPOSED = 1 } cvgs_color_planes_mode;

/* elem_type: CV type of ONE tensor element (CV_32FC1 for split tensors, CV_32FC4 for packed).
 * Allocates the output tensor and the internal ring on `device_id` (ctor/Alloc, :605-610).     */
int cvgs_circular_create(cvgs_circular_t* out, int32_t width, int32_t height, int32_t elem_type,
                         int32_t color_planes, int32_t batch, int32_t order, int32_t cp_mode,
                         int32_t device_id);
/* Opt-in variant ("mirrored ring"): the tensor lives in a ring of 2*BATCH image slots and every
 * new frame is written to slot p and to slot p+BATCH, so the BATCH most recent frames are ALWAYS contiguous and in
 * order somewhere in the ring.  An update then costs one fused pass over the new frame (two stores per element) and
 * NO shift traffic: ~50 MB instead of ~800 MB per update at cfg #4.  The price is the API break the reference
 * cannot make: cvgs_circular_data() MOVES with every update (call it after each update), and only the Standard
 * plane order (N,C,H,W) exists.  Tensor contents at data() are identical to the default mode's.                */
#define CVGS_CIRCULAR_MIRRORED 1u
/* CVGS_CIRCULAR_CAPTURABLE: cvgs_circular_update may be captured into a HIP graph (the reference's update is an ordinary stream
 * launch, include/cvGPUSpeedup.cuh:612-622; a serving loop that replays graphs needs it inside them).  The update count then
 * lives in device memory; per-pixel pushes (the form the reference tests) stay ONE fused launch that derives its ring slot from
 * that count, pushes with a resize / NV12 / warp read go through a staging image and a device-indexed shift (one extra pass over
 * ONE image); N captured updates replay as the NEXT N updates.  cvgs_circular_updates() and, for mirrored
 * handles, cvgs_circular_data() read the device-side count and therefore synchronise the device.                        */
#define CVGS_CIRCULAR_CAPTURABLE 2u
int cvgs_circular_create_ex(cvgs_circular_t* out, int32_t width, int32_t height, int32_t elem_type,
                            int32_t color_planes, int32_t batch, int32_t order, int32_t cp_mode,
                            int32_t device_id, uint32_t flags);
/* update(stream, [GpuMat,] iops..., write) (:612-622): `chain` carries the read stage (batch 1),
 * the pointwise stages and the write KIND (TENSOR_SPLIT / TENSOR_T_SPLIT / PIXEL_3D); the write
 * target is the handle's own tensor (write.data is ignored).  The new frame is computed ONCE and stored both into
 * its slot of the ordered tensor and into the history ring, and the BATCH-1 older frames move from the ring to their
 * new slots.  Per-pixel u8 pushes (the form the reference tests) do all of it in ONE kernel launch; pushes with a
 * resize / NV12 / warp read use the chain's own kernel plus one plane-copy kernel (mirrored handles: no copy at all).
 * A default handle cannot be captured into a HIP graph (its ring index is host state): CVGS_ERR_UNSUPPORTED on a capturing
 * stream; handles created with CVGS_CIRCULAR_CAPTURABLE can (above).                                                */
int cvgs_circular_update(cvgs_circular_t ct, const cvgs_chain_desc* chain, cvgs_stream_t stream);
/* data() (:624-626): device pointer of the ordered output tensor; stable for the handle's life
 * (mirrored handles: the window of the LAST update -- it moves).                                 */
void* cvgs_circular_data(cvgs_circular_t ct);
size_t cvgs_circular_bytes(cvgs_circular_t ct);
/* number of updates so far (the reference keeps this host-side ring index private)             */
int64_t cvgs_circular_updates(cvgs_circular_t ct);
int cvgs_circular_destroy(cvgs_circular_t ct);

/* ---- streaming copy ----------------------------------------------------------------------------
 * dst[0..bytes) <- src[0..bytes) with the CircularTensor's plane-copy kernel (non-temporal 16-byte accesses), asynchronous
 * on `stream`.  No reference equivalent: it is the on-box "streaming kernel" copy ceiling SURVEY.md 8(d) asks the
 * roofline fractions to be quoted against (bench.py), and a utility for callers that re-pack tensors.  The two
 * ranges must not overlap.                                                                                      */
int cvgs_stream_copy(void* dst, const void* src, size_t bytes, cvgs_stream_t stream);

/* ---- profiling ranges (reference tests/nvtx.h PUSH_RANGE/POP_RANGE) -------------------------- */
void cvgs_range_push(const char* name);
void cvgs_range_pop(void);

#ifdef __cplusplus
}
#endif
#endif /* CVGS_HIP_H */
