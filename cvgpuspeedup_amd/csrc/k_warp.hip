// k_warp.hip -- cvGS::warp: affine / perspective warping fused in front of a pointwise chain and a write stage
// (reference include/cvGPUSpeedup.cuh:288-442 -> fk::Warping<WT, Read<PerThreadRead<_2D,T>>>, batched with
// usedPlanes / default value like the resize; tests/warping/test_warping_opencv.cu).  SURVEY.md 8(f)4.
// One thread = one output pixel of plane z: destination (x,y) -> source position through the inverse transform
// (strict fp32, products and sums in the written order, IEEE division), INTER_LINEAR taps as in the resize, zero
// outside the source.  Interpreted program and generic write stage: this is not a hot-path kernel.
#include <memory>
#include <type_traits>

#include "k_taps.hpp"

namespace cvgs {

template <int NPL>
struct WarpKernArgs {
    ChainArgs c;
    WarpPlane planes[NPL > 0 ? NPL : 1];
};
static_assert(sizeof(WarpKernArgs<kInlineWarp>) <= 4096, "kernel-argument block must fit 4 KB");

template <int NPL>
__global__ __launch_bounds__(256) void k_warp(const WarpKernArgs<NPL> a, const WarpPlane* __restrict__ table) {
    const ChainArgs& c = a.c;
    const ReadArgs& r = c.read;
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = blockIdx.y * 4 + threadIdx.y;
    const int z = blockIdx.z;
    if (x >= r.dst_w || y >= r.dst_h) return;
    WarpPlane P;
    if constexpr (NPL == 0) P = table[z];
    else P = a.planes[z];
    if (x >= P.dw || y >= P.dh) return; // this plane's own destination size (the launch covers the largest)

    Px p;
    p.v[0] = p.v[1] = p.v[2] = p.v[3] = 0.f;
    int depth = CVGS_DEPTH_32F, cn = r.out_cn;
    if (z >= r.used) {
#pragma unroll
        for (int k = 0; k < 4; ++k) p.v[k] = r.bg[k]; // fk::BatchRead default value, then the whole chain
    } else {
        const float fx = (float)x, fy = (float)y;
        float sx = (P.m[0] * fx + P.m[1] * fy) + P.m[2];
        float sy = (P.m[3] * fx + P.m[4] * fy) + P.m[5];
        if (r.kind == CVGS_READ_WARP_PERSPECTIVE) {
            const float w = (P.m[6] * fx + P.m[7] * fy) + P.m[8];
            sx = sx / w;
            sy = sy / w;
        }
        if (sx >= 0.f && sx < (float)P.w && sy >= 0.f && sy < (float)P.h) {
            const int x1 = (int)floorf(sx), y1 = (int)floorf(sy);
            const int x2 = x1 + 1, y2 = y1 + 1;
            const int x2r = min(x2, P.w - 1), y2r = min(y2, P.h - 1);
            Px p00, p10, p01, p11;
            const uint8_t* ra = P.data + (size_t)y1 * (size_t)P.step;
            const uint8_t* rb = P.data + (size_t)y2r * (size_t)P.step;
            load_px(ra, r.depth, r.cn, x1, p00);
            load_px(ra, r.depth, r.cn, x2r, p10);
            load_px(rb, r.depth, r.cn, x1, p01);
            load_px(rb, r.depth, r.cn, x2r, p11);
            const float w00 = ((float)x2 - sx) * ((float)y2 - sy);
            const float w10 = (sx - (float)x1) * ((float)y2 - sy);
            const float w01 = ((float)x2 - sx) * (sy - (float)y1);
            const float w11 = (sx - (float)x1) * (sy - (float)y1);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < r.cn) {
                    float acc = tap_f(p00.v[k], r.depth) * w00;
                    acc = acc + tap_f(p10.v[k], r.depth) * w10;
                    acc = acc + tap_f(p01.v[k], r.depth) * w01;
                    acc = acc + tap_f(p11.v[k], r.depth) * w11;
                    p.v[k] = acc;
                }
            }
        }
    }
    InterpProgInt::run(c.prog, p, depth, cn);
    const DstPlane* dst = c.write.table ? c.write.table : c.dst_inline;
    write_px<true>(c.write, dst, x, y, z, p, depth, cn);
}

template <int NPL>
static hipError_t launch_warp_t(const ChainArgs& c, const WarpPlane* planes, int n, const WarpPlane* table, hipStream_t s) {
    WarpKernArgs<NPL> a;
    a.c = c;
    for (int i = 0; i < (NPL > 0 ? NPL : 1); ++i) a.planes[i] = (NPL > 0 && i < n) ? planes[i] : WarpPlane{};
    const dim3 block(64, 4, 1);
    const dim3 grid((c.read.dst_w + 63) / 64, (c.read.dst_h + 3) / 4, c.read.batch);
    hipLaunchKernelGGL(k_warp<NPL>, grid, block, 0, s, a, table);
    return hipGetLastError();
}

// ---- fast path: u8 C3/C4 sources -> program -> planar fp32 tensor (the batched "align N faces / N detections and
// hand them to the network" shape).  Same structure as the fast resize kernel: lane = output column, wave = one output
// row, blockIdx.y = plane; both horizontal taps of a source row arrive in ONE unaligned 8-byte load (two loads per
// pixel), compile-time pointwise program, non-temporal 256-byte planar rows.  Bit-identical to k_warp.
struct WarpGeom {
    uint32_t col_tiles;
    int32_t dst_w, dst_h, used, out_w, pad;
    int64_t img_stride, ch_stride;
    void* out; // float* or _Float16* (OT)
    int64_t row_pitch, img_pitch; // PACKED: bytes between output rows / images
};

// One output pixel of the fast kernels, from the default-value test to the store: the transform, the window loads, the four weights and the
// program stand here ONCE, and the single launch (k_warp_fast) and the tick (k_warp_fast_many) both run this text -- the tick is bit-identical
// to n single launches by construction.  read_plane: the plane has a source (z < used; wave-uniform); plane_of() fetches its descriptor (a
// device table, the kernel arguments) and is called only then; the "s" constraints keep the descriptor in SGPRs.  orow: row y of the plane's
// first channel in the target tensor (PACKED: pixel 0 of row y).
template <int CN, class Prog, bool PERSP, typename OT, bool PACKED, class PlaneOf>
__device__ __forceinline__ void warp_fast_px(const ChainArgs& c, bool read_plane, PlaneOf plane_of, int x, int y, OT* orow, int64_t ch_stride) {
    Px p;
    p.v[0] = p.v[1] = p.v[2] = p.v[3] = 0.f;
    if (!read_plane) {
#pragma unroll
        for (int k = 0; k < 4; ++k) p.v[k] = c.read.bg[k];
    } else {
        const WarpPlane P = plane_of();
        asm volatile("" ::"s"(P.w), "s"(P.h), "s"(P.step), "s"(P.data), "s"(P.m[0]), "s"(P.m[1]), "s"(P.m[2]), "s"(P.m[3]), "s"(P.m[4]),
                     "s"(P.m[5]), "s"(P.m[6]), "s"(P.m[7]), "s"(P.m[8]));
        const float fx = (float)x, fy = (float)y;
        float sx = (P.m[0] * fx + P.m[1] * fy) + P.m[2];
        float sy = (P.m[3] * fx + P.m[4] * fy) + P.m[5];
        if constexpr (PERSP) {
            const float w = (P.m[6] * fx + P.m[7] * fy) + P.m[8];
            sx = sx / w;
            sy = sy / w;
        }
        if (sx >= 0.f && sx < (float)P.w && sy >= 0.f && sy < (float)P.h) {
            const int x1 = (int)floorf(sx), y1 = (int)floorf(sy);
            const int x2 = x1 + 1, y2 = y1 + 1;
            const int y2r = min(y2, P.h - 1);
            const bool edge = x2 > P.w - 1;
            const int row_bytes = P.w * CN;
            const int o = x1 * CN;
            const bool tiny = row_bytes < 8; // uniform per plane
            const uint32_t ol = (uint32_t)(tiny ? o : min(o, row_bytes - 8));
            const int sh = (o - (int)ol) * 8;
            const gptr_u8 ra = (gptr_u8)P.data + (size_t)y1 * (size_t)P.step;
            const gptr_u8 rb = (gptr_u8)P.data + (size_t)y2r * (size_t)P.step;
            Win<1> va, vb;
            if (!tiny) {
                va = load_win<1>(ra + ol);
                vb = load_win<1>(rb + ol);
            } else {
                va = gather_win<CN, 1>(ra, o, row_bytes);
                vb = gather_win<CN, 1>(rb, o, row_bytes);
            }
            float p00[4], p10[4], p01[4], p11[4];
            unpack_pair<CN, SRC_U8>(shift_win<1>(va, sh), edge, p00, p10);
            unpack_pair<CN, SRC_U8>(shift_win<1>(vb, sh), edge, p01, p11);
            const float w00 = ((float)x2 - sx) * ((float)y2 - sy);
            const float w10 = (sx - (float)x1) * ((float)y2 - sy);
            const float w01 = ((float)x2 - sx) * (sy - (float)y1);
            const float w11 = (sx - (float)x1) * (sy - (float)y1);
#pragma unroll
            for (int k = 0; k < CN; ++k) {
                float acc = p00[k] * w00;
                acc = acc + p10[k] * w10;
                acc = acc + p01[k] * w01;
                acc = acc + p11[k] * w11;
                p.v[k] = acc;
            }
        }
    }
    int depth = CVGS_DEPTH_32F, cn = CN;
    Prog::run(c.prog, p, depth, cn);
    if constexpr (PACKED) { // NHWC: one 12 / 16-byte store per pixel, consecutive lanes write consecutive pixels
        store_packed_px<CN, OT>(orow + (int64_t)x * cn, p.v, cn);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cn) st_nt(orow + (int64_t)k * ch_stride + x, p.v[k]); // OT = _Float16 / __bf16: the chain's trailing CAST
    }
}

template <int CN, int NPL, class Prog, bool PERSP, typename OT = float, bool PACKED = false>
__global__ __launch_bounds__(256) void k_warp_fast(const WarpKernArgs<NPL> a, const WarpPlane* __restrict__ table, const WarpGeom g) {
    const ChainArgs& c = a.c;
    const int z = (int)blockIdx.y;
    const int dst_w = g.dst_w, dst_h = g.dst_h, used = g.used, W = g.out_w;
    asm volatile("" ::"s"(dst_w), "s"(dst_h), "s"(used), "s"(W));
    int col_tile = 0, row_tile = (int)blockIdx.x;
    if (g.col_tiles > 1) {
        col_tile = (int)(blockIdx.x % g.col_tiles);
        row_tile = (int)(blockIdx.x / g.col_tiles);
    }
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const int x = col_tile * 64 + lane;
    const int y = row_tile * 4 + wave;
    if (y >= dst_h || x >= dst_w) return;
    OT* orow;
    if constexpr (PACKED) orow = (OT*)((uint8_t*)g.out + (int64_t)z * g.img_pitch + (int64_t)y * g.row_pitch);
    else orow = (OT*)g.out + (int64_t)z * g.img_stride + (int64_t)y * W;
    warp_fast_px<CN, Prog, PERSP, OT, PACKED>(c, z < used, [&]() -> WarpPlane {
        if constexpr (NPL == 0) return table[z];
        else return a.planes[z];
    }, x, y, orow, g.ch_stride);
}

// ---- the tick: the warp chains of one cvgs_execute_many call, k_warp_fast for n chains in ONE launch (planar targets) ----
// grid: x = column tiles x row tiles as above, y = plane inside the chain (up to the tick's largest batch), z = chain.  The chain's segment is read
// wave-uniformly; a workgroup beyond its chain's batch leaves; planes from seg.used on take the background; seg.out is the chain's tensor.
// NPL == 0: seg.table is the chain's WarpPlane table in device memory, the caller's own.  NPL < 0: the WarpPlanes of ALL chains inside the kernel
// arguments (WarpArgsManyInline<-NPL>), seg.table = first index.  No store stands in front of the descriptor's loads (k_area.hip: k_area_fast_many).
struct WarpManyGeom {
    uint32_t col_tiles;
    int32_t dst_w, dst_h, out_w;
    int64_t img_stride, ch_stride;
};
template <int NPL> using WarpManyArgs = std::conditional_t<NPL == 0, KernArgsMany, WarpArgsManyInline<(NPL < 0 ? -NPL : 1)>>;

template <int CN, int NPL, class Prog, bool PERSP, typename OT>
__global__ __launch_bounds__(256) void k_warp_fast_many(const WarpManyArgs<NPL> a, const WarpManyGeom g) {
    static_assert(NPL <= 0, "the tick reads its planes through segments");
    const ManySeg sg = a.seg[blockIdx.z];
    const int z = (int)blockIdx.y;
    if (z >= sg.batch) return; // a shorter chain of the tick
    const int dst_w = g.dst_w, dst_h = g.dst_h, W = g.out_w;
    asm volatile("" ::"s"(dst_w), "s"(dst_h), "s"(W), "s"(sg.used), "s"(sg.out));
    int col_tile = 0, row_tile = (int)blockIdx.x;
    if (g.col_tiles > 1) {
        col_tile = (int)(blockIdx.x % g.col_tiles);
        row_tile = (int)(blockIdx.x / g.col_tiles);
    }
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const int x = col_tile * 64 + lane;
    const int y = row_tile * 4 + wave;
    if (y >= dst_h || x >= dst_w) return;
    OT* const orow = (OT*)sg.out + (int64_t)z * g.img_stride + (int64_t)y * W;
    warp_fast_px<CN, Prog, PERSP, OT, false>(a.c, z < sg.used, [&]() -> WarpPlane {
        if constexpr (NPL == 0) return ((const WarpPlane*)sg.table)[z];
        else return a.planes[(uint32_t)(uintptr_t)sg.table + (uint32_t)z];
    }, x, y, orow, g.ch_stride);
}

// the staging buffer of an inline tick's argument block (20 KB): one per thread, handed over by address (as the AREA tick's)
static WarpArgsManyInline<kManyInlineWarp>& warp_many_staged() {
    static thread_local std::unique_ptr<WarpArgsManyInline<kManyInlineWarp>> staged;
    if (!staged) staged.reset(new WarpArgsManyInline<kManyInlineWarp>());
    return *staged;
}

// x.segs: the tick's chains (c.read.batch = the largest batch).  table != nullptr: every seg.table is the device address of a WarpPlane table;
// else planes / n: the planes of all chains (at most kManyInlineWarp), which travel in the kernel arguments.
template <int CN, class Prog, bool PERSP, typename OT>
static hipError_t launch_warp_fast_many_t(const ChainArgs& c, const WarpPlane* planes, int n, const WarpPlane* table, LaunchCtx& x) {
    if (x.record_only) return hipErrorNotSupported; // (no launch record is kept here: nothing is enqueued)
    if (x.n_segs < 1 || x.n_segs > CVGS_MAX_CHAINS) return hipErrorInvalidValue;
    WarpManyGeom g;
    g.col_tiles = (uint32_t)((c.read.dst_w + 63) / 64);
    g.dst_w = c.read.dst_w; g.dst_h = c.read.dst_h; g.out_w = c.write.width;
    g.img_stride = c.write.img_stride; g.ch_stride = c.write.ch_stride;
    const dim3 grid(g.col_tiles * (uint32_t)((c.read.dst_h + 3) / 4), (unsigned)c.read.batch, (unsigned)x.n_segs);
    auto launch = [&](const void* fn, void* a) {
        void* args[] = {a, (void*)&g};
        const hipError_t e = hipLaunchKernel(fn, grid, dim3(256), args, 0, (hipStream_t)x.stream);
        return e != hipSuccess ? e : hipGetLastError();
    };
    if (!table) { // host descriptors: segments + planes in the arguments, capturable
        if (!planes || n < 1 || n > kManyInlineWarp) return hipErrorInvalidValue;
        for (int i = 0; i < x.n_segs; ++i) // every chain's planes lie inside the block
            if ((uintptr_t)x.segs[i].table > (uintptr_t)n || x.segs[i].batch < 0 || (uintptr_t)x.segs[i].table + (uintptr_t)x.segs[i].batch > (uintptr_t)n) return hipErrorInvalidValue;
        WarpArgsManyInline<kManyInlineWarp>& a = warp_many_staged();
        a.c = c;
        for (int i = 0; i < CVGS_MAX_CHAINS; ++i) a.seg[i] = i < x.n_segs ? x.segs[i] : ManySeg{nullptr, nullptr, 0, 0};
        for (int i = 0; i < n; ++i) a.planes[i] = planes[i];
        return launch((const void*)&k_warp_fast_many<CN, -kManyInlineWarp, Prog, PERSP, OT>, &a);
    }
    KernArgsMany a;
    a.c = c;
    for (int i = 0; i < CVGS_MAX_CHAINS; ++i) a.seg[i] = i < x.n_segs ? x.segs[i] : ManySeg{nullptr, nullptr, 0, 0};
    return launch((const void*)&k_warp_fast_many<CN, 0, Prog, PERSP, OT>, &a);
}

template <int CN, class Prog, bool PERSP, typename OT, bool PACKED = false>
static hipError_t launch_warp_fast_t(const ChainArgs& c, const WarpPlane* planes, int n, const WarpPlane* table, LaunchCtx& x) {
    if (x.segs) { // the chains of a tick: planar targets only (try_warp_fast)
        if constexpr (PACKED) return hipErrorInvalidValue;
        else return launch_warp_fast_many_t<CN, Prog, PERSP, OT>(c, planes, n, table, x);
    }
    hipStream_t s = (hipStream_t)x.stream;
    WarpGeom g;
    g.col_tiles = (uint32_t)((c.read.dst_w + 63) / 64);
    g.dst_w = c.read.dst_w; g.dst_h = c.read.dst_h; g.used = c.read.used; g.out_w = c.write.width; g.pad = 0;
    g.img_stride = c.write.img_stride; g.ch_stride = c.write.ch_stride;
    g.out = c.write.data;
    const int64_t px_bytes = (int64_t)sizeof(OT) * c.write.cn;
    g.row_pitch = c.write.kind == CVGS_WRITE_PIXEL_2D ? c.write.step : c.write.width * px_bytes;
    g.img_pitch = c.write.kind == CVGS_WRITE_PIXEL_2D ? 0 : c.write.img_stride * px_bytes;
    const dim3 grid(g.col_tiles * (uint32_t)((c.read.dst_h + 3) / 4), (unsigned)c.read.batch);
    if (table) {
        WarpKernArgs<0> a;
        a.c = c;
        a.planes[0] = WarpPlane{};
        hipLaunchKernelGGL((k_warp_fast<CN, 0, Prog, PERSP, OT, PACKED>), grid, dim3(256), 0, s, a, table, g);
    } else {
        WarpKernArgs<kInlineWarp> a;
        a.c = c;
        for (int i = 0; i < kInlineWarp; ++i) a.planes[i] = i < n ? planes[i] : WarpPlane{};
        hipLaunchKernelGGL((k_warp_fast<CN, kInlineWarp, Prog, PERSP, OT, PACKED>), grid, dim3(256), 0, s, a, (const WarpPlane*)nullptr, g);
    }
    return hipGetLastError();
}

template <int CN, bool PERSP, typename OT>
static hipError_t launch_warp_fast_ot(int prog_id, const ChainArgs& c, const WarpPlane* planes, int n, const WarpPlane* table, LaunchCtx& x) {
    if (prog_id == 0) return launch_warp_fast_t<CN, ProgSwapMulSubDiv, PERSP, OT>(c, planes, n, table, x);
    if (prog_id == 1) return launch_warp_fast_t<CN, ProgMulSubDiv, PERSP, OT>(c, planes, n, table, x);
    return launch_warp_fast_t<CN, InterpProg, PERSP, OT>(c, planes, n, table, x);
}
// packed fp32 pixels (NHWC): interpreted program
template <int CN, bool PERSP>
static hipError_t launch_warp_fast_packed(const ChainArgs& c, const WarpPlane* planes, int n, const WarpPlane* table, LaunchCtx& x) {
    return launch_warp_fast_t<CN, InterpProg, PERSP, float, true>(c, planes, n, table, x);
}
template <int CN, bool PERSP>
static hipError_t launch_warp_fast_prog(bool f16, int prog_id, const ChainArgs& c, const WarpPlane* planes, int n, const WarpPlane* table,
                                        LaunchCtx& x) {
    if (f16) return launch_warp_fast_ot<CN, PERSP, _Float16>(prog_id, c, planes, n, table, x);
    return launch_warp_fast_ot<CN, PERSP, float>(prog_id, c, planes, n, table, x);
}

// bf16 (CV_16BF) tensors: the fp16 instantiations' twins with OT = __bf16, compiled in k_warp_bf16.hip (this file with CVGS_WARP_BF16_TU)
hipError_t warp_fast_launch_bf16(int cn, bool persp, int prog_id, const ChainArgs& c, const WarpPlane* planes, int n, const WarpPlane* table, LaunchCtx& x);
#ifdef CVGS_WARP_BF16_TU
hipError_t warp_fast_launch_bf16(int cn, bool persp, int prog_id, const ChainArgs& c, const WarpPlane* planes, int n, const WarpPlane* table, LaunchCtx& x) {
    if (cn == 3) return persp ? launch_warp_fast_ot<3, true, __bf16>(prog_id, c, planes, n, table, x) : launch_warp_fast_ot<3, false, __bf16>(prog_id, c, planes, n, table, x);
    return persp ? launch_warp_fast_ot<4, true, __bf16>(prog_id, c, planes, n, table, x) : launch_warp_fast_ot<4, false, __bf16>(prog_id, c, planes, n, table, x);
}
#else
// 1 = took it, 0 = not eligible.  x.segs: the chains of a tick (launch_warp_many) -- the same conditions, planar targets only, the tick kernel
static int try_warp_fast(const ChainArgs& c_in, const WarpPlane* planes, int n, const WarpPlane* table, LaunchCtx& x, bool dry_run,
                         LaunchInfo* info, hipError_t* err) {
    const ReadArgs& r = c_in.read;
    if (r.depth != CVGS_DEPTH_8U || (r.cn != 3 && r.cn != 4) || r.batch > 65535) return 0;
    const bool planar = c_in.write.kind == CVGS_WRITE_TENSOR_SPLIT || c_in.write.kind == CVGS_WRITE_TENSOR_T_SPLIT;
    const bool packed = c_in.write.kind == CVGS_WRITE_PIXEL_2D || c_in.write.kind == CVGS_WRITE_PIXEL_3D;
    if ((!planar && !packed) || c_in.write.data2 || (packed && x.segs)) return 0;
    // bf16 tensors take the fp16 path with the bf16 twins ("f16" below: a 16-bit float store); the program may hold no other bf16 cast
    const bool bf16 = c_in.write.depth == kDepthBF16;
    const bool f16 = c_in.write.depth == CVGS_DEPTH_16F || bf16;
    if (!f16 && c_in.write.depth != CVGS_DEPTH_32F) return 0;
    if (packed && f16) return 0;
    ChainArgs c_cut;
    if (f16) { // fp16 tensors: the trailing CAST(CV_16F) moves into the store
        if (c_in.prog.n < 1 || c_in.prog.opcode[c_in.prog.n - 1] != CVGS_OP_CAST) return 0;
        c_cut = c_in;
        c_cut.prog.n -= 1;
    }
    const ChainArgs& c = f16 ? c_cut : c_in;
    for (int k = 0; k < c.prog.n; ++k)
        if (c.prog.opcode[k] == CVGS_OP_CAST || c.prog.opcode[k] == CVGS_OP_CAST_TRUNC) return 0;
    const ProgArgs& p = c.prog;
    const int swap = r.cn == 3 ? (2 | (1 << 2) | (0 << 4)) : (2 | (1 << 2) | (0 << 4) | (3 << 6));
    int prog_id = 2;
    if (p.n == 4 && p.opcode[0] == CVGS_OP_REORDER && p.aux[0] == swap && p.opcode[1] == CVGS_OP_MUL && p.opcode[2] == CVGS_OP_SUB &&
        p.opcode[3] == CVGS_OP_DIV)
        prog_id = 0;
    else if (p.n == 3 && p.opcode[0] == CVGS_OP_MUL && p.opcode[1] == CVGS_OP_SUB && p.opcode[2] == CVGS_OP_DIV)
        prog_id = 1;
    const bool persp = r.kind == CVGS_READ_WARP_PERSPECTIVE;
    if (info) {
        static const char* names[2][2][3] = {
            {{"warp_affine_u8c3_swap_mul_sub_div", "warp_affine_u8c3_mul_sub_div", "warp_affine_u8c3_interp"},
             {"warp_affine_u8c4_swap_mul_sub_div", "warp_affine_u8c4_mul_sub_div", "warp_affine_u8c4_interp"}},
            {{"warp_perspective_u8c3_swap_mul_sub_div", "warp_perspective_u8c3_mul_sub_div", "warp_perspective_u8c3_interp"},
             {"warp_perspective_u8c4_swap_mul_sub_div", "warp_perspective_u8c4_mul_sub_div", "warp_perspective_u8c4_interp"}}};
        static const char* names16[2][2][3] = {
            {{"warp_affine_u8c3_swap_mul_sub_div_f16", "warp_affine_u8c3_mul_sub_div_f16", "warp_affine_u8c3_interp_f16"},
             {"warp_affine_u8c4_swap_mul_sub_div_f16", "warp_affine_u8c4_mul_sub_div_f16", "warp_affine_u8c4_interp_f16"}},
            {{"warp_perspective_u8c3_swap_mul_sub_div_f16", "warp_perspective_u8c3_mul_sub_div_f16", "warp_perspective_u8c3_interp_f16"},
             {"warp_perspective_u8c4_swap_mul_sub_div_f16", "warp_perspective_u8c4_mul_sub_div_f16", "warp_perspective_u8c4_interp_f16"}}};
        static const char* names_packed[2][2] = {{"warp_affine_u8c3_packed_f32", "warp_affine_u8c4_packed_f32"},
                                                 {"warp_perspective_u8c3_packed_f32", "warp_perspective_u8c4_packed_f32"}};
        info->kernel = packed ? names_packed[persp][r.cn == 4] : (f16 ? names16[persp][r.cn == 4][prog_id] : names[persp][r.cn == 4][prog_id]);
        if (bf16) info->kernel = bf16_kernel_name(info->kernel);
    }
    if (dry_run) return 1;
    if (packed) {
        if (r.cn == 3) *err = persp ? launch_warp_fast_packed<3, true>(c, planes, n, table, x) : launch_warp_fast_packed<3, false>(c, planes, n, table, x);
        else *err = persp ? launch_warp_fast_packed<4, true>(c, planes, n, table, x) : launch_warp_fast_packed<4, false>(c, planes, n, table, x);
        return 1;
    }
    if (bf16) {
        *err = warp_fast_launch_bf16(r.cn, persp, prog_id, c, planes, n, table, x);
        return 1;
    }
    if (r.cn == 3) *err = persp ? launch_warp_fast_prog<3, true>(f16, prog_id, c, planes, n, table, x) : launch_warp_fast_prog<3, false>(f16, prog_id, c, planes, n, table, x);
    else *err = persp ? launch_warp_fast_prog<4, true>(f16, prog_id, c, planes, n, table, x) : launch_warp_fast_prog<4, false>(f16, prog_id, c, planes, n, table, x);
    return 1;
}

int launch_warp(const ChainArgs& c, const WarpPlane* planes, int n, const WarpPlane* dev_table, uint32_t chain_flags, void* stream,
                bool dry_run, LaunchInfo* info) {
    const bool persp = c.read.kind == CVGS_READ_WARP_PERSPECTIVE;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    LaunchCtx one(stream);
    if (!(chain_flags & CVGS_CHAIN_FORCE_GENERIC) && try_warp_fast(c, planes, n, dev_table, one, dry_run, info, &e))
        return e == hipSuccess ? 0 : -(int)e - 1000;
    if (info) info->kernel = persp ? "warp_perspective_interp" : "warp_affine_interp";
    if (dry_run) return 0;
    if (dev_table) e = launch_warp_t<0>(c, nullptr, 0, dev_table, s);
    else if (n <= 4) e = launch_warp_t<4>(c, planes, n, nullptr, s);
    else e = launch_warp_t<kInlineWarp>(c, planes, n, nullptr, s);
    return e == hipSuccess ? 0 : -(int)e - 1000;
}

int launch_warp_many(const ChainArgs& c, const WarpPlane* planes, int n_planes, const WarpPlane* dev_table, LaunchCtx& ctx, bool dry_run, LaunchInfo* info) {
    if (!ctx.segs || ctx.n_segs < 1 || ctx.n_segs > CVGS_MAX_CHAINS) return 0;
    hipError_t e = hipSuccess;
    if (!try_warp_fast(c, planes, n_planes, dev_table, ctx, dry_run, info, &e)) return 0;
    return e == hipSuccess ? 1 : -(int)e - 1000;
}
#endif // CVGS_WARP_BF16_TU

} // namespace cvgs
