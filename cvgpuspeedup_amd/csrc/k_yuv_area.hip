// k_yuv_area.hip -- INTER_AREA (box filter) resize of 4:2:0 decoder surfaces (NV12 / NV21 / P010) fused in front of a pointwise chain and a
// write stage: CVGS_READ_NV12_RESIZE_AREA.  An engine extension: the bilinear NV12 kind reads 2 x 2 taps per output pixel, this kind weighs
// every luma sample of the view by the share of it the output pixel covers and every chroma sample by the luma area it sits under, then
// converts the three means ONCE (yuv_to_rgb, the bilinear kind's per-tap conversion; it is affine, so this is "convert, then box-filter" up
// to rounding).  The planes are the bilinear NV12 resize's PlaneParams (fx, fy, window, uv_off), inline in the kernel arguments or in a
// device table.
// The arithmetic is the contract written down in include/cvgs_hip.h (strict fp32, every operation rounded once, in the written order);
// ALL kernels below run the same text for it (yuv_area_value over area_axis / area_chroma_axis of k_area_axis.hpp), so the fast kernel is
// bit-identical to the interpreted one -- and the fast kernel's pixel is ONE function (yuv_area_fast_px) that the single launch and the
// cvgs_execute_many tick (k_yuv_area_fast_many: the chains of a tick in one launch, grid z = chain) both call.  One lane = one output pixel; the tap loops are dynamic loops over the footprint and every weight
// is recomputed from (a, b, index) inside them: no per-lane arrays, nothing in scratch or LDS.  Luma taps are one sample each, chroma taps
// one load of the (U, V) pair; adjacent lanes own adjacent footprints, so a wave's loads of one source row form one contiguous span.
#include <memory>
#include <type_traits>

#include "k_area_axis.hpp"
#include "k_taps.hpp"

namespace cvgs {

typedef uint16_t yuv_area_u16u __attribute__((aligned(1))); // the chroma pair of an 8-bit surface: no alignment assumed (any data, step)
typedef const __attribute__((address_space(1))) yuv_area_u16u* gptr_yuv_area_u16u;
typedef const __attribute__((address_space(1))) uint16_t* gptr_yuv_area_u16;

// (Y, U, V) means of output pixel (tx, ty) of the window of plane P.  TEN: 16-bit samples with the 10-bit code in the high bits (P010);
// otherwise bytes.  The pair's first sample goes to c0, the second to c1 (NV12: U, V; NV21: V, U -- the caller swaps after the load).
template <bool TEN>
__device__ __forceinline__ void yuv_area_means(const PlaneParams& P, int tx, int ty, float& Ym, float& c0m, float& c1m) {
    const AreaAxis X = area_axis(tx, P.fx, P.w), Y = area_axis(ty, P.fy, P.h);
    const AreaAxis CX = area_chroma_axis(X, P.w), CY = area_chroma_axis(Y, P.h);
    const gptr_u8 base = (gptr_u8)P.data;
    {
        float acc = 0.0f;
        for (int jj = 0; jj < Y.cnt; ++jj) {
            const float wy = area_w(Y, jj);
            const int j = max(min(Y.i0 + jj, P.h - 1), 0);
            const gptr_u8 rp = base + (size_t)j * (size_t)P.step;
            float row = 0.0f;
            for (int ii = 0; ii < X.cnt; ++ii) {
                const float wx = area_w(X, ii);
                const int i = max(min(X.i0 + ii, P.w - 1), 0);
                float v;
                if constexpr (TEN) v = (float)(((gptr_yuv_area_u16)rp)[i] >> 6);
                else v = (float)rp[i];
                row = row + v * wx;
            }
            acc = acc + row * wy;
        }
        Ym = acc * (1.0f / (X.W * Y.W));
    }
    {
        const int ncx = (P.w + 1) >> 1, ncy = (P.h + 1) >> 1;
        const gptr_u8 cbase = base + (size_t)P.uv_off;
        float acc0 = 0.0f, acc1 = 0.0f;
        for (int jj = 0; jj < CY.cnt; ++jj) {
            const float wy = area_w(CY, jj);
            const int j = max(min(area_chroma_index(CY, jj, P.h), ncy - 1), 0);
            const gptr_u8 rp = cbase + (size_t)j * (size_t)P.step;
            float row0 = 0.0f, row1 = 0.0f;
            for (int ii = 0; ii < CX.cnt; ++ii) {
                const float wx = area_w(CX, ii);
                const int i = max(min(area_chroma_index(CX, ii, P.w), ncx - 1), 0);
                float v0, v1;
                if constexpr (TEN) {
                    const gptr_yuv_area_u16 pp = (gptr_yuv_area_u16)rp + 2 * i;
                    v0 = (float)(pp[0] >> 6);
                    v1 = (float)(pp[1] >> 6);
                } else {
                    const uint32_t pair = ((gptr_yuv_area_u16u)rp)[i];
                    v0 = (float)(pair & 0xffu);
                    v1 = (float)(pair >> 8);
                }
                row0 = row0 + v0 * wx;
                row1 = row1 + v1 * wx;
            }
            acc0 = acc0 + row0 * wy;
            acc1 = acc1 + row1 * wy;
        }
        const float inv = 1.0f / (CX.W * CY.W);
        c0m = acc0 * inv;
        c1m = acc1 * inv;
    }
}

// the value of output pixel (x, y) of a plane before the chain's program: the converted means inside the window, the background
// outside it and on planes without a source (z >= used: fk::BatchRead's default value) -- the rules of the bilinear NV12 kind.
// read_plane: the plane has a source (wave-uniform); plane_of() fetches its descriptor (a device table, the kernel arguments, a tick's
// segment) and is called only then.
template <bool TEN, class PlaneOf>
__device__ __forceinline__ void yuv_area_value(const ReadArgs& r, bool read_plane, PlaneOf plane_of, int x, int y, Px& p) {
    p.v[0] = p.v[1] = p.v[2] = p.v[3] = 0.f;
    bool inside = false;
    if (read_plane) {
        const PlaneParams P = plane_of();
        if (x >= P.x1 && x <= P.x2 && y >= P.y1 && y <= P.y2) {
            inside = true;
            float Ym, c0, c1;
            yuv_area_means<TEN>(P, x - P.x1, y - P.y1, Ym, c0, c1);
            const bool vu = r.yuv_layout == CVGS_YUV_NV21; // V first: swapped after the load
            const YuvK k = yuv_matrix(r.yuv_range, r.yuv_primaries, r.yuv_layout);
            yuv_to_rgb(Ym, vu ? c1 : c0, vu ? c0 : c1, k, p);
        }
    }
    if (!inside) {
#pragma unroll
        for (int k = 0; k < 4; ++k) p.v[k] = r.bg[k];
    }
}
template <bool TEN, int NPL>
__device__ __forceinline__ void yuv_area_px(const KernArgs<NPL>& a, int x, int y, int z, int used, Px& p) {
    yuv_area_value<TEN>(a.c.read, z < used, [&]() -> PlaneParams {
        if constexpr (NPL == 0) return a.c.read.table[z];
        else return a.planes[z];
    }, x, y, p);
}

// ---- the interpreted kernel: every served layout, interpreted program, generic write stage ----
template <int NPL>
__global__ __launch_bounds__(256) void k_yuv_area(const KernArgs<NPL> a) {
    const ChainArgs& c = a.c;
    const ReadArgs& r = c.read;
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = blockIdx.y * 4 + threadIdx.y;
    const int z = blockIdx.z;
    if (x >= r.dst_w || y >= r.dst_h) return;

    Px p;
    if (r.yuv_layout == CVGS_YUV_P010) yuv_area_px<true, NPL>(a, x, y, z, r.used, p);
    else yuv_area_px<false, NPL>(a, x, y, z, r.used, p);
    int depth = CVGS_DEPTH_32F, cn = r.out_cn;
    InterpProgInt::run(c.prog, p, depth, cn);
    const DstPlane* dst = c.write.table ? c.write.table : c.dst_inline;
    write_px<true>(c.write, dst, x, y, z, p, depth, cn);
}

template <int NPL>
static hipError_t launch_yuv_area_t(const ChainArgs& c, const PlaneParams* planes, int n, hipStream_t s) {
    KernArgs<NPL> a;
    a.c = c;
    for (int i = 0; i < (NPL > 0 ? NPL : 1); ++i) a.planes[i] = (NPL > 0 && i < n) ? planes[i] : PlaneParams{};
    const dim3 block(64, 4, 1);
    const dim3 grid((c.read.dst_w + 63) / 64, (c.read.dst_h + 3) / 4, c.read.batch);
    hipLaunchKernelGGL(k_yuv_area<NPL>, grid, block, 0, s, a);
    return hipGetLastError();
}

// ---- fast path: 8-bit NV12 / NV21 crops -> program -> planar fp32 / fp16 / bf16 tensor (N detections of a decoder surface -> N x C x H x W) ----
// lane = output column, wave = one output row, blockIdx.y = plane; byte loads for luma, one 2-byte load per chroma pair, the running sums
// in registers, compile-time pointwise program, non-temporal planar rows.  Not staged through LDS (to be measured).
struct YuvAreaGeom {
    uint32_t col_tiles;
    int32_t dst_w, dst_h, used, out_w, pad;
    int64_t img_stride, ch_stride;
    void* out; // float* / _Float16* / __bf16* (OT)
};

// One output pixel of the fast kernels, from the window test to the store: the single launch (k_yuv_area_fast) and the tick
// (k_yuv_area_fast_many) both run this text -- the tick is bit-identical to n single launches by construction.  read_plane / plane_of: as
// yuv_area_value.  orow: row y of the plane's first channel in the target tensor.
template <int CN, class Prog, typename OT, class PlaneOf>
__device__ __forceinline__ void yuv_area_fast_px(const ChainArgs& c, bool read_plane, PlaneOf plane_of, int x, int y, OT* orow, int64_t ch_stride) {
    Px p;
    yuv_area_value<false>(c.read, read_plane, plane_of, x, y, p);
    int depth = CVGS_DEPTH_32F, cn = CN;
    Prog::run(c.prog, p, depth, cn);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < cn) st_nt(orow + (int64_t)k * ch_stride + x, p.v[k]); // OT = _Float16 / __bf16: the chain's trailing CAST
}

template <int CN, int NPL, class Prog, typename OT>
__global__ __launch_bounds__(256) void k_yuv_area_fast(const KernArgs<NPL> a, const YuvAreaGeom g) {
    const ChainArgs& c = a.c;
    const int z = (int)blockIdx.y;
    int col_tile = 0, row_tile = (int)blockIdx.x;
    if (g.col_tiles > 1) {
        col_tile = (int)(blockIdx.x % g.col_tiles);
        row_tile = (int)(blockIdx.x / g.col_tiles);
    }
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const int x = col_tile * 64 + lane;
    const int y = row_tile * 4 + wave;
    if (y >= g.dst_h || x >= g.dst_w) return;
    OT* const orow = (OT*)g.out + (int64_t)z * g.img_stride + (int64_t)y * g.out_w;
    yuv_area_fast_px<CN, Prog, OT>(c, z < g.used, [&]() -> PlaneParams {
        if constexpr (NPL == 0) return c.read.table[z];
        else return a.planes[z];
    }, x, y, orow, g.ch_stride);
}

// ---- the tick: the chains of one cvgs_execute_many call, k_yuv_area_fast for n chains in ONE launch ----
// grid: x = column tiles x row tiles as above, y = plane inside the chain (up to the tick's largest batch), z = chain.  The chain's segment is read
// wave-uniformly; a workgroup beyond its chain's batch leaves; planes from seg.used on take the background; seg.out is the chain's tensor.
// NPL == 0: seg.table is the chain's table in device memory -- the caller's own, or the staged host table (one instantiation serves both: the
// table arrives as a pointer).  NPL < 0: the planes of ALL chains inside the kernel arguments (KernArgsManyInline<-NPL>), seg.table = first index.
struct YuvAreaManyGeom {
    uint32_t col_tiles;
    int32_t dst_w, dst_h, out_w;
    int64_t img_stride, ch_stride;
    // a tick whose tables sit in a pooled slot (NPL == 0; cvgs_api.cpp: ManyPool): one work-item stores done_value into *done_word (pinned host
    // memory) -- every earlier launch of the stream has finished by then (as K1 / K4)
    uint64_t* done_word;
    uint64_t done_value;
};
template <int NPL> using YuvAreaManyArgs = std::conditional_t<NPL == 0, KernArgsMany, KernArgsManyInline<(NPL < 0 ? -NPL : 1)>>;

template <int CN, int NPL, class Prog, typename OT>
__global__ __launch_bounds__(256) void k_yuv_area_fast_many(const YuvAreaManyArgs<NPL> a, const YuvAreaManyGeom g) {
    static_assert(NPL <= 0, "the tick reads its planes through segments");
    const ManySeg sg = a.seg[blockIdx.z];
    const int z = (int)blockIdx.y;
    if (z >= sg.batch) return; // a shorter chain of the tick
    const int dst_w = g.dst_w, dst_h = g.dst_h, W = g.out_w;
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
    yuv_area_fast_px<CN, Prog, OT>(a.c, z < sg.used, [&]() -> PlaneParams {
        if constexpr (NPL == 0) return sg.table[z];
        else return a.planes[(uint32_t)(uintptr_t)sg.table + (uint32_t)z];
    }, x, y, orow, g.ch_stride);
    // (behind the pixel: a store in front of the descriptor's scalar loads would make the compiler fetch it with vector loads.  Work-item 0 of
    // workgroup (0, 0, 0) always owns pixel (0, 0) of plane 0 of chain 0 and so always gets here)
    if constexpr (NPL == 0) {
        if (g.done_word && (blockIdx.x | blockIdx.y | blockIdx.z) == 0 && threadIdx.x == 0)
            __hip_atomic_store(g.done_word, g.done_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// the staging buffer of an inline tick's argument block (16 KB / 52 KB): one per thread and size, handed over by address (as K1's / K4's)
template <int CAP> static KernArgsManyInline<CAP>& yuv_area_many_staged() {
    static thread_local std::unique_ptr<KernArgsManyInline<CAP>> staged;
    if (!staged) staged.reset(new KernArgsManyInline<CAP>());
    return *staged;
}

// x.segs: the tick's chains (c.read.batch = the largest batch).  planes / n: the planes of all chains when they travel in the kernel arguments
// (c.read.table == nullptr), else every seg.table is a device address.
template <int CN, class Prog, typename OT>
static hipError_t launch_yuv_area_fast_many_t(const ChainArgs& c, const PlaneParams* planes, int n, LaunchCtx& x) {
    hipStream_t s = (hipStream_t)x.stream;
    if (x.record_only) return hipErrorNotSupported; // (no launch record is kept here: nothing is enqueued)
    YuvAreaManyGeom g;
    g.col_tiles = (uint32_t)((c.read.dst_w + 63) / 64);
    g.dst_w = c.read.dst_w; g.dst_h = c.read.dst_h; g.out_w = c.write.width;
    g.img_stride = c.write.img_stride; g.ch_stride = c.write.ch_stride;
    g.done_word = nullptr;
    g.done_value = 0;
    const dim3 grid(g.col_tiles * (uint32_t)((c.read.dst_h + 3) / 4), (unsigned)c.read.batch, (unsigned)x.n_segs);
    auto launch = [&](const void* fn, void* a) {
        void* args[] = {a, (void*)&g};
        hipError_t e;
        if (x.stop_event && !x.stop_event_taken) { // the staged table's slot learns from the kernel's own completion signal (as K1)
            x.stop_event_taken = true;
            e = hipExtLaunchKernel(fn, grid, dim3(256), args, 0, s, nullptr, (hipEvent_t)x.stop_event, 0);
        } else {
            e = hipLaunchKernel(fn, grid, dim3(256), args, 0, s);
        }
        return e != hipSuccess ? e : hipGetLastError();
    };
    if (!c.read.table) { // host descriptors of at most kManyInlineLarge planes: segments + planes in the arguments, capturable
        if (!planes || n < 1 || n > kManyInlineLarge) return hipErrorInvalidValue;
        auto go = [&](auto cap_tag) {
            constexpr int CAP = decltype(cap_tag)::value;
            KernArgsManyInline<CAP>& a = yuv_area_many_staged<CAP>();
            a.c = c;
            for (int i = 0; i < CVGS_MAX_CHAINS; ++i) a.seg[i] = i < x.n_segs ? x.segs[i] : ManySeg{nullptr, nullptr, 0, 0};
            for (int i = 0; i < n && i < CAP; ++i) a.planes[i] = planes[i];
            return launch((const void*)&k_yuv_area_fast_many<CN, -CAP, Prog, OT>, &a);
        };
        if (n <= kManyInlineSmall) return go(std::integral_constant<int, kManyInlineSmall>{});
        return go(std::integral_constant<int, kManyInlineLarge>{});
    }
    KernArgsMany a;
    a.c = c;
    for (int i = 0; i < CVGS_MAX_CHAINS; ++i) a.seg[i] = i < x.n_segs ? x.segs[i] : ManySeg{nullptr, nullptr, 0, 0};
    if (x.done_word && !x.done_word_taken) {
        x.done_word_taken = true;
        g.done_word = x.done_word;
        g.done_value = x.done_value;
    }
    return launch((const void*)&k_yuv_area_fast_many<CN, 0, Prog, OT>, &a);
}

template <int CN, class Prog, typename OT>
static hipError_t launch_yuv_area_fast_t(const ChainArgs& c, const PlaneParams* planes, int n, LaunchCtx& x) {
    if (x.segs) return launch_yuv_area_fast_many_t<CN, Prog, OT>(c, planes, n, x);
    hipStream_t s = (hipStream_t)x.stream;
    YuvAreaGeom g;
    g.col_tiles = (uint32_t)((c.read.dst_w + 63) / 64);
    g.dst_w = c.read.dst_w; g.dst_h = c.read.dst_h; g.used = c.read.used; g.out_w = c.write.width; g.pad = 0;
    g.img_stride = c.write.img_stride; g.ch_stride = c.write.ch_stride;
    g.out = c.write.data;
    const dim3 grid(g.col_tiles * (uint32_t)((c.read.dst_h + 3) / 4), (unsigned)c.read.batch);
    if (c.read.table) {
        KernArgs<0> a;
        a.c = c;
        a.planes[0] = PlaneParams{};
        hipLaunchKernelGGL((k_yuv_area_fast<CN, 0, Prog, OT>), grid, dim3(256), 0, s, a, g);
    } else {
        KernArgs<CVGS_KERNARG_PLANES> a;
        a.c = c;
        for (int i = 0; i < CVGS_KERNARG_PLANES; ++i) a.planes[i] = i < n ? planes[i] : PlaneParams{};
        hipLaunchKernelGGL((k_yuv_area_fast<CN, CVGS_KERNARG_PLANES, Prog, OT>), grid, dim3(256), 0, s, a, g);
    }
    return hipGetLastError();
}

template <int CN, typename OT>
static hipError_t launch_yuv_area_fast_ot(int prog_id, const ChainArgs& c, const PlaneParams* planes, int n, LaunchCtx& s) {
    if (prog_id == 0) return launch_yuv_area_fast_t<CN, ProgSwapMulSubDiv, OT>(c, planes, n, s);
    if (prog_id == 1) return launch_yuv_area_fast_t<CN, ProgMulSubDiv, OT>(c, planes, n, s);
    return launch_yuv_area_fast_t<CN, InterpProg, OT>(c, planes, n, s);
}
template <int CN>
static hipError_t launch_yuv_area_fast_cn(int ot, int prog_id, const ChainArgs& c, const PlaneParams* planes, int n, LaunchCtx& s) {
    if (ot == 2) return launch_yuv_area_fast_ot<CN, __bf16>(prog_id, c, planes, n, s);
    if (ot == 1) return launch_yuv_area_fast_ot<CN, _Float16>(prog_id, c, planes, n, s);
    return launch_yuv_area_fast_ot<CN, float>(prog_id, c, planes, n, s);
}

// 1 = took it, 0 = not eligible.  s.segs: the chains of a tick (launch_yuv_area_many) -- the same conditions, the tick kernel
static int try_yuv_area_fast(const ChainArgs& c_in, const PlaneParams* planes, int n, LaunchCtx& s, bool dry_run, LaunchInfo* info, hipError_t* err) {
    const ReadArgs& r = c_in.read;
    if ((r.yuv_layout != CVGS_YUV_NV12 && r.yuv_layout != CVGS_YUV_NV21) || r.depth != CVGS_DEPTH_8U || r.batch > 65535) return 0;
    if ((c_in.write.kind != CVGS_WRITE_TENSOR_SPLIT && c_in.write.kind != CVGS_WRITE_TENSOR_T_SPLIT) || c_in.write.data2) return 0;
    const bool bf16 = c_in.write.depth == kDepthBF16;
    const bool f16 = c_in.write.depth == CVGS_DEPTH_16F || bf16; // a 16-bit float store
    if (!f16 && c_in.write.depth != CVGS_DEPTH_32F) return 0;
    ChainArgs c_cut;
    if (f16) { // the trailing CAST moves into the store
        if (c_in.prog.n < 1 || c_in.prog.opcode[c_in.prog.n - 1] != CVGS_OP_CAST) return 0;
        c_cut = c_in;
        c_cut.prog.n -= 1;
    }
    const ChainArgs& c = f16 ? c_cut : c_in;
    for (int k = 0; k < c.prog.n; ++k) // the value stays CV_32F with the read's channels: nothing that changes type or channel count
        if (c.prog.opcode[k] != CVGS_OP_MUL && c.prog.opcode[k] != CVGS_OP_ADD && c.prog.opcode[k] != CVGS_OP_SUB && c.prog.opcode[k] != CVGS_OP_DIV &&
            c.prog.opcode[k] != CVGS_OP_REORDER)
            return 0;
    const ProgArgs& p = c.prog;
    const int cn = r.out_cn;
    const int swap = cn == 3 ? (2 | (1 << 2) | (0 << 4)) : (2 | (1 << 2) | (0 << 4) | (3 << 6));
    int prog_id = 2;
    if (p.n == 4 && p.opcode[0] == CVGS_OP_REORDER && p.aux[0] == swap && p.opcode[1] == CVGS_OP_MUL && p.opcode[2] == CVGS_OP_SUB &&
        p.opcode[3] == CVGS_OP_DIV)
        prog_id = 0;
    else if (p.n == 3 && p.opcode[0] == CVGS_OP_MUL && p.opcode[1] == CVGS_OP_SUB && p.opcode[2] == CVGS_OP_DIV)
        prog_id = 1;
    if (info) {
        static const char* names[2][3] = {{"yuv_area_c3_swap_mul_sub_div", "yuv_area_c3_mul_sub_div", "yuv_area_c3_interp"},
                                          {"yuv_area_c4_swap_mul_sub_div", "yuv_area_c4_mul_sub_div", "yuv_area_c4_interp"}};
        static const char* names16[2][3] = {{"yuv_area_c3_swap_mul_sub_div_f16", "yuv_area_c3_mul_sub_div_f16", "yuv_area_c3_interp_f16"},
                                            {"yuv_area_c4_swap_mul_sub_div_f16", "yuv_area_c4_mul_sub_div_f16", "yuv_area_c4_interp_f16"}};
        info->kernel = f16 ? names16[cn == 4][prog_id] : names[cn == 4][prog_id];
        if (bf16) info->kernel = bf16_kernel_name(info->kernel);
    }
    if (dry_run) return 1;
    const int ot = bf16 ? 2 : (f16 ? 1 : 0);
    *err = cn == 3 ? launch_yuv_area_fast_cn<3>(ot, prog_id, c, planes, n, s) : launch_yuv_area_fast_cn<4>(ot, prog_id, c, planes, n, s);
    return 1;
}

int launch_yuv_area(const ChainArgs& c, const PlaneParams* inline_planes, int n_inline, uint32_t chain_flags, void* stream, bool dry_run, LaunchInfo* info) {
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (!c.read.table && n_inline > CVGS_KERNARG_PLANES) return -1; // (the caller stages larger batches into a table)
    LaunchCtx one(stream);
    if (!(chain_flags & CVGS_CHAIN_FORCE_GENERIC) && try_yuv_area_fast(c, inline_planes, n_inline, one, dry_run, info, &e))
        return e == hipSuccess ? 0 : -(int)e - 1000;
    if (info) info->kernel = "yuv_area_interp";
    if (dry_run) return 0;
    if (c.read.table) e = launch_yuv_area_t<0>(c, nullptr, 0, s);
    else if (n_inline <= 8) e = launch_yuv_area_t<8>(c, inline_planes, n_inline, s);
    else e = launch_yuv_area_t<CVGS_KERNARG_PLANES>(c, inline_planes, n_inline, s);
    return e == hipSuccess ? 0 : -(int)e - 1000;
}

int launch_yuv_area_many(const ChainArgs& c, const PlaneParams* planes, int n_planes, LaunchCtx& ctx, bool dry_run, LaunchInfo* info) {
    if (!ctx.segs || ctx.n_segs < 1 || ctx.n_segs > CVGS_MAX_CHAINS) return 0;
    hipError_t e = hipSuccess;
    if (!try_yuv_area_fast(c, planes, n_planes, ctx, dry_run, info, &e)) return 0;
    return e == hipSuccess ? 1 : -(int)e - 1000;
}

} // namespace cvgs
