// k_yuv_family.hpp -- what the YUV resize families with one kernel per layout family share (k_nv12.hip: K4, the 4:2:0 layouts;
// k_yuv422.hip: packed 4:2:2; k_yuv444.hip: planar 4:4:4): the geometry block of their kernels, the argument-block forms, and ONE host
// launcher -- the dispatch rules (program matching, the u8 cast move, canonicalisation, argument-block selection, rows per wave), written
// once as a template over a small family-traits type F:
//
//   struct F : YuvFamDefaults {
//       using Geom = ...;                                  // the kernels' second argument: YuvFamGeom or a struct derived from it
//       template <int NPL, class Prog, typename OT, int RPW, int CN, bool WIN> static const void* kernel();   // the entry points
//       static bool eligible(const ReadArgs& r);           // is this read the family's?  (kind and layout)
//       static const char* name(int id);                   // cvgs_kernel_name() of YuvFamName id (CVGS_YUV_FAMILY_NAMES("k_..."))
//       static hipError_t launch_bf16(int prog, ...);      // the OT = __bf16 instantiations, compiled in the family's bf16 twin file
//       // what K4 alone redefines (YuvFamDefaults holds the other families' answers):
//       static constexpr bool kRows4;                      // are there RPW = 4 kernels (fp32, cn 3)?          K4: not for planar chroma
//       static constexpr bool kManyInline;                 // ... NPL < 0 kernels (fused chains, planes in the arguments)?   K4: likewise
//       static int frame_kernel(...);                      // another kernel of the family for whole frames (K4: k_nv12_x2.hip); 0: none
//   };
//
// The kernels keep K1's / K4's mapping (lane = output column, wave = RPW output rows of one plane) and differ in how the taps of a source
// row reach the registers; everything in this file is independent of that.
#pragma once
#include <cstdlib>
#include <memory>
#include <type_traits>

#include "k_taps.hpp"

namespace cvgs {

struct YuvFamGeom {
    int32_t dst_w, dst_h, out_w, cn; // cn: 3, or 4 with alpha
    int64_t img_stride, ch_stride;
    uint8_t* out;
    int32_t out_step; // packed 2D writes: bytes per row
    int32_t packed;   // 0: planar tensor, 1: packed pixels
    // optional second planar target with its own strides (CircularTensor push: history ring + ordered tensor)
    uint8_t* out2;
    int64_t img_stride2, ch_stride2;
    uint32_t col_tiles; // NPL <= 0 (fused chains): blockIdx.x = row group * col_tiles + column tile
    uint32_t pad;
    // fused launches whose tables sit in a pooled slot (NPL == 0; cvgs_api.cpp: ManyPool): the first work-item stores done_value into
    // *done_word (pinned host memory) when the kernel starts -- every earlier launch of the stream has finished by then (as K1 / K4)
    uint64_t* done_word;
    uint64_t done_value;
};

// NPL > 0: the planes travel in the kernel arguments, grid = (column tiles, row groups, planes).  NPL == 0: the chains of a
// cvgs_execute_many launch, planes in per-chain device tables, grid = (column tiles x row groups, planes, chains).
// NPL < 0: the segments with the planes of ALL chains inside the kernel arguments (KernArgsManyInline<-NPL>), as K1 / K4.
template <int NPL> using YuvFamArgs = std::conditional_t<NPL == 0, KernArgsMany, std::conditional_t<(NPL < 0), KernArgsManyInline<(NPL < 0 ? -NPL : 1)>, KernArgs<(NPL > 0 ? NPL : 1)>>>;

constexpr int kYuvFamWaves = 4;
constexpr int kYuvFamTileRow = 80; // floats between the rows of a wave's LDS tile (64 + padding: the 16-byte reads of a row group do not collide)

// what the launcher hands to the instantiation it picks: the call's LaunchCtx and the chains of a cvgs_execute_many launch
struct YuvFamMany {
    LaunchCtx* ctx;
    const ManySeg* segs;
    int n_segs;
    const PlaneParams* planes; // host-described fused chains whose planes travel in the kernel arguments (segs[i].table = first index), or null
    int n_planes;
};

// the names cvgs_kernel_name() reports: <family>_<suffix>
enum YuvFamName {
    kYuvNameU8C3, kYuvNameSwapU8C3, kYuvNameArithU8C3, kYuvNameInterpU8C3, kYuvNameU8C4, kYuvNameSwapU8C4, kYuvNameArithU8C4, kYuvNameInterpU8C4,
    kYuvNameSwapMulSubDivF16, kYuvNameArithF16, kYuvNameInterpF16, kYuvNameSwapMulSubDiv, kYuvNameMulSubDiv, kYuvNameArith, kYuvNameInterp
};
#define CVGS_YUV_FAMILY_NAMES(P)                                                                                                              \
    static const char* name(int id) {                                                                                                         \
        static const char* const n[] = {P "_u8c3", P "_swap_u8c3", P "_arith_u8c3", P "_interp_u8c3", P "_u8c4", P "_swap_u8c4",               \
                                        P "_arith_u8c4", P "_interp_u8c4", P "_swap_mul_sub_div_f16", P "_arith_f16", P "_interp_f16",        \
                                        P "_swap_mul_sub_div", P "_mul_sub_div", P "_arith", P "_interp"};                                     \
        return n[id];                                                                                                                         \
    }

struct YuvFamDefaults {
    static constexpr bool kRows4 = true, kManyInline = true;
    static int frame_kernel(const ChainArgs&, const PlaneParams*, int, bool, bool, const LaunchCtx&, uint32_t, bool, LaunchInfo*) { return 0; }
};

// the staging buffer of an inline tick's argument block (16 KB / 52 KB): one per thread and size, handed over by address (as K1's / K4's)
template <int CAP> static KernArgsManyInline<CAP>& yuv_fam_staged() {
    static thread_local std::unique_ptr<KernArgsManyInline<CAP>> staged;
    if (!staged) staged.reset(new KernArgsManyInline<CAP>());
    return *staged;
}

template <class F, class Prog, typename OT, int RPW, int CN, bool WIN = false>
static hipError_t launch_yuv_fam_r(const ChainArgs& c, const PlaneParams* ip, int ni, const YuvFamGeom& g_in, const YuvFamMany& many) {
    hipStream_t s = (hipStream_t)many.ctx->stream;
    typename F::Geom g{};
    static_cast<YuvFamGeom&>(g) = g_in;
    const uint32_t col_tiles = (uint32_t)((g.dst_w + 63) / 64), row_groups = (uint32_t)((g.dst_h + kYuvFamWaves * RPW - 1) / (kYuvFamWaves * RPW));
    g.col_tiles = col_tiles;
    g.pad = 0;
    g.done_word = nullptr;
    g.done_value = 0;
    const dim3 block(64 * kYuvFamWaves);
    auto launch = [&](auto npl_tag, const dim3& grid, void* a) {
        void* args[] = {a, (void*)&g};
        return hipLaunchKernel(F::template kernel<decltype(npl_tag)::value, Prog, OT, RPW, CN, WIN>(), grid, block, args, 0, s);
    };
    constexpr bool kImage = std::is_same_v<OT, uint8_t>; // packed u8 images: never fused chains, never the 16 KB argument block
    if constexpr (!kImage && !WIN && F::kManyInline) if (many.segs && many.planes) {
        // host descriptors of at most kManyInlineLarge planes: segments + planes in the arguments (16 KB / 52 KB blocks), capturable
        const dim3 grid(col_tiles * row_groups, (unsigned)c.read.batch, (unsigned)many.n_segs);
        auto go = [&](auto cap_tag) {
            constexpr int CAP = decltype(cap_tag)::value;
            KernArgsManyInline<CAP>& a = yuv_fam_staged<CAP>();
            a.c = c;
            for (int i = 0; i < CVGS_MAX_CHAINS; ++i) a.seg[i] = i < many.n_segs ? many.segs[i] : ManySeg{nullptr, nullptr, 0, 0};
            for (int i = 0; i < many.n_planes && i < CAP; ++i) a.planes[i] = many.planes[i];
            (void)launch(std::integral_constant<int, -CAP>{}, grid, &a);
        };
        if (many.n_planes <= kManyInlineSmall) go(std::integral_constant<int, kManyInlineSmall>{});
        else go(std::integral_constant<int, kManyInlineLarge>{});
        return hipGetLastError();
    }
    if constexpr (!kImage && !WIN) if (many.segs) {
        KernArgsMany a;
        a.c = c;
        for (int i = 0; i < CVGS_MAX_CHAINS; ++i) a.seg[i] = i < many.n_segs ? many.segs[i] : ManySeg{nullptr, nullptr, 0, 0};
        LaunchCtx& x = *many.ctx;
        if (x.done_word && !x.done_word_taken) {
            x.done_word_taken = true;
            g.done_word = x.done_word;
            g.done_value = x.done_value;
        }
        (void)launch(std::integral_constant<int, 0>{}, dim3(col_tiles * row_groups, (unsigned)c.read.batch, (unsigned)many.n_segs), &a);
        return hipGetLastError();
    }
    if (many.segs) return hipErrorInvalidValue; // (fused chains are stretch-only planar tensors: the launcher never gets here)
    const dim3 grid(col_tiles, row_groups, c.read.batch);
    auto planes_in_args = [&](auto npl_tag) {
        constexpr int N = decltype(npl_tag)::value;
        KernArgs<N> a;
        a.c = c;
        for (int i = 0; i < N; ++i) a.planes[i] = i < ni ? ip[i] : PlaneParams{};
        (void)launch(npl_tag, grid, &a);
    };
    if (ni <= 8) planes_in_args(std::integral_constant<int, 8>{});
    else if (ni <= CVGS_KERNARG_PLANES) planes_in_args(std::integral_constant<int, CVGS_KERNARG_PLANES>{}); // crop lists of a surface in the kernel arguments
    else if constexpr (!kImage) planes_in_args(std::integral_constant<int, kKernargPlanesBig>{}); // ... up to CVGS_KERNARG_PLANES_MAX in a 16 KB argument block
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

template <class F, class Prog, typename OT = float>
static hipError_t launch_yuv_fam_rows(const ChainArgs& c, const PlaneParams* ip, int ni, const YuvFamGeom& g, const YuvFamMany& s, bool win = false) {
    if (win) return g.cn == 4 ? launch_yuv_fam_r<F, Prog, OT, 1, 4, true>(c, ip, ni, g, s) : launch_yuv_fam_r<F, Prog, OT, 1, 3, true>(c, ip, ni, g, s);
    // launches in the throughput regime (cvgs_execute_many: the crops of several surfaces; one chain of hundreds of crops): four rows per
    // wave, the rows leaving as 16-byte stores through a wave-private LDS tile -- K4's rule and K4's threshold
    if constexpr (std::is_same_v<OT, float> && F::kRows4) {
        if (g.cn == 3) {
            int64_t planes = s.segs ? 0 : c.read.batch;
            for (int i = 0; s.segs && i < s.n_segs; ++i) planes += s.segs[i].batch;
            if (planes * g.dst_h * ((g.dst_w + 63) / 64) >= 32768) return launch_yuv_fam_r<F, Prog, OT, 4, 3>(c, ip, ni, g, s);
        }
    }
    return g.cn == 4 ? launch_yuv_fam_r<F, Prog, OT, 1, 4>(c, ip, ni, g, s) : launch_yuv_fam_r<F, Prog, OT, 1, 3>(c, ip, ni, g, s);
}

// the body of a family's bf16 twin (F::launch_bf16): prog 0 swap-mul-sub-div, 1 canonical, 2 interpreted
template <class F>
static hipError_t launch_yuv_fam_bf16(int prog, const ChainArgs& c, const PlaneParams* ip, int ni, const YuvFamGeom& g, const YuvFamMany& s, bool win) {
    return prog == 0 ? launch_yuv_fam_rows<F, ProgSwapMulSubDiv, __bf16>(c, ip, ni, g, s, win)
                     : (prog == 1 ? launch_yuv_fam_rows<F, K1CanonProg, __bf16>(c, ip, ni, g, s, win) : launch_yuv_fam_rows<F, InterpProg, __bf16>(c, ip, ni, g, s, win));
}

// stretch geometry on every plane?  (otherwise: the windowed instantiations)
static inline bool yuv_fam_stretch(const PlaneParams* planes, int n, int dst_w, int dst_h) {
    for (int i = 0; i < n; ++i) {
        const PlaneParams& P = planes[i];
        if (P.x1 != 0 || P.y1 != 0 || P.x2 != dst_w - 1 || P.y2 != dst_h - 1) return false;
    }
    return true;
}

// Returns 1 if it took the chain, 0 if not eligible, <0 on error.
// ctx.segs (n_segs >= 1): the chains of a cvgs_execute_many launch -- stretch geometry, checked by the caller;
// c_in.read.batch is the largest batch.  nullptr: one chain (inline_planes).  Any plane width is served (K4 refuses narrow rows before
// it comes here).  chain_flags: for F::frame_kernel.
template <class F>
static int launch_yuv_family(const ChainArgs& c_in, const PlaneParams* inline_planes, int n_inline, LaunchCtx& ctx, bool dry_run, LaunchInfo* info,
                             uint32_t chain_flags = 0) {
    const ManySeg* const segs = ctx.segs;
    const int n_segs = ctx.n_segs;
    const ReadArgs& r = c_in.read;
    if (!F::eligible(r)) return 0;
    // fp16 / bf16 planar tensors: the trailing CAST(CV_16F / CV_16BF) moves into the store (a bf16 chain of any other shape: the
    // interpreted kernel); "f16" below means "a 16-bit float store" from here on
    const bool planar_kind = c_in.write.kind == CVGS_WRITE_TENSOR_SPLIT || c_in.write.kind == CVGS_WRITE_TENSOR_T_SPLIT;
    const bool trailing_cast = c_in.prog.n >= 1 && c_in.prog.opcode[c_in.prog.n - 1] == CVGS_OP_CAST;
    const bool bf16 = planar_kind && c_in.write.depth == kDepthBF16 && trailing_cast;
    if (chain_has_bf16(c_in) && !bf16) return 0;
    const bool f16 = planar_kind && (c_in.write.depth == CVGS_DEPTH_16F || bf16) && trailing_cast;
    ChainArgs c_cut;
    if (f16) {
        c_cut = c_in;
        c_cut.prog.n -= 1;
        for (int k = 0; k < c_cut.prog.n; ++k)
            if (c_cut.prog.opcode[k] == CVGS_OP_CAST || c_cut.prog.opcode[k] == CVGS_OP_CAST_TRUNC) return 0;
    }
    const ChainArgs& c = f16 ? c_cut : c_in;
    if (segs) {
        if (n_segs < 1 || n_segs > CVGS_MAX_CHAINS || c_in.write.data2) return 0;
        if (!r.table && (!F::kManyInline || !inline_planes || n_inline < 1 || n_inline > kManyInlineLarge)) return 0; // segments without a table: planes in the arguments
    } else {
        if (r.table || n_inline > kKernargPlanesBig) return 0; // resident tables: generic kernel
        if (n_inline > CVGS_KERNARG_PLANES && !(planar_kind && (c_in.write.depth == CVGS_DEPTH_32F || f16))) return 0; // the large block: tensors only
    }
    if (r.batch > 65535) return 0;
    const WriteArgs& w = c.write;
    const bool planar = planar_kind && (w.depth == CVGS_DEPTH_32F || f16);
    const bool packed = w.kind == CVGS_WRITE_PIXEL_2D || w.kind == CVGS_WRITE_PIXEL_3D;
    if (!planar && !packed) return 0;
    if (segs && !planar) return 0; // fused chains: planar tensors only
    const int swap = r.out_cn == 3 ? (2 | (1 << 2) | (0 << 4)) : (2 | (1 << 2) | (0 << 4) | (3 << 6));

    // packed u8 images (camera frame -> thumbnail / display image): resize -> [REORDER / MUL / ADD / SUB / DIV in float] -> CAST(CV_8U) ->
    // write.  The trailing SaturateCast becomes the store's conversion and the store a coalesced tile (K4's rules).
    bool u8img = false;
    int u8_prog = 2; // 0: nothing in front of the cast, 1: the R<->B swap only, 2: interpreted / canonical
    ChainArgs c8 = c;
    // a cast followed by a pure permutation of the bytes: the permutation commutes with the per-channel cast, so the cast moves to the end
    if (c8.prog.n >= 2 && c8.prog.opcode[c8.prog.n - 1] == CVGS_OP_REORDER && c8.prog.opcode[c8.prog.n - 2] == CVGS_OP_CAST &&
        c8.prog.aux[c8.prog.n - 2] == CVGS_DEPTH_8U) {
        const int a = c8.prog.n - 2, b = c8.prog.n - 1;
        std::swap(c8.prog.opcode[a], c8.prog.opcode[b]);
        std::swap(c8.prog.aux[a], c8.prog.aux[b]);
        for (int k = 0; k < 4; ++k) std::swap(c8.prog.operand[a][k], c8.prog.operand[b][k]);
    }
    if (packed && !f16 && !segs && w.depth == CVGS_DEPTH_8U && n_inline <= CVGS_KERNARG_PLANES && c8.prog.n >= 1 &&
        c8.prog.opcode[c8.prog.n - 1] == CVGS_OP_CAST && c8.prog.aux[c8.prog.n - 1] == CVGS_DEPTH_8U) {
        u8img = true;
        for (int k = 0; k + 1 < c8.prog.n; ++k) {
            const int op = c8.prog.opcode[k];
            const bool arith = op == CVGS_OP_MUL || op == CVGS_OP_ADD || op == CVGS_OP_SUB || op == CVGS_OP_DIV || op == CVGS_OP_REORDER || op == CVGS_OP_NOP;
            if (!arith && !(op == CVGS_OP_CAST && c8.prog.aux[k] == CVGS_DEPTH_32F)) u8img = false; // the value stays out_cn floats up to the cast
        }
        if (c8.prog.n == 1) u8_prog = 0;
        else if (c8.prog.n == 2 && c8.prog.opcode[0] == CVGS_OP_REORDER && c8.prog.aux[0] == swap) u8_prog = 1;
    }
    const bool stretch = yuv_fam_stretch(inline_planes, n_inline, r.dst_w, r.dst_h);
    if (u8img) {
        c8.prog.n -= 1;
        c8.prog.fast_div = 0;
        bool canon8 = false; // brightness / contrast on the way to a u8 image, ...: the canonical arithmetic program (k_taps.hpp)
        if (u8_prog == 2) {
            ProgArgs canon;
            if (k1_canonicalise(c8.prog, r.out_cn, canon)) {
                c8.prog = canon;
                canon8 = true;
            }
        }
        YuvFamGeom g8{};
        g8.dst_w = r.dst_w; g8.dst_h = r.dst_h; g8.out_w = w.width; g8.cn = r.out_cn;
        g8.out = w.data; g8.out_step = w.step; g8.packed = 1;
        if (info) info->kernel = F::name((r.out_cn == 3 ? kYuvNameU8C3 : kYuvNameU8C4) + (u8_prog == 0 ? 0 : (u8_prog == 1 ? 1 : (canon8 ? 2 : 3))));
        if (dry_run) return 1;
        const YuvFamMany s8{&ctx, nullptr, 0, nullptr, 0};
        const bool win8 = r.used != r.batch || !stretch;
        const hipError_t e8 = u8_prog == 0   ? launch_yuv_fam_rows<F, ProgNone, uint8_t>(c8, inline_planes, n_inline, g8, s8, win8)
                              : u8_prog == 1 ? launch_yuv_fam_rows<F, K1Prog<kOpSwapRB>, uint8_t>(c8, inline_planes, n_inline, g8, s8, win8)
                              : canon8       ? launch_yuv_fam_rows<F, K1CanonProg, uint8_t>(c8, inline_planes, n_inline, g8, s8, win8)
                                             : launch_yuv_fam_rows<F, InterpProg, uint8_t>(c8, inline_planes, n_inline, g8, s8, win8);
        return e8 == hipSuccess ? 1 : -(int)e8 - 1000;
    }

    YuvFamGeom g{};
    g.dst_w = r.dst_w; g.dst_h = r.dst_h; g.out_w = w.width; g.cn = r.out_cn;
    g.img_stride = w.img_stride; g.ch_stride = w.ch_stride;
    g.out = w.data; g.out_step = w.step; g.packed = packed ? 1 : 0;
    g.out2 = w.data2; g.img_stride2 = w.img_stride2; g.ch_stride2 = w.ch_stride2;

    const ProgArgs& p = c.prog;
    const bool fast_prog = planar && p.n == 4 && p.opcode[0] == CVGS_OP_REORDER && p.aux[0] == swap &&
                           p.opcode[1] == CVGS_OP_MUL && p.opcode[2] == CVGS_OP_SUB && p.opcode[3] == CVGS_OP_DIV;
    // the same normalisation in the surface's own R, G, B order (no swap)
    const bool fast_rgb = planar && !f16 && p.n == 3 && p.opcode[0] == CVGS_OP_MUL && p.opcode[1] == CVGS_OP_SUB && p.opcode[2] == CVGS_OP_DIV;
    ChainArgs c_fd = c;
    c_fd.prog.fast_div = 0;
    for (int k = 0; k < 4; ++k) c_fd.prog.rdiv[k] = 0.f;
    if (fast_prog) fast_div_setup(c_fd.prog, 3, 1, r.out_cn, r.bg); // division by the host reciprocal under K1's / K4's guards
    else if (fast_rgb) fast_div_setup(c_fd.prog, 2, 0, r.out_cn, r.bg);
    if (fast_prog || fast_rgb) { // the two compile-time normalisations at frame size: the family may have another kernel for them
        const int rc = F::frame_kernel(c_fd, inline_planes, n_inline, fast_prog, f16, ctx, chain_flags, dry_run, info);
        if (rc != 0) return rc;
    }
    // any other chain of the canonical arithmetic shape ([swap] {mul|add|sub} x 0..2 [div] {mul|add|sub} x 0..2): the straight-line K1CanonProg
    bool canon_prog = false;
    if (!fast_prog && !(fast_rgb && !f16)) { // (planar tensors and packed fp32 / fp16 pixels alike)
        ProgArgs canon;
        if (k1_canonicalise(c_fd.prog, r.out_cn, canon)) {
            c_fd.prog = canon;
            canon_prog = true;
        }
    }
    if (info)
        info->kernel = F::name(f16 ? (fast_prog ? kYuvNameSwapMulSubDivF16 : (canon_prog ? kYuvNameArithF16 : kYuvNameInterpF16))
                                   : (fast_prog ? kYuvNameSwapMulSubDiv : (fast_rgb ? kYuvNameMulSubDiv : (canon_prog ? kYuvNameArith : kYuvNameInterp))));
    if (info && bf16) info->kernel = bf16_kernel_name(info->kernel);
    if (dry_run) return 1;
    const YuvFamMany s{&ctx, segs, n_segs, segs && !r.table ? inline_planes : nullptr, segs && !r.table ? n_inline : 0};
    // the windowed instantiations: an aspect-ratio window or default-value planes (never for fused chains / staged tables, whose
    // callers admit stretch geometry only)
    const bool win = !segs && (r.used != r.batch || !stretch);
    hipError_t e;
    if (bf16) e = F::launch_bf16(fast_prog ? 0 : (canon_prog ? 1 : 2), c_fd, inline_planes, n_inline, g, s, win);
    else if (f16) e = fast_prog ? launch_yuv_fam_rows<F, ProgSwapMulSubDiv, _Float16>(c_fd, inline_planes, n_inline, g, s, win)
                           : (canon_prog ? launch_yuv_fam_rows<F, K1CanonProg, _Float16>(c_fd, inline_planes, n_inline, g, s, win)
                                         : launch_yuv_fam_rows<F, InterpProg, _Float16>(c_fd, inline_planes, n_inline, g, s, win));
    else if (fast_prog) e = launch_yuv_fam_rows<F, ProgSwapMulSubDiv>(c_fd, inline_planes, n_inline, g, s, win);
    else if (fast_rgb) e = launch_yuv_fam_rows<F, ProgMulSubDiv>(c_fd, inline_planes, n_inline, g, s, win);
    else e = canon_prog ? launch_yuv_fam_rows<F, K1CanonProg>(c_fd, inline_planes, n_inline, g, s, win) : launch_yuv_fam_rows<F, InterpProg>(c_fd, inline_planes, n_inline, g, s, win);
    return e == hipSuccess ? 1 : -(int)e - 1000;
}

} // namespace cvgs
