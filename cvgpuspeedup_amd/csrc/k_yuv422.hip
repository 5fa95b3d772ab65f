// k_yuv422.hip -- packed 4:2:2 surfaces (YUYV / UYVY: capture cards, V4L2 cameras, 4:2:2 JPEG decoders) read back inside the bilinear
// resize: each of the 4 taps is converted YCbCr -> RGB(A) in float (k_common.hpp: k4_tap, the 4:2:0 kernels' conversion), THEN
// interpolated, pushed through the pointwise program and written -- planar fp32 / fp16 / bf16 tensor, packed fp32 / fp16 pixels, packed
// u8 image: the targets K4 (k_nv12.hip) serves for NV12, with K4's dispatch rules.
//
// Mapping (as K1 / K4): lane = output column, wave = RPW output rows of one plane, blockIdx.y / .z = row group / plane (fused chains:
// plane / chain).  A row of the surface is a sequence of 4-byte pixel pairs {Y0 U Y1 V} (UYVY: {U Y0 V Y1}); the taps x1 and x1 + 1 lie
// in pair m = x1 >> 1 and at most m + 1, so ONE 8-byte load at 4 * m -- clamped back into the row when m is the last pair; rows of a
// single pair: one 4-byte load -- brings both lumas and both chroma pairs of a source row: two loads per output pixel, 4-byte aligned,
// where K4 needs four.  The twelve samples are picked out of the two windows with v_perm_b32; the byte order is a wave-uniform XOR on
// the selectors, not a second set of kernels.  The bytes a plane reads are [0, 4 * ceil(w / 2)) of each of its rows, nothing else.
#include "k_yuv_family.hpp"

namespace cvgs {

typedef uint32_t y422_u32x2 __attribute__((ext_vector_type(2)));
typedef y422_u32x2 y422_u32x2_a4 __attribute__((aligned(4)));
typedef const __attribute__((address_space(1))) y422_u32x2_a4* gptr_pair2; // two pixel pairs
typedef const __attribute__((address_space(1))) uint32_t* gptr_pair1;      // one pixel pair

// the geometry block, the argument-block forms (NPL > 0 / == 0 / < 0) and the launcher are the YUV families' common ones (k_yuv_family.hpp)
struct Y422Geom : YuvFamGeom {}; // (a type of its own: part of the kernels' signature)

// RPW output rows per wave; CN output channels (3, or 4 with alpha).  WIN: the target may hold an aspect-ratio window and default-value
// planes (usedPlanes < BATCH) -- K1's / K4's machinery: the background value runs through the program once, pixels outside the window
// take it; a separate instantiation, so that stretch-only launches do not pay for the selects.
// All but the tap fetch stands in k_nv12.hip and in the other 4:x:x file as well, and a fix to one belongs in all three: writing it once
// changes the machine code.
template <int NPL, class Prog, typename OT = float, int RPW = 1, int CN = 3, bool WIN = false>
__global__ __launch_bounds__(64 * kYuvFamWaves) void k_yuv422_resize(const YuvFamArgs<NPL> a, const Y422Geom g) {
    const ChainArgs& c = a.c;
    const int dst_w = g.dst_w, dst_h = g.dst_h, W = g.out_w;
    PlaneParams P;
    int z, col_tile, row_group, used;
    uint8_t* out_base;
    if constexpr (NPL <= 0) {
        z = (int)blockIdx.y;
        const ManySeg sg = a.seg[blockIdx.z];
        if (z >= sg.batch) return; // a shorter chain of the fused launch
        used = sg.used;
        if constexpr (NPL == 0) P = sg.table[z < used ? z : 0];
        else P = a.planes[(uint32_t)(uintptr_t)sg.table + (uint32_t)(z < used ? z : 0)]; // (sg.table: the chain's first index into a.planes)
        out_base = sg.out;
        col_tile = 0;
        row_group = (int)blockIdx.x;
        if (g.col_tiles > 1) { // the quotient comes out of the VALU: hand it back to the scalar side explicitly
            col_tile = __builtin_amdgcn_readfirstlane((int)(blockIdx.x % g.col_tiles));
            row_group = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / g.col_tiles));
        }
    } else {
        z = (int)blockIdx.z;
        used = c.read.used;
        P = a.planes[z];
        out_base = g.out;
        col_tile = (int)blockIdx.x;
        row_group = (int)blockIdx.y;
    }
    const int yuv_range = c.read.yuv_range, yuv_prim = c.read.yuv_primaries, packed = g.packed;
    const uint32_t uyvy = c.read.yuv_layout == CVGS_YUV_UYVY ? 1u : 0u; // wave-uniform: every sample sits at its YUYV byte ^ 1
    const int64_t img_stride = g.img_stride, ch_stride = g.ch_stride;
    typedef float f32x4s __attribute__((ext_vector_type(4)));
    const f32x4s op0 = *(const f32x4s*)c.prog.operand[0], op1 = *(const f32x4s*)c.prog.operand[1],
                 op2 = *(const f32x4s*)c.prog.operand[2], op3 = *(const f32x4s*)c.prog.operand[3];
    // one batch of scalar loads, one wait, in front of the first branch (see k_k1.hip)
    if constexpr (WIN) asm volatile("" ::"s"(used), "s"(P.x1), "s"(P.y1), "s"(P.x2), "s"(P.y2));
    asm volatile("" ::"s"(dst_w), "s"(dst_h), "s"(W), "s"(CN), "s"(P.w), "s"(P.h), "s"(P.step), "s"(P.fx), "s"(P.fy), "s"(P.data),
                 "s"(yuv_range), "s"(yuv_prim), "s"(uyvy), "s"(packed), "s"(img_stride), "s"(ch_stride), "s"(out_base), "s"(op0), "s"(op1),
                 "s"(op2), "s"(op3));
    // (behind the scalar loads: a store in front of them would make the compiler fetch the descriptors with vector loads)
    if constexpr (NPL == 0) {
        if (g.done_word && (blockIdx.x | blockIdx.y | blockIdx.z) == 0 && threadIdx.x == 0)
            __hip_atomic_store(g.done_word, g.done_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const YuvK yk = yuv_matrix(yuv_range, yuv_prim, CVGS_YUV_NV12); // 8-bit samples: the 4:2:0 layouts' constants

    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const int x = col_tile * 64 + lane;
    const int row0 = (row_group * kYuvFamWaves + wave) * RPW;
    if (row0 >= dst_h || x >= dst_w) return;

    // one output pixel of row y (wave-uniform row pointers; planar: non-temporal rows, packed: one store per pixel / a coalesced u8 tile)
    auto store_px = [&](const Px& p, int depth, int cn, int y) {
    if constexpr (std::is_same_v<OT, uint8_t>) {
        // packed u8 images (thumbnails, display surfaces): the chain's trailing SaturateCast is the store's conversion
        const WriteArgs& w = c.write;
        auto put = [&](uint8_t* row) {
            if constexpr (CN == 4) {
                typedef uint32_t u32a1 __attribute__((aligned(1)));
                const uint32_t q = sat_u8_insert(p.v[3], 3, sat_u8_insert(p.v[2], 2, sat_u8_insert(p.v[1], 1, sat_u8_insert(p.v[0], 0, 0))));
                __builtin_nontemporal_store(q, (u32a1*)(row + (size_t)x * 4));
            } else {
                if (col_tile * 64 + 63 < dst_w) store_u8c3_tile(row + (size_t)(col_tile * 64) * 3, lane, p.v); // wave-uniform: every lane is alive
                else store_packed_px<3, uint8_t>(row + (size_t)x * 3, p.v, 3);
            }
        };
        put(w.kind == CVGS_WRITE_PIXEL_2D ? w.data + (size_t)y * (size_t)w.step : w.data + ((size_t)z * w.img_stride + (size_t)y * (size_t)W) * CN);
        if (w.kind == CVGS_WRITE_PIXEL_3D && w.data2) // wave-uniform (a second target with its own image stride)
            put(w.data2 + ((size_t)z * w.img_stride2 + (size_t)y * (size_t)W) * CN);
    } else if (packed) {
        const WriteArgs& w = c.write;
        if (depth == CVGS_DEPTH_32F && cn == CN) { // wave-uniform: packed float pixels leave as ONE dwordx3 / x4 store per lane
            float* const px = w.kind == CVGS_WRITE_PIXEL_2D ? (float*)(w.data + (size_t)y * (size_t)w.step) + (size_t)x * CN
                                                            : (float*)w.data + ((size_t)z * w.img_stride + (size_t)y * (size_t)W + x) * CN;
            store_packed_px<CN, float>(px, p.v, CN);
            if (w.kind == CVGS_WRITE_PIXEL_3D && w.data2)
                store_packed_px<CN, float>((float*)w.data2 + ((size_t)z * w.img_stride2 + (size_t)y * (size_t)W + x) * CN, p.v, CN);
        } else {
            write_px(c.write, c.dst_inline, x, y, z, p, depth, cn);
        }
    } else {
        // OT = _Float16 / __bf16: the chain's trailing CAST is this round-to-nearest-even conversion
        const uint32_t xb = (uint32_t)x * (uint32_t)sizeof(OT);
        OT* const orow = (OT*)out_base + (int64_t)z * img_stride + (int64_t)y * W;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cn) st_row(orow + (int64_t)k * ch_stride, xb, p.v[k]);
        if (g.out2) { // wave-uniform
            OT* const orow2 = (OT*)g.out2 + (int64_t)z * g.img_stride2 + (int64_t)y * W;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cn) st_row(orow2 + (int64_t)k * g.ch_stride2, xb, p.v[k]);
        }
    }
    };
    // does the source cover the whole target?  (always, except aspect-ratio padding and planes >= usedPlanes; wave-uniform.)
    const bool whole = !WIN || (z < used && ((P.x1 | P.y1 | (P.x2 ^ (dst_w - 1)) | (P.y2 ^ (dst_h - 1))) == 0));
    Px bgp;
    bgp.v[0] = bgp.v[1] = bgp.v[2] = bgp.v[3] = 0.f;
    bool in_x = true;
    int xr = x;
    if constexpr (WIN) {
        int bg_cn = CN, bg_depth = CVGS_DEPTH_32F;
        if (!whole) {
#pragma unroll
            for (int k = 0; k < 4; ++k) bgp.v[k] = k < CN ? c.read.bg[k] : 0.f;
            Prog::run(c.prog, bgp, bg_depth, bg_cn);
        }
        if (z >= used) { // a default-value plane: nothing is read
#pragma unroll
            for (int j = 0; j < RPW; ++j)
                if (row0 + j < dst_h) store_px(bgp, bg_depth, bg_cn, row0 + j);
            return;
        }
        in_x = x >= P.x1 && x <= P.x2;
        xr = in_x ? x - P.x1 : 0;
    }

    // column geometry (once per lane, reused for every row).  Tap coordinates are clamped into the plane before they address anything.
    const float sx = (float)xr * P.fx;
    const int x1 = (int)floorf(sx);
    const int x2 = x1 + 1;
    const float wxa = (float)x2 - sx, wxb = sx - (float)x1;
    const int xa = max(0, min(x1, P.w - 1)), xb2 = max(xa, min(x2, P.w - 1)); // taps 0 / 1 (tap 1 repeats tap 0 at the right edge)
    const int npairs = (P.w + 1) >> 1; // wave-uniform; >= 1
    const bool single = npairs < 2;    // rows of one pixel pair: a 4-byte window
    const int m0 = xa >> 1, m1 = xb2 >> 1;
    const int wp = single ? 0 : min(m0, npairs - 2); // first pair of the 8-byte window: clamped back into the row at the last pair
    const uint32_t wo = (uint32_t)wp * 4u;
    // v_perm_b32 selectors into the window's 8 bytes (YUYV: luma at 4 * pair + 2 * (x & 1), U at 4 * pair + 1, V at 4 * pair + 3; UYVY: ^ 1):
    //   sel_yu -> {Y tap 0, Y tap 1, U tap 0, U tap 1},  sel_v -> {V tap 0, V tap 1, 0, 0}
    const uint32_t b0 = (uint32_t)(m0 - wp) * 4u, b1 = (uint32_t)(m1 - wp) * 4u;
    const uint32_t sel_yu = ((b0 + 2u * (uint32_t)(xa & 1)) | ((b1 + 2u * (uint32_t)(xb2 & 1)) << 8) | ((b0 + 1u) << 16) | ((b1 + 1u) << 24)) ^ (uyvy * 0x01010101u);
    const uint32_t sel_v = (((b0 + 3u) | ((b1 + 3u) << 8)) ^ (uyvy * 0x00000101u)) | 0x0c0c0000u;
    const gptr_u8 base = (gptr_u8)P.data;
    const size_t step = (size_t)P.step;

    uint32_t wa_lo[RPW], wa_hi[RPW], wb_lo[RPW], wb_hi[RPW]; // the windows of source rows y1 / y2
    float wya[RPW], wyb[RPW];
    bool in_y[RPW];
    // four rows per wave into a planar fp32 tensor: a full 64-column tile with all four rows inside the target leaves through the LDS transpose
    constexpr bool kRowsTile = RPW == 4 && std::is_same_v<OT, float> && !WIN;
    [[maybe_unused]] const bool tile_rows = kRowsTile && !packed && !g.out2 && col_tile * 64 + 63 < dst_w && row0 + RPW <= dst_h;
    [[maybe_unused]] float tv[RPW][4];
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        // row geometry (wave-uniform)
        const int y = min(row0 + j, dst_h - 1);
        in_y[j] = !WIN || (y >= P.y1 && y <= P.y2);
        const int yr = WIN ? (in_y[j] ? y - P.y1 : 0) : y;
        const float sy = (float)yr * P.fy;
        const int y1 = (int)floorf(sy);
        const int y2 = y1 + 1;
        wya[j] = (float)y2 - sy;
        wyb[j] = sy - (float)y1;
        const int r1 = __builtin_amdgcn_readfirstlane(max(0, min(y1, P.h - 1))), r2 = __builtin_amdgcn_readfirstlane(max(0, min(y2, P.h - 1)));
        const gptr_u8 ra = pin_uniform(base + (size_t)r1 * step);
        const gptr_u8 rb = pin_uniform(base + (size_t)r2 * step);
        if (single) { // wave-uniform
            wa_lo[j] = wa_hi[j] = *(gptr_pair1)(ra + wo);
            wb_lo[j] = wb_hi[j] = *(gptr_pair1)(rb + wo);
        } else {
            const y422_u32x2 qa = *(gptr_pair2)(ra + wo), qb = *(gptr_pair2)(rb + wo);
            wa_lo[j] = qa.x; wa_hi[j] = qa.y;
            wb_lo[j] = qb.x; wb_hi[j] = qb.y;
        }
    }

#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const int y = row0 + j;
        if (y >= dst_h) break; // wave-uniform
        // {Y0, Y1, U0, U1} and {V0, V1} of row a / row b
        const uint32_t ayu = __builtin_amdgcn_perm(wa_hi[j], wa_lo[j], sel_yu), av = __builtin_amdgcn_perm(wa_hi[j], wa_lo[j], sel_v);
        const uint32_t byu = __builtin_amdgcn_perm(wb_hi[j], wb_lo[j], sel_yu), bv = __builtin_amdgcn_perm(wb_hi[j], wb_lo[j], sel_v);
        float fy[4], fu[4], fv[4]; // taps 00, 10, 01, 11
        fy[0] = (float)(ayu & 0xffu); fy[1] = (float)((ayu >> 8) & 0xffu); fu[0] = (float)((ayu >> 16) & 0xffu); fu[1] = (float)(ayu >> 24);
        fy[2] = (float)(byu & 0xffu); fy[3] = (float)((byu >> 8) & 0xffu); fu[2] = (float)((byu >> 16) & 0xffu); fu[3] = (float)(byu >> 24);
        fv[0] = (float)(av & 0xffu); fv[1] = (float)((av >> 8) & 0xffu);
        fv[2] = (float)(bv & 0xffu); fv[3] = (float)((bv >> 8) & 0xffu);

        float t00[4], t10[4], t01[4], t11[4];
        if (yuv_range == CVGS_YUV_FULL) { // wave-uniform
            k4_tap<CN, true>(fy[0], fu[0], fv[0], yk, t00);
            k4_tap<CN, true>(fy[1], fu[1], fv[1], yk, t10);
            k4_tap<CN, true>(fy[2], fu[2], fv[2], yk, t01);
            k4_tap<CN, true>(fy[3], fu[3], fv[3], yk, t11);
        } else {
            k4_tap<CN, false>(fy[0], fu[0], fv[0], yk, t00);
            k4_tap<CN, false>(fy[1], fu[1], fv[1], yk, t10);
            k4_tap<CN, false>(fy[2], fu[2], fv[2], yk, t01);
            k4_tap<CN, false>(fy[3], fu[3], fv[3], yk, t11);
        }

        const float w00 = wxa * wya[j], w10 = wxb * wya[j], w01 = wxa * wyb[j], w11 = wxb * wyb[j];
        Px p;
        p.v[3] = 0.f;
#pragma unroll
        for (int k = 0; k < CN; ++k) {
            float acc = t00[k] * w00;
            acc = acc + t10[k] * w10;
            acc = acc + t01[k] * w01;
            acc = acc + t11[k] * w11;
            p.v[k] = acc;
        }
        int depth = CVGS_DEPTH_32F, cn = CN;
        Prog::run(c.prog, p, depth, cn);
        if constexpr (WIN) {
            if (!whole) { // wave-uniform: only padded planes pay the per-lane select
                const bool take = in_x && in_y[j];
#pragma unroll
                for (int k = 0; k < 4; ++k) p.v[k] = take ? p.v[k] : bgp.v[k];
            }
        }

        if constexpr (kRowsTile) {
            if (tile_rows) { // wave-uniform: the wave's four rows leave together below
#pragma unroll
                for (int k = 0; k < CN; ++k) tv[j][k] = p.v[k];
                continue;
            }
        }
        store_px(p, depth, cn, y);
    }
    if constexpr (kRowsTile) {
        if (tile_rows) {
            // the lane = column register layout transposed through a wave-private LDS tile: lane l then owns 4 consecutive columns of row
            // l / 16 -- 16 bytes per lane and store instruction, three stores for the wave's four rows instead of twelve (as K4)
            __shared__ __attribute__((aligned(16))) float tiles[kYuvFamWaves][CN * RPW * kYuvFamTileRow];
            float* const tile = tiles[wave];
#pragma unroll
            for (int k = 0; k < CN; ++k)
#pragma unroll
                for (int j = 0; j < RPW; ++j) tile[(k * RPW + j) * kYuvFamTileRow + lane] = tv[j][k];
            __builtin_amdgcn_wave_barrier(); // (compiler ordering only: one wave's LDS operations run in order)
            typedef float f32x4t __attribute__((ext_vector_type(4)));
            typedef f32x4t f32x4t_a4 __attribute__((aligned(4)));
            typedef __attribute__((address_space(1))) f32x4t_a4* gf4;
            const int i = lane >> 4, q = lane & 15;
            float* const orow = (float*)out_base + (int64_t)z * img_stride + (int64_t)(row0 + i) * W + col_tile * 64 + q * 4;
#pragma unroll
            for (int k = 0; k < CN; ++k) {
                const f32x4t o = *(const f32x4t*)(tile + (k * RPW + i) * kYuvFamTileRow + q * 4);
                __builtin_nontemporal_store(o, (gf4)(orow + (int64_t)k * ch_stride));
            }
        }
    }
}

// the family's traits for the shared launcher (k_yuv_family.hpp)
hipError_t y422_launch_bf16(int prog, const ChainArgs& c, const PlaneParams* ip, int ni, const YuvFamGeom& g, const YuvFamMany& s, bool win);
struct Y422Family : YuvFamDefaults {
    using Geom = Y422Geom;
    template <int NPL, class Prog, typename OT, int RPW, int CN, bool WIN> static const void* kernel() {
        return (const void*)&k_yuv422_resize<NPL, Prog, OT, RPW, CN, WIN>;
    }
    static bool eligible(const ReadArgs& r) {
        return r.kind == CVGS_READ_NV12_RESIZE_LINEAR && (r.yuv_layout == CVGS_YUV_YUYV || r.yuv_layout == CVGS_YUV_UYVY);
    }
    CVGS_YUV_FAMILY_NAMES("k_yuv422_resize")
    static hipError_t launch_bf16(int prog, const ChainArgs& c, const PlaneParams* ip, int ni, const YuvFamGeom& g, const YuvFamMany& s, bool win) {
        return y422_launch_bf16(prog, c, ip, ni, g, s, win);
    }
};

// bf16 (CV_16BF) planar tensors: the fp16 instantiations' twins with OT = __bf16, compiled in k_yuv422_bf16.hip (this file included with
// CVGS_Y422_BF16_TU, so the bf16 kernels build in parallel with the others).
#ifdef CVGS_Y422_BF16_TU
hipError_t y422_launch_bf16(int prog, const ChainArgs& c, const PlaneParams* ip, int ni, const YuvFamGeom& g, const YuvFamMany& s, bool win) {
    return launch_yuv_fam_bf16<Y422Family>(prog, c, ip, ni, g, s, win);
}
#else
// 1 launched / 0 not eligible / < 0 error.  Narrow rows take the
// 4-byte window, so any plane width is served.
int launch_yuv422(const ChainArgs& c_in, const PlaneParams* inline_planes, int n_inline, LaunchCtx& ctx, bool dry_run, LaunchInfo* info) {
    return launch_yuv_family<Y422Family>(c_in, inline_planes, n_inline, ctx, dry_run, info);
}
#endif // CVGS_Y422_BF16_TU

} // namespace cvgs
