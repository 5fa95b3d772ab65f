// k_yuv444.hip -- planar 4:4:4 surfaces (I444: rocDecode's YUV444 output of 4:4:4 HEVC / AV1 streams, rocJPEG's output for non-subsampled
// JPEGs) read back inside the bilinear resize: each of the 4 taps is converted YCbCr -> RGB(A) in float (k_common.hpp: k4_tap, the 4:2:0
// kernels' conversion), THEN interpolated, pushed through the pointwise program and written -- planar fp32 / fp16 / bf16 tensor, packed
// fp32 / fp16 pixels, packed u8 image: the targets K4 (k_nv12.hip) and k_yuv422_resize serve, with their dispatch rules (the shared
// launcher of k_yuv_family.hpp).
//
// Mapping (as K1 / K4): lane = output column, wave = RPW output rows of one plane, blockIdx.y / .z = row group / plane (fused chains:
// plane / chain).  The surface is three full-resolution planes Y, U, V that share one step and lie uv_off bytes apart; the taps x1 and
// x1 + 1 of a source row of a plane arrive in ONE 2-byte load at column x1 -- clamped back into the row when x1 is the last column; rows
// of width 1: one byte load -- so an output pixel costs six loads (3 planes x 2 rows), all issued before the first is used.  Nothing is
// assumed about the alignment of data, step or uv_off; row bases are wave-uniform, lane offsets 32-bit, and the three plane bases are
// computed once per wave on the scalar side.  The bytes a plane reads are [0, w) of each of its h rows in each of the three planes.
#include "k_yuv_family.hpp"

namespace cvgs {

typedef uint16_t y444_u16u __attribute__((aligned(1)));
typedef const __attribute__((address_space(1))) y444_u16u* gptr_tap2; // both horizontal taps of one source row of one plane

// RPW output rows per wave; CN output channels (3, or 4 with alpha).  WIN: the target may hold an aspect-ratio window and default-value
// planes (usedPlanes < BATCH) -- K1's / K4's machinery: the background value runs through the program once, pixels outside the window
// take it; a separate instantiation, so that stretch-only launches do not pay for the selects.
// All but the tap fetch stands in k_nv12.hip and in the other 4:x:x file as well, and a fix to one belongs in all three: writing it once
// changes the machine code.
template <int NPL, class Prog, typename OT = float, int RPW = 1, int CN = 3, bool WIN = false>
__global__ __launch_bounds__(64 * kYuvFamWaves) void k_yuv444_resize(const YuvFamArgs<NPL> a, const YuvFamGeom g) {
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
    const int64_t img_stride = g.img_stride, ch_stride = g.ch_stride;
    typedef float f32x4s __attribute__((ext_vector_type(4)));
    const f32x4s op0 = *(const f32x4s*)c.prog.operand[0], op1 = *(const f32x4s*)c.prog.operand[1],
                 op2 = *(const f32x4s*)c.prog.operand[2], op3 = *(const f32x4s*)c.prog.operand[3];
    // one batch of scalar loads, one wait, in front of the first branch (see k_k1.hip)
    if constexpr (WIN) asm volatile("" ::"s"(used), "s"(P.x1), "s"(P.y1), "s"(P.x2), "s"(P.y2));
    asm volatile("" ::"s"(dst_w), "s"(dst_h), "s"(W), "s"(CN), "s"(P.w), "s"(P.h), "s"(P.step), "s"(P.fx), "s"(P.fy), "s"(P.data), "s"(P.uv_off),
                 "s"(yuv_range), "s"(yuv_prim), "s"(packed), "s"(img_stride), "s"(ch_stride), "s"(out_base), "s"(op0), "s"(op1),
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
    // both taps of a source row of a plane lie in ONE 2-byte window at xa -- clamped back into the row when xa is the last column; rows of
    // a single pixel: a 1-byte window.  s0 / s1: the bit position of tap 0 / 1 inside the window.  Nothing is assumed about alignment.
    const bool single = P.w < 2; // wave-uniform
    const int xo = single ? 0 : min(xa, P.w - 2);
    const uint32_t wo = (uint32_t)xo; // 32-bit lane offset
    const uint32_t s0 = (uint32_t)(xa - xo) * 8u, s1 = (uint32_t)(xb2 - xo) * 8u;
    // the three plane bases, once per wave on the scalar side: U and V lie uv_off and 2 * uv_off behind Y, all with the same step
    const gptr_u8 ybase = (gptr_u8)P.data;
    const gptr_u8 ubase = pin_uniform(ybase + (size_t)(uint32_t)P.uv_off), vbase = pin_uniform(ubase + (size_t)(uint32_t)P.uv_off);
    const size_t step = (size_t)P.step;

    uint32_t wy[RPW][2], wu[RPW][2], wv[RPW][2]; // the windows of source rows y1 / y2 in the three planes: six loads per output pixel
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
        const size_t o1 = (size_t)r1 * step, o2 = (size_t)r2 * step; // wave-uniform row offsets, shared by the planes
        const gptr_u8 ya = pin_uniform(ybase + o1), yb = pin_uniform(ybase + o2);
        const gptr_u8 ua = pin_uniform(ubase + o1), ub = pin_uniform(ubase + o2);
        const gptr_u8 va = pin_uniform(vbase + o1), vb = pin_uniform(vbase + o2);
        if (single) { // wave-uniform
            wy[j][0] = *(ya + wo); wy[j][1] = *(yb + wo);
            wu[j][0] = *(ua + wo); wu[j][1] = *(ub + wo);
            wv[j][0] = *(va + wo); wv[j][1] = *(vb + wo);
        } else {
            wy[j][0] = *(gptr_tap2)(ya + wo); wy[j][1] = *(gptr_tap2)(yb + wo);
            wu[j][0] = *(gptr_tap2)(ua + wo); wu[j][1] = *(gptr_tap2)(ub + wo);
            wv[j][0] = *(gptr_tap2)(va + wo); wv[j][1] = *(gptr_tap2)(vb + wo);
        }
    }

#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const int y = row0 + j;
        if (y >= dst_h) break; // wave-uniform
        float fy[4], fu[4], fv[4]; // taps 00, 10, 01, 11
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            fy[2 * r] = (float)((wy[j][r] >> s0) & 0xffu); fy[2 * r + 1] = (float)((wy[j][r] >> s1) & 0xffu);
            fu[2 * r] = (float)((wu[j][r] >> s0) & 0xffu); fu[2 * r + 1] = (float)((wu[j][r] >> s1) & 0xffu);
            fv[2 * r] = (float)((wv[j][r] >> s0) & 0xffu); fv[2 * r + 1] = (float)((wv[j][r] >> s1) & 0xffu);
        }

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
hipError_t y444_launch_bf16(int prog, const ChainArgs& c, const PlaneParams* ip, int ni, const YuvFamGeom& g, const YuvFamMany& s, bool win);
struct Y444Family : YuvFamDefaults {
    using Geom = YuvFamGeom;
    template <int NPL, class Prog, typename OT, int RPW, int CN, bool WIN> static const void* kernel() {
        return (const void*)&k_yuv444_resize<NPL, Prog, OT, RPW, CN, WIN>;
    }
    static bool eligible(const ReadArgs& r) { return r.kind == CVGS_READ_NV12_RESIZE_LINEAR && r.yuv_layout == CVGS_YUV_I444; }
    CVGS_YUV_FAMILY_NAMES("k_yuv444_resize")
    static hipError_t launch_bf16(int prog, const ChainArgs& c, const PlaneParams* ip, int ni, const YuvFamGeom& g, const YuvFamMany& s, bool win) {
        return y444_launch_bf16(prog, c, ip, ni, g, s, win);
    }
};

// bf16 (CV_16BF) planar tensors: the fp16 instantiations' twins with OT = __bf16, compiled in k_yuv444_bf16.hip (this file included with
// CVGS_Y444_BF16_TU, so the bf16 kernels build in parallel with the others).
#ifdef CVGS_Y444_BF16_TU
hipError_t y444_launch_bf16(int prog, const ChainArgs& c, const PlaneParams* ip, int ni, const YuvFamGeom& g, const YuvFamMany& s, bool win) {
    return launch_yuv_fam_bf16<Y444Family>(prog, c, ip, ni, g, s, win);
}
#else
// 1 launched / 0 not eligible / < 0 error.  Rows of one pixel take the 1-byte window, so any plane width is served.
int launch_yuv444(const ChainArgs& c_in, const PlaneParams* inline_planes, int n_inline, LaunchCtx& ctx, bool dry_run, LaunchInfo* info) {
    return launch_yuv_family<Y444Family>(c_in, inline_planes, n_inline, ctx, dry_run, info);
}
#endif // CVGS_Y444_BF16_TU

} // namespace cvgs
