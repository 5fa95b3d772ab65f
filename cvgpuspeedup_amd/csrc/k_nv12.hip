// k_nv12.hip -- K4: NV12 read-back fused into the bilinear resize: each of the 4 taps is fetched from the luma
// plane and the interleaved chroma plane, converted YCbCr -> RGB(A) in float, THEN interpolated, then pushed
// through the pointwise program and written (planar fp32 tensor, or packed pixels).  Replaces
//   fk::Resize<INTER_LINEAR>::build(fk::fuse(Read<ReadYUV<NV12>>, Unary<ConvertYUVToRGB<NV12,range,primaries,alpha,floatN>>), size)
// (reference tests/resize/test_fused_resize.cu:141-147).
//
// Mapping: lane = output column, wave = one output row (blockIdx.y = row group, blockIdx.z = plane).  Per output
// pixel and source row: ONE unaligned 2-byte load brings both luma taps, ONE unaligned 4-byte load both chroma
// pairs (4 loads per pixel instead of 12 byte loads); windows are clamped into the row.  Planar stores are
// full-wave 256-byte rows, non-temporal.
#include <cstdio>

#include "k_yuv_family.hpp"

namespace cvgs {

typedef uint16_t u16_unaligned __attribute__((aligned(1)));
typedef uint32_t u32_unaligned __attribute__((aligned(1)));
typedef const __attribute__((address_space(1))) u16_unaligned* gptr_u16;
typedef const __attribute__((address_space(1))) u32_unaligned* gptr_u32;
typedef uint64_t u64_unaligned __attribute__((aligned(1)));
typedef const __attribute__((address_space(1))) u64_unaligned* gptr_u64;

struct N12Geom : YuvFamGeom {}; // (a type of its own: part of the kernels' signature)

// The prologue, the store stage, the window machinery, the blend and the LDS epilogue below stand a second and a third time in
// k_yuv422.hip and k_yuv444.hip, and a fix to one belongs in all three: writing them once changes the machine code.
// RPW output rows per wave (the launcher uses 1 or 4, see launch_yuv_fam_rows); CN output channels (3, or 4 with alpha).  One tap's conversion:
// k4_tap (k_common.hpp), shared with the descriptor queue's NV12 worker (k_queue.hip).
// S16: P010 -- the same geometry with 16-bit samples (10-bit code = sample >> 6): the two luma taps are ONE 4-byte load, the
// two chroma pairs ONE 8-byte load.
// WIN: the target may hold an aspect-ratio window (letterboxed detector inputs: PRESERVE_AR*) and default-value planes
// (usedPlanes < BATCH) -- K1's machinery: the background value runs through the program once, pixels outside the window take it.
// A separate instantiation: K4 is bound by its VALU work per row, and the window's selects cost the stretch-only launches 4-8 %
// when they are compiled in (tools/k4_ar_ab.sh: cfg #3 8.6 -> 9.0 us, 50 crops 4.92 -> 5.32 us).
// PL: planar chroma (I420 / YV12, software decoders' yuv420p): two (W/2) x (H/2) planes with rows of step/2 bytes behind the luma
// plane.  The two chroma taps of a plane are ONE unaligned 2-byte load per source row (6 loads per pixel instead of 4); the
// (U,V) pairs are then assembled in registers and everything downstream is the NV12 arithmetic, bit for bit.
template <int NPL, class Prog, typename OT = float, int RPW = 1, int CN = 3, bool S16 = false, bool WIN = false, bool PL = false>
__global__ __launch_bounds__(64 * kYuvFamWaves) void k4_nv12_resize(const YuvFamArgs<NPL> a, const N12Geom g) {
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
    const bool vu = c.read.yuv_layout == CVGS_YUV_NV21 || c.read.yuv_layout == CVGS_YUV_YV12; // wave-uniform: V comes first
    const int64_t img_stride = g.img_stride, ch_stride = g.ch_stride;
    typedef float f32x4s __attribute__((ext_vector_type(4)));
    const f32x4s op0 = *(const f32x4s*)c.prog.operand[0], op1 = *(const f32x4s*)c.prog.operand[1],
                 op2 = *(const f32x4s*)c.prog.operand[2], op3 = *(const f32x4s*)c.prog.operand[3];
    // one batch of scalar loads, one wait (see k_k1.hip)
    if constexpr (WIN) asm volatile("" ::"s"(used), "s"(P.x1), "s"(P.y1), "s"(P.x2), "s"(P.y2));
    asm volatile("" ::"s"(dst_w), "s"(dst_h), "s"(W), "s"(CN), "s"(P.w), "s"(P.h), "s"(P.step), "s"(P.fx), "s"(P.fy), "s"(P.data), "s"(P.uv_off),
                 "s"(yuv_range), "s"(yuv_prim), "s"(packed), "s"(img_stride), "s"(ch_stride), "s"(out_base), "s"(op0), "s"(op1),
                 "s"(op2), "s"(op3));
    // (behind the scalar loads: a store in front of them would make the compiler fetch the descriptors with vector loads)
    if constexpr (NPL == 0) {
        if (g.done_word && (blockIdx.x | blockIdx.y | blockIdx.z) == 0 && threadIdx.x == 0)
            __hip_atomic_store(g.done_word, g.done_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const YuvK yk = yuv_matrix(yuv_range, yuv_prim, S16 ? CVGS_YUV_P010 : CVGS_YUV_NV12);

    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const int x = col_tile * 64 + lane;
    const int row0 = (row_group * kYuvFamWaves + wave) * RPW;
    if (row0 >= dst_h || x >= dst_w) return;

    // one output pixel of row y (wave-uniform row pointers; planar: non-temporal rows, packed: the generic write stage)
    auto store_px = [&](const Px& p, int depth, int cn, int y) {
    if constexpr (std::is_same_v<OT, uint8_t>) {
        // packed u8 images (thumbnails, display surfaces): the chain's trailing SaturateCast is the store's conversion.  C3: a full
        // 64-column tile leaves as 48 dword stores (k_taps.hpp: store_u8c3_tile), ragged tiles as 3 bytes per lane; C4 (the
        // reference's own chain, tests/resize/test_fused_resize.cu:141-147: uchar4): one dword per lane, 256 bytes per wave
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
        // OT = _Float16: the chain's trailing CAST(CV_16F) is this round-to-nearest-even conversion
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
    // does the source cover the whole target?  (always, except aspect-ratio padding -- letterboxed detector inputs -- and planes
    // >= usedPlanes; wave-uniform.)  Otherwise the background value runs through the program once and replaces the pixels outside.
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

    // column geometry (once per lane, reused for every row)
    const float sx = (float)xr * P.fx;
    const int x1 = (int)floorf(sx);
    const int x2 = x1 + 1;
    const float wxa = (float)x2 - sx, wxb = sx - (float)x1;
    const bool edge = x2 > P.w - 1;
    const int x2r = edge ? x1 : x2;
    constexpr int kSB = S16 ? 2 : 1; // bytes per sample
    const uint32_t yo = (uint32_t)min(x1, P.w - 2) * kSB;
    const int ysh = (x1 * kSB - (int)yo) * 8;
    const int c1 = x1 >> 1, c2 = x2r >> 1;
    // interleaved: a window of two pairs, clamped into the row; planar: a window of two samples of one chroma plane
    const uint32_t uo = PL ? (uint32_t)min(c1, ((P.w - 1) >> 1) - 1) : (uint32_t)min(2 * c1, P.w - 4) * kSB;
    const int ush = PL ? (c1 - (int)uo) * 8 : (2 * c1 * kSB - (int)uo) * 8;
    const bool same_pair = c2 == c1;
    // 8-bit interleaved chroma: v_perm_b32 selectors that pick the pixel's four tap samples {a0, a1, b0, b1} (row a / b, tap 0 / 1) out of its two
    // 2-byte luma windows / its two 4-byte chroma windows -- what was a shift, a mask and a select per sample: the luma window clamped back at
    // the right edge (then both taps are its second byte), the chroma window clamped back at the last pair, taps sharing a chroma pair, NV21's
    // byte order (k_nv12_x2.hip and the queue's k4q_rows pick their samples the same way)
    [[maybe_unused]] uint32_t sel_y = 0, sel_u = 0, sel_v = 0;
    if constexpr (!S16 && !PL) {
        sel_y = edge ? 0x05050101u : 0x05040100u;
        const uint32_t pr0 = 2 * c1 != (int)uo ? 2u : 0u; // byte of tap 0's pair inside the chroma window
        const uint32_t pr1 = same_pair ? pr0 : 2u;        // ... of tap 1's
        const uint32_t sel_c = pr0 | (pr1 << 8) | ((4u + pr0) << 16) | ((4u + pr1) << 24);
        const bool vu_first = c.read.yuv_layout == CVGS_YUV_NV21;
        sel_u = sel_c + (vu_first ? 0x01010101u : 0u);
        sel_v = sel_c + (vu_first ? 0u : 0x01010101u);
    }
    const gptr_u8 base = (gptr_u8)P.data;
    const size_t step = (size_t)P.step;
    const gptr_u8 uvp = base + (size_t)P.uv_off; // crops of a surface carry their own luma -> chroma offset
    const size_t cstep = PL ? step >> 1 : step;  // bytes per chroma row
    const size_t plane2 = (size_t)(P.h >> 1) * cstep; // planar: the second chroma plane follows the first

    using ChromaWin = std::conditional_t<S16, uint64_t, uint32_t>; // two (U,V) pairs
    uint32_t vya[RPW], vyb[RPW];
    ChromaWin vua[RPW], vub[RPW];
    uint32_t vva[RPW], vvb[RPW]; // planar chroma: the windows of the second plane
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
        const int y2r = min(y2, P.h - 1);
        wya[j] = (float)y2 - sy;
        wyb[j] = sy - (float)y1;
        const int r1 = __builtin_amdgcn_readfirstlane(y1), r2 = __builtin_amdgcn_readfirstlane(y2r);
        const gptr_u8 ya = pin_uniform(base + (size_t)r1 * step);
        const gptr_u8 yb = pin_uniform(base + (size_t)r2 * step);
        const gptr_u8 ua = pin_uniform(uvp + (size_t)(r1 >> 1) * cstep);
        if constexpr (PL) {
            const gptr_u8 ub = pin_uniform(uvp + (size_t)(r2 >> 1) * cstep);
            vya[j] = *(gptr_u16)(ya + yo);
            vyb[j] = *(gptr_u16)(yb + yo);
            vua[j] = *(gptr_u16)(ua + uo);
            vub[j] = *(gptr_u16)(ub + uo);
            vva[j] = *(gptr_u16)(pin_uniform(ua + plane2) + uo);
            vvb[j] = *(gptr_u16)(pin_uniform(ub + plane2) + uo);
            continue;
        }
        if constexpr (S16) {
            vya[j] = *(gptr_u32)(ya + yo);
            vyb[j] = *(gptr_u32)(yb + yo);
            vua[j] = *(gptr_u64)(ua + uo);
        } else {
            vya[j] = *(gptr_u16)(ya + yo);
            vyb[j] = *(gptr_u16)(yb + yo);
            vua[j] = *(gptr_u32)(ua + uo);
        }
        // Every other row pair shares ONE chroma row; skipping its second load behind a wave-uniform branch was measured
        // and lost (cfg #3 9.15 vs 8.02 us, 50 NV12 crops 5.04 vs 4.52 us): the redundant load hits L1,
        // the branch delays the loads behind it.
        const gptr_u8 ub = pin_uniform(uvp + (size_t)(r2 >> 1) * step);
        if constexpr (S16) vub[j] = *(gptr_u64)(ub + uo);
        else vub[j] = *(gptr_u32)(ub + uo);
    }

#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const int y = row0 + j;
        if (y >= dst_h) break; // wave-uniform
        float fy[4], fu[4], fv[4]; // taps 00, 10, 01, 11
        if constexpr (S16) {
            const uint32_t ya0 = (vya[j] >> ysh) & 0xffffu, ya1 = edge ? ya0 : vya[j] >> 16;
            const uint32_t yb0 = (vyb[j] >> ysh) & 0xffffu, yb1 = edge ? yb0 : vyb[j] >> 16;
            const uint32_t pa0 = (uint32_t)(vua[j] >> ush), pa1 = same_pair ? pa0 : (uint32_t)(vua[j] >> 32);
            const uint32_t pb0 = (uint32_t)(vub[j] >> ush), pb1 = same_pair ? pb0 : (uint32_t)(vub[j] >> 32);
            fy[0] = (float)(ya0 >> 6); fy[1] = (float)(ya1 >> 6); fy[2] = (float)(yb0 >> 6); fy[3] = (float)(yb1 >> 6);
            fu[0] = (float)((pa0 & 0xffffu) >> 6); fu[1] = (float)((pa1 & 0xffffu) >> 6);
            fu[2] = (float)((pb0 & 0xffffu) >> 6); fu[3] = (float)((pb1 & 0xffffu) >> 6);
            fv[0] = (float)(pa0 >> 22); fv[1] = (float)(pa1 >> 22); fv[2] = (float)(pb0 >> 22); fv[3] = (float)(pb1 >> 22);
        } else if constexpr (!PL) {
            const uint32_t ly = __builtin_amdgcn_perm(vyb[j], vya[j], sel_y);
            const uint32_t lu = __builtin_amdgcn_perm((uint32_t)vub[j], (uint32_t)vua[j], sel_u), lv = __builtin_amdgcn_perm((uint32_t)vub[j], (uint32_t)vua[j], sel_v);
            fy[0] = (float)(ly & 0xffu); fy[1] = (float)((ly >> 8) & 0xffu); fy[2] = (float)((ly >> 16) & 0xffu); fy[3] = (float)(ly >> 24);
            fu[0] = (float)(lu & 0xffu); fu[1] = (float)((lu >> 8) & 0xffu); fu[2] = (float)((lu >> 16) & 0xffu); fu[3] = (float)(lu >> 24);
            fv[0] = (float)(lv & 0xffu); fv[1] = (float)((lv >> 8) & 0xffu); fv[2] = (float)((lv >> 16) & 0xffu); fv[3] = (float)(lv >> 24);
        } else {
            const uint32_t ya0 = (vya[j] >> ysh) & 0xffu, ya1 = edge ? ya0 : (vya[j] >> 8) & 0xffu;
            const uint32_t yb0 = (vyb[j] >> ysh) & 0xffu, yb1 = edge ? yb0 : (vyb[j] >> 8) & 0xffu;
            uint32_t ca = vua[j], cb = vub[j];
            if constexpr (PL) { // spread the two samples of each plane into the (first, second) pairs of an interleaved window
                const uint32_t fa = (uint32_t)vua[j] >> ush, fb = (uint32_t)vub[j] >> ush, sa = vva[j] >> ush, sb = vvb[j] >> ush;
                ca = (fa & 0xffu) | ((sa & 0xffu) << 8) | ((fa & 0xff00u) << 8) | ((sa & 0xff00u) << 16);
                cb = (fb & 0xffu) | ((sb & 0xffu) << 8) | ((fb & 0xff00u) << 8) | ((sb & 0xff00u) << 16);
            }
            if (vu) { // NV21: swap the bytes of every pair once, then everything below is NV12
                ca = ((ca & 0x00ff00ffu) << 8) | ((ca >> 8) & 0x00ff00ffu);
                cb = ((cb & 0x00ff00ffu) << 8) | ((cb >> 8) & 0x00ff00ffu);
            }
            const int psh = PL ? 0 : ush; // planar: the windows were shifted before the spread
            const uint32_t pa0 = (ca >> psh) & 0xffffu, pa1 = same_pair ? pa0 : (ca >> 16) & 0xffffu;
            const uint32_t pb0 = (cb >> psh) & 0xffffu, pb1 = same_pair ? pb0 : (cb >> 16) & 0xffffu;
            fy[0] = (float)ya0; fy[1] = (float)ya1; fy[2] = (float)yb0; fy[3] = (float)yb1;
            fu[0] = (float)(pa0 & 0xffu); fu[1] = (float)(pa1 & 0xffu); fu[2] = (float)(pb0 & 0xffu); fu[3] = (float)(pb1 & 0xffu);
            fv[0] = (float)(pa0 >> 8); fv[1] = (float)(pa1 >> 8); fv[2] = (float)(pb0 >> 8); fv[3] = (float)(pb1 >> 8);
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
            // l / 16 -- 16 bytes per lane and store instruction, three stores for the wave's four rows instead of twelve (the descriptor
            // queue's row workers publish their rows this way, k_queue.hip: q_lds_put / q_lds_get; fused launches of 4:2:0 crops are bound by
            // the number of memory instructions: four tap loads per row and lane)
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

// the family's traits for the shared launcher (k_yuv_family.hpp): one family per kernel variant -- interleaved 8-bit chroma (NV12 / NV21),
// S16 (P010), PL (I420 / YV12) --, picked from the layout by k4_pick
hipError_t k4_launch_bf16(int prog, const ChainArgs& c, const PlaneParams* ip, int ni, const YuvFamGeom& g, const YuvFamMany& s, bool win);
struct K4FamilyBase : YuvFamDefaults {
    using Geom = N12Geom;
    static bool eligible(const ReadArgs& r) { return r.kind == CVGS_READ_NV12_RESIZE_LINEAR; } // (launch_nv12 is handed the 4:2:0 layouts only)
    CVGS_YUV_FAMILY_NAMES("k4_nv12_resize")
    static hipError_t launch_bf16(int prog, const ChainArgs& c, const PlaneParams* ip, int ni, const YuvFamGeom& g, const YuvFamMany& s, bool win) {
        return k4_launch_bf16(prog, c, ip, ni, g, s, win);
    }
    // whole surfaces stretched into large targets (cfg #3: 6K -> 1280 x 720): two output pixels per lane (k_nv12_x2.hip) once the
    // launch is paced by instruction issue rather than by its latency; CVGS_CHAIN_NO_THREAD_FUSION keeps the one-pixel kernel
    static int frame_kernel(const ChainArgs& c, const PlaneParams* planes, int n, bool prog_swap, bool f16, const LaunchCtx& ctx, uint32_t chain_flags,
                            bool dry_run, LaunchInfo* info) {
        const ReadArgs& r = c.read;
        if (f16 || ctx.segs || r.out_cn != 3 || (chain_flags & CVGS_CHAIN_NO_THREAD_FUSION)) return 0;
        const char* x2_env = getenv("CVGS_K4_X2"); // tuning / test hook: 0 = never, 1 = whenever eligible
        const int64_t wave_rows = (int64_t)r.batch * r.dst_h * ((r.dst_w + 63) / 64);
        if (!(x2_env ? x2_env[0] == '1' : wave_rows >= kK4X2MinWaveRows)) return 0;
        int rows = 0;
        const int rc = launch_nv12_x2(c, planes, n, prog_swap, ctx.stream, dry_run, &rows);
        if (rc != 0 && info) {
            info->kernel = prog_swap ? "k4_nv12_x2_swap_mul_sub_div" : "k4_nv12_x2_mul_sub_div";
            if (x2_env) { // under the hook, and only then, the name says which form was taken: "@r1" / "@r2" (tests/test_k4_x2_cases.py), as k_k1.hip's does:
                // a per-thread buffer, valid until this thread's next call that asks for a name; cvgs_kernel_name copies it out before it returns
                static thread_local char hooked[96];
                snprintf(hooked, sizeof(hooked), "%s@r%d", info->kernel, rows);
                info->kernel = hooked;
            }
        }
        return rc;
    }
};
template <bool S16, bool PL> struct K4Family : K4FamilyBase {
    template <int NPL, class Prog, typename OT, int RPW, int CN, bool WIN> static const void* kernel() {
        return (const void*)&k4_nv12_resize<NPL, Prog, OT, RPW, CN, S16, WIN, PL>;
    }
    // planar chroma: one row per wave at every size, and fused chains through device tables only (no instantiations for either)
    static constexpr bool kRows4 = !PL, kManyInline = !PL;
};
template <class Fn> static auto k4_pick(int yuv_layout, Fn fn) {
    if (yuv_layout == CVGS_YUV_I420 || yuv_layout == CVGS_YUV_YV12) return fn(K4Family<false, true>{});
    if (yuv_layout == CVGS_YUV_P010) return fn(K4Family<true, false>{});
    return fn(K4Family<false, false>{});
}

// bf16 (CV_16BF) planar tensors: the fp16 instantiations' twins with OT = __bf16, compiled in k_nv12_bf16.hip (this file included with
// CVGS_K4_BF16_TU, so the bf16 kernels build in parallel with the others).
#ifdef CVGS_K4_BF16_TU
hipError_t k4_launch_bf16(int prog, const ChainArgs& c, const PlaneParams* ip, int ni, const YuvFamGeom& g, const YuvFamMany& s, bool win) {
    return k4_pick(c.read.yuv_layout, [&](auto f) { return launch_yuv_fam_bf16<decltype(f)>(prog, c, ip, ni, g, s, win); });
}
#else
// Stretch geometry on rows wide enough for the 4-byte chroma window: what the callers that cannot pick the windowed instantiations
// (fused chains, staged tables) check on their planes.
bool k4_planes_eligible(const PlaneParams* planes, int n, int dst_w, int dst_h) {
    for (int i = 0; i < n; ++i)
        if (planes[i].w < 4) return false;
    return yuv_fam_stretch(planes, n, dst_w, dst_h);
}

// The 4:2:0 layouts through the shared launcher: 1 launched / 0 not eligible / < 0 error.  min_width: over the planes that are read;
// narrower rows than the chroma window are the generic kernel's (fused chains: the caller has checked them with k4_planes_eligible).
int launch_nv12(const ChainArgs& c, const PlaneParams* inline_planes, int n_inline, int min_width, LaunchCtx& ctx, bool dry_run, LaunchInfo* info,
                uint32_t chain_flags) {
    if (!ctx.segs) {
        if (min_width < 4) return 0;
        for (int i = 0; i < n_inline && i < c.read.used; ++i)
            if (inline_planes[i].w < 4) return 0;
    }
    return k4_pick(c.read.yuv_layout, [&](auto f) { return launch_yuv_family<decltype(f)>(c, inline_planes, n_inline, ctx, dry_run, info, chain_flags); });
}
#endif // CVGS_K4_BF16_TU

} // namespace cvgs
