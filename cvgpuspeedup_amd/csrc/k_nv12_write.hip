// k_nv12_write.hip -- NV12 / NV21 encoder surfaces written by the fused chain itself: CVGS_WRITE_NV12.
// An engine extension for pipelines that END in a video encoder (scaling ladders, re-encoded crops; the reference writes pixels and tensors
// only): the chain's CV_32FC3 R, G, B value is converted to Y'CbCr, the chroma of every 2 x 2 block is averaged, and the 8-bit surface is
// stored by the launch that read and resized the picture -- 1.5 bytes per pixel instead of the 3 a packed CV_8UC3 image costs, and no
// second pass that reads them back.
// The arithmetic is the contract written down in include/cvgs_hip.h (strict fp32, every operation rounded once, in the written order); BOTH
// kernels below run the same text for it (nv12w_convert, nv12w_chroma, nv12w_u8) and for the bilinear blend of NV12 taps (nv12w_blend), so
// the fast kernel stores the bytes the interpreted one stores.  A lane owns whole 2 x 2 blocks, so the chroma average needs no exchange
// between lanes: nothing goes through LDS.  No kernel here is compiled into any other translation unit, and no existing kernel sees the
// write kind: dispatch() (cvgs_api.cpp) hands it to launch_nv12_write before any other launcher.
#include "k_taps.hpp"

namespace cvgs {

// ---- the conversion R, G, B -> Y, U, V (floats on the 8-bit code scale) ----
struct YuvW {
    float kr, kg, kb; // luma weights
    float cu, cv;     // 0.5 / (1 - Kb), 0.5 / (1 - Kr)
    bool limited;     // Y = y * sy + 16, chroma * sc
    bool vu;          // NV21: V first
};
constexpr float kNv12wSy = 0.858824f, kNv12wSc = 0.878431f; // 219 / 255, 224 / 255

// 6-decimal literals of the derivation from the standards' luma weights (tests/test_nv12_write.py re-derives every one in float64)
__device__ __forceinline__ YuvW yuv_write_matrix(int params) {
    YuvW k;
    const int primaries = CVGS_WRITE_YUV_PRIMARIES(params);
    k.limited = CVGS_WRITE_YUV_RANGE(params) == CVGS_YUV_LIMITED;
    k.vu = CVGS_WRITE_YUV_LAYOUT(params) == CVGS_YUV_NV21;
    if (primaries == CVGS_BT601) { k.kr = 0.299f; k.kg = 0.587f; k.kb = 0.114f; k.cu = 0.564334f; k.cv = 0.713267f; }
    else if (primaries == CVGS_BT709) { k.kr = 0.2126f; k.kg = 0.7152f; k.kb = 0.0722f; k.cu = 0.538909f; k.cv = 0.635001f; }
    else { k.kr = 0.2627f; k.kg = 0.678f; k.kb = 0.0593f; k.cu = 0.531519f; k.cv = 0.67815f; }
    return k;
}

__device__ __forceinline__ void nv12w_convert(float R, float G, float B, const YuvW& k, float& Y, float& U, float& V) {
    const float y = (k.kr * R + k.kg * G) + k.kb * B;
    const float cb = (B - y) * k.cu;
    const float cr = (R - y) * k.cv;
    if (k.limited) { // wave-uniform
        Y = y * kNv12wSy + 16.0f;
        U = cb * kNv12wSc + 128.0f;
        V = cr * kNv12wSc + 128.0f;
    } else {
        Y = y;
        U = cb + 128.0f;
        V = cr + 128.0f;
    }
}
// the chroma sample of a 2 x 2 block from its four float values: top row, bottom row, then the quarter
__device__ __forceinline__ float nv12w_chroma(float c00, float c10, float c01, float c11) { return ((c00 + c10) + (c01 + c11)) * 0.25f; }
// the CVGS_OP_CAST-to-8U rule in front of a store: round to nearest even, saturate, NaN -> 0 (k_common.hpp: sat_u8_insert), byte `b` of `old`
__device__ __forceinline__ uint32_t nv12w_u8(float v, uint32_t b, uint32_t old) { return sat_u8_insert(v, b, old); }

// the bilinear blend of four converted taps (k_generic.hip's order)
__device__ __forceinline__ float nv12w_blend(float t00, float t10, float t01, float t11, float w00, float w10, float w01, float w11) {
    float acc = t00 * w00;
    acc = acc + t10 * w10;
    acc = acc + t01 * w01;
    acc = acc + t11 * w11;
    return acc;
}

typedef uint16_t nv12w_u16u __attribute__((aligned(1)));
typedef uint32_t nv12w_u32u __attribute__((aligned(1)));
typedef const __attribute__((address_space(1))) nv12w_u16u* nv12w_gld16;
typedef const __attribute__((address_space(1))) nv12w_u32u* nv12w_gld32;

// ---- the interpreted kernel: every read the generic kernel serves without a warp, interpreted program -------------------------------------
// one tap of a bilinear read (k_generic.hip: read_tap)
__device__ __forceinline__ void nv12w_read_tap(const ReadArgs& r, const PlaneParams& P, const YuvK& yk, int x, int y, Px& p) {
    if (r.kind == CVGS_READ_NV12 || r.kind == CVGS_READ_NV12_RESIZE_LINEAR) {
        nv12_px(P, x, y, yk, p);
    } else {
        load_px(P.data + (size_t)y * (size_t)P.step, r.depth, r.cn, x, p);
#pragma unroll
        for (int c = 0; c < 4; ++c) p.v[c] = tap_f(p.v[c], r.depth);
    }
}

// the value of output pixel (x, y) of plane z in front of the program: k_generic.hip's read stage, its text
__device__ __forceinline__ void nv12w_read_px(const ReadArgs& r, const PlaneParams& P, const YuvK& yk, int x, int y, bool live, int depth, Px& p) {
    p.v[0] = p.v[1] = p.v[2] = p.v[3] = 0.f;
    if (!live) { // fk::BatchRead<N,CONDITIONAL_WITH_DEFAULT>: default value, then the whole chain
#pragma unroll
        for (int k = 0; k < 4; ++k) p.v[k] = depth == CVGS_DEPTH_32S ? from_int((int)r.bg[k]) : round_to_depth(r.bg[k], depth);
    } else if (!r.is_resize) {
        if (r.kind == CVGS_READ_NV12) nv12_px(P, x, y, yk, p);
        else load_px(P.data + (size_t)y * (size_t)P.step, r.depth, r.cn, x, p);
    } else if (x >= P.x1 && x <= P.x2 && y >= P.y1 && y <= P.y2) {
        const float sx = (float)(x - P.x1) * P.fx;
        const float sy = (float)(y - P.y1) * P.fy;
        const int x1 = (int)floorf(sx), y1 = (int)floorf(sy);
        const int x2 = x1 + 1, y2 = y1 + 1;
        const int x2r = min(x2, P.w - 1), y2r = min(y2, P.h - 1);
        const int x1r = min(x1, P.w - 1), y1r = min(y1, P.h - 1); // (never binds on a plane_geometry table: no read leaves the view whatever the table says)
        Px p00, p10, p01, p11;
        nv12w_read_tap(r, P, yk, x1r, y1r, p00);
        nv12w_read_tap(r, P, yk, x2r, y1r, p10);
        nv12w_read_tap(r, P, yk, x1r, y2r, p01);
        nv12w_read_tap(r, P, yk, x2r, y2r, p11);
        const float w00 = ((float)x2 - sx) * ((float)y2 - sy);
        const float w10 = (sx - (float)x1) * ((float)y2 - sy);
        const float w01 = ((float)x2 - sx) * (sy - (float)y1);
        const float w11 = (sx - (float)x1) * (sy - (float)y1);
#pragma unroll
        for (int k = 0; k < 4; ++k) p.v[k] = nv12w_blend(p00.v[k], p10.v[k], p01.v[k], p11.v[k], w00, w10, w01, w11);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) p.v[k] = r.bg[k];
    }
}

// 64 x 4 threads, one lane = one 2 x 2 block: a wave covers 128 columns x 2 rows, its luma stores are two 128-byte rows, its chroma store one
template <int NPL>
__global__ __launch_bounds__(256) void k_nv12w(const KernArgs<NPL> a) {
    const ChainArgs& c = a.c;
    const ReadArgs& r = c.read;
    const int bx = blockIdx.x * 64 + threadIdx.x;
    const int by = blockIdx.y * 4 + threadIdx.y;
    const int z = blockIdx.z;
    if (2 * bx >= r.dst_w || 2 * by >= r.dst_h) return; // (width and height are even: a block is inside or outside as a whole)

    const bool live = z < r.used;
    PlaneParams P{};
    if (live) {
        if constexpr (NPL == 0) P = r.table[z];
        else P = a.planes[z];
    }
    const YuvK yk = yuv_matrix(r.yuv_range, r.yuv_primaries, r.yuv_layout);
    const YuvW wk = yuv_write_matrix(c.write.yuv_params);
    const int depth0 = r.is_resize || r.kind == CVGS_READ_NV12 ? CVGS_DEPTH_32F : r.depth;
    const DstPlane d = (c.write.table ? c.write.table : c.dst_inline)[z];

    float urow0 = 0.f, urow1 = 0.f, vrow0 = 0.f, vrow1 = 0.f; // U(2bx, y) + U(2bx + 1, y) of the block's two rows
#pragma unroll 1
    for (int dy = 0; dy < 2; ++dy) {
        const int y = 2 * by + dy;
        float Y[2], U[2], V[2];
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            Px p;
            int depth = depth0, cn = r.out_cn;
            nv12w_read_px(r, P, yk, 2 * bx + dx, y, live, depth, p);
            InterpProgInt::run(c.prog, p, depth, cn); // (the host has checked: the value is CV_32FC3 here)
            nv12w_convert(p.v[0], p.v[1], p.v[2], wk, Y[dx], U[dx], V[dx]);
        }
        const float us = U[0] + U[1], vs = V[0] + V[1];
        urow0 = dy == 0 ? us : urow0;
        urow1 = dy == 0 ? urow1 : us;
        vrow0 = dy == 0 ? vs : vrow0;
        vrow1 = dy == 0 ? vrow1 : vs;
        const uint32_t q = nv12w_u8(Y[1], 1, nv12w_u8(Y[0], 0, 0));
        *(nv12w_u16u*)(d.data + (size_t)y * (size_t)d.step + (size_t)(2 * bx)) = (uint16_t)q;
    }
    const float Ub = (urow0 + urow1) * 0.25f, Vb = (vrow0 + vrow1) * 0.25f; // nv12w_chroma with the row sums taken above
    const uint32_t q = wk.vu ? nv12w_u8(Ub, 1, nv12w_u8(Vb, 0, 0)) : nv12w_u8(Vb, 1, nv12w_u8(Ub, 0, 0));
    *(nv12w_u16u*)(d.data + (size_t)(uint32_t)d.pad + (size_t)by * (size_t)d.step + (size_t)(2 * bx)) = (uint16_t)q;
}

template <int NPL>
static hipError_t launch_nv12w_t(const ChainArgs& c, const PlaneParams* planes, int n, hipStream_t s) {
    KernArgs<NPL> a;
    a.c = c;
    for (int i = 0; i < (NPL > 0 ? NPL : 1); ++i) a.planes[i] = (NPL > 0 && i < n) ? planes[i] : PlaneParams{};
    const dim3 block(64, 4, 1);
    const dim3 grid((c.read.dst_w / 2 + 63) / 64, (c.read.dst_h / 2 + 3) / 4, c.read.batch);
    hipLaunchKernelGGL(k_nv12w<NPL>, grid, block, 0, s, a);
    return hipGetLastError();
}

// ---- the fast kernel: NV12 / NV21 surface -> bilinear resize -> NV12 / NV21 surface, empty program (transcoding ladders, re-encoded crops) ----
// A lane owns 4 columns x 2 rows: two whole 2 x 2 blocks, one 4-byte luma store per row and one 4-byte chroma store; a wave covers 256 columns
// x 2 rows (256-byte rows per store instruction), a workgroup of 4 waves 8 rows.  blockIdx = (column tile, row group, plane).  The taps are
// K4's (k_nv12.hip): per source row one unaligned 2-byte load holds both luma taps and one 4-byte load both chroma pairs, the windows
// clamped back into the row at its right edge.  No LDS: every chroma average is lane-private.
struct Nv12wCol {  // column geometry of one output column
    float wxa, wxb;
    uint32_t yo, uo;   // byte offsets of the luma / chroma window inside the row
    uint32_t ysh0, ysh1, ush0, ush1; // bit shifts that pick tap 0 / tap 1 out of the windows
    bool take;         // inside the plane's window
};

__device__ __forceinline__ Nv12wCol nv12w_col(const PlaneParams& P, int x, int dst_w) {
    Nv12wCol C;
    C.take = x < dst_w && x >= P.x1 && x <= P.x2;
    const int xr = C.take ? x - P.x1 : 0;
    const float sx = (float)xr * P.fx;
    const int x1 = (int)floorf(sx);
    const int x2 = x1 + 1;
    C.wxa = (float)x2 - sx;
    C.wxb = sx - (float)x1;
    const int x1r = min(x1, P.w - 1), x2r = min(x2, P.w - 1);
    const int yo = min(x1r, P.w - 2); // (NV12 views are at least 2 wide)
    C.yo = (uint32_t)yo;
    C.ysh0 = (uint32_t)(x1r - yo) * 8u;
    C.ysh1 = (uint32_t)(x2r - yo) * 8u;
    const int c1 = x1r >> 1, c2 = x2r >> 1;
    const int uo = max(min(2 * c1, P.w - 4), 0); // (a 2-wide view has one pair: the window is that pair twice, see nv12w_chroma_win)
    C.uo = (uint32_t)uo;
    C.ush0 = (uint32_t)(2 * c1 - uo) * 8u;
    C.ush1 = (uint32_t)(2 * c2 - uo) * 8u;
    return C;
}
// two chroma pairs from byte `off` of a chroma row; a view narrower than the window (2 columns) holds one pair, which is read alone
__device__ __forceinline__ uint32_t nv12w_chroma_win(gptr_u8 row, uint32_t off, bool wide) {
    if (wide) return *(nv12w_gld32)(row + off); // wave-uniform
    const uint32_t pr = *(nv12w_gld16)(row + off);
    return pr | (pr << 16);
}

template <int NPL>
__global__ __launch_bounds__(256) void k_nv12w_resize(const KernArgs<NPL> a) {
    const ChainArgs& c = a.c;
    const ReadArgs& r = c.read;
    const int z = (int)blockIdx.z;
    const int dst_w = r.dst_w, dst_h = r.dst_h;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const int x0 = ((int)blockIdx.x * 64 + lane) * 4;
    const int y0 = ((int)blockIdx.y * 4 + wave) * 2;
    if (y0 >= dst_h || x0 >= dst_w) return; // (even extents: x0 + 1 and y0 + 1 are inside too)

    const bool live = z < r.used; // wave-uniform
    PlaneParams P{};
    if (live) {
        if constexpr (NPL == 0) P = r.table[z];
        else P = a.planes[z];
    }
    const YuvK yk = yuv_matrix(r.yuv_range, r.yuv_primaries, CVGS_YUV_NV12);
    const bool vu_in = r.yuv_layout == CVGS_YUV_NV21;
    const YuvW wk = yuv_write_matrix(c.write.yuv_params);
    const DstPlane d = (c.write.table ? c.write.table : c.dst_inline)[z];
    const bool wide = P.w >= 4;
    const gptr_u8 base = (gptr_u8)P.data;
    const size_t step = (size_t)P.step;
    const gptr_u8 uvp = base + (size_t)(uint32_t)P.uv_off;

    Nv12wCol C[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) C[i] = nv12w_col(P, x0 + i, dst_w);

    float Yv[2][4], Uv[2][4], Vv[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        // row geometry (wave-uniform)
        const int y = y0 + j;
        const bool in_y = live && y >= P.y1 && y <= P.y2;
        const int yr = in_y ? y - P.y1 : 0;
        const float sy = (float)yr * P.fy;
        const int y1 = (int)floorf(sy);
        const int y2 = y1 + 1;
        const float wya = (float)y2 - sy, wyb = sy - (float)y1;
        const int r1 = __builtin_amdgcn_readfirstlane(min(y1, P.h - 1)), r2 = __builtin_amdgcn_readfirstlane(min(y2, P.h - 1));
        const gptr_u8 ya = base + (size_t)r1 * step, yb = base + (size_t)r2 * step;
        const gptr_u8 ua = uvp + (size_t)(r1 >> 1) * step, ub = uvp + (size_t)(r2 >> 1) * step;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float R = r.bg[0], G = r.bg[1], B = r.bg[2]; // outside the window / a default-value plane: the background (the program is empty)
            if (in_y && C[i].take) {
                const uint32_t la = *(nv12w_gld16)(ya + C[i].yo), lb = *(nv12w_gld16)(yb + C[i].yo);
                uint32_t ca = nv12w_chroma_win(ua, C[i].uo, wide), cb = nv12w_chroma_win(ub, C[i].uo, wide);
                if (vu_in) { // NV21: swap the bytes of every pair once, then everything below is NV12
                    ca = ((ca & 0x00ff00ffu) << 8) | ((ca >> 8) & 0x00ff00ffu);
                    cb = ((cb & 0x00ff00ffu) << 8) | ((cb >> 8) & 0x00ff00ffu);
                }
                const uint32_t pa0 = ca >> C[i].ush0, pa1 = ca >> C[i].ush1, pb0 = cb >> C[i].ush0, pb1 = cb >> C[i].ush1;
                Px t00, t10, t01, t11;
                yuv_to_rgb((float)((la >> C[i].ysh0) & 0xffu), (float)(pa0 & 0xffu), (float)((pa0 >> 8) & 0xffu), yk, t00);
                yuv_to_rgb((float)((la >> C[i].ysh1) & 0xffu), (float)(pa1 & 0xffu), (float)((pa1 >> 8) & 0xffu), yk, t10);
                yuv_to_rgb((float)((lb >> C[i].ysh0) & 0xffu), (float)(pb0 & 0xffu), (float)((pb0 >> 8) & 0xffu), yk, t01);
                yuv_to_rgb((float)((lb >> C[i].ysh1) & 0xffu), (float)(pb1 & 0xffu), (float)((pb1 >> 8) & 0xffu), yk, t11);
                const float w00 = C[i].wxa * wya, w10 = C[i].wxb * wya, w01 = C[i].wxa * wyb, w11 = C[i].wxb * wyb;
                R = nv12w_blend(t00.v[0], t10.v[0], t01.v[0], t11.v[0], w00, w10, w01, w11);
                G = nv12w_blend(t00.v[1], t10.v[1], t01.v[1], t11.v[1], w00, w10, w01, w11);
                B = nv12w_blend(t00.v[2], t10.v[2], t01.v[2], t11.v[2], w00, w10, w01, w11);
            }
            nv12w_convert(R, G, B, wk, Yv[j][i], Uv[j][i], Vv[j][i]);
        }
    }

    // the stores: 4 bytes per row and lane, 2 where the plane's last block pair is a single block (width % 4 == 2)
    const bool four = x0 + 4 <= dst_w;
    uint32_t cq = 0;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const float Ub = nv12w_chroma(Uv[0][2 * b], Uv[0][2 * b + 1], Uv[1][2 * b], Uv[1][2 * b + 1]);
        const float Vb = nv12w_chroma(Vv[0][2 * b], Vv[0][2 * b + 1], Vv[1][2 * b], Vv[1][2 * b + 1]);
        cq = nv12w_u8(wk.vu ? Vb : Ub, 2 * b, cq);
        cq = nv12w_u8(wk.vu ? Ub : Vb, 2 * b + 1, cq);
    }
    uint8_t* const crow = d.data + (size_t)(uint32_t)d.pad + (size_t)(y0 >> 1) * (size_t)d.step + (size_t)x0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t q = nv12w_u8(Yv[j][3], 3, nv12w_u8(Yv[j][2], 2, nv12w_u8(Yv[j][1], 1, nv12w_u8(Yv[j][0], 0, 0))));
        uint8_t* const yrow = d.data + (size_t)(y0 + j) * (size_t)d.step + (size_t)x0;
        if (four) *(nv12w_u32u*)yrow = q;
        else *(nv12w_u16u*)yrow = (uint16_t)q;
    }
    if (four) *(nv12w_u32u*)crow = cq;
    else *(nv12w_u16u*)crow = (uint16_t)cq;
}

template <int NPL>
static hipError_t launch_nv12w_resize_t(const ChainArgs& c, const PlaneParams* planes, int n, hipStream_t s) {
    KernArgs<NPL> a;
    a.c = c;
    for (int i = 0; i < (NPL > 0 ? NPL : 1); ++i) a.planes[i] = (NPL > 0 && i < n) ? planes[i] : PlaneParams{};
    const dim3 grid((c.read.dst_w + 255) / 256, (c.read.dst_h / 2 + 3) / 4, c.read.batch);
    hipLaunchKernelGGL(k_nv12w_resize<NPL>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

static bool nv12w_fast_eligible(const ChainArgs& c) {
    const ReadArgs& r = c.read;
    return r.kind == CVGS_READ_NV12_RESIZE_LINEAR && (r.yuv_layout == CVGS_YUV_NV12 || r.yuv_layout == CVGS_YUV_NV21) && r.depth == CVGS_DEPTH_8U &&
           r.yuv_alpha == 0 && c.prog.n == 0;
}

int launch_nv12_write(const ChainArgs& c, const PlaneParams* inline_planes, int n_inline, uint32_t chain_flags, void* stream, bool dry_run, LaunchInfo* info) {
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (!c.read.table && n_inline > CVGS_KERNARG_PLANES) return -1; // (the caller stages larger batches into a table)
    if ((c.read.dst_w | c.read.dst_h) & 1) return -1;                // (the lowering refuses odd surfaces)
    const bool fast = !(chain_flags & CVGS_CHAIN_FORCE_GENERIC) && nv12w_fast_eligible(c);
    if (info) info->kernel = fast ? "nv12w_nv12_resize" : "nv12w_interp";
    if (dry_run) return 0;
    if (fast) {
        if (c.read.table) e = launch_nv12w_resize_t<0>(c, nullptr, 0, s);
        else if (n_inline <= 8) e = launch_nv12w_resize_t<8>(c, inline_planes, n_inline, s);
        else e = launch_nv12w_resize_t<CVGS_KERNARG_PLANES>(c, inline_planes, n_inline, s);
    } else {
        if (c.read.table) e = launch_nv12w_t<0>(c, nullptr, 0, s);
        else if (n_inline <= 8) e = launch_nv12w_t<8>(c, inline_planes, n_inline, s);
        else e = launch_nv12w_t<CVGS_KERNARG_PLANES>(c, inline_planes, n_inline, s);
    }
    return e == hipSuccess ? 0 : -(int)e - 1000;
}

} // namespace cvgs
