// k_head.hip -- a detector's raw head -> the candidates cvgs_boxes_select reads (cvgs_head_decode, include/cvgs_hip_ext.h: THE CONTRACT).
// Two launches per call, up to CVGS_HEAD_MAX_FRAMES frames each, the frames' descriptors in the kernel arguments (1.5 KB); both have the
// grid (ceil(max candidates / 256), frame) and 256 work-items, and workgroup b of a frame owns the candidates [256 b, 256 b + 256).
//   k_head_score    steps 1-4 for every candidate (the host's own text, cvgs_geometry.h); stores the dense score and the code
//                   class | member << 16 at scratch, and the tile's member count (a ballot per wave, the four wave totals through LDS).  Two
//                   forms per element type, chosen on the host by stride (HeadFrame::group), dispatched on a workgroup-uniform switch:
//                     column (group == 0)  lane = candidate, walking the classes eight loads at a time: with cand_stride == 1 ([A, N]) a
//                                          wave's load of one class is one contiguous span.  Serves every stride pair.
//                     row (attr_stride == 1)  a group of G = 4 .. 64 lanes per candidate reads G consecutive attributes, so a wave's load is
//                                          64 / G spans of G elements (one span when rows are dense); each lane walks its classes gl, gl + G,
//                                          .. in order (the sequential form) and the group combines the partial results by a butterfly under
//                                          head_best_wins (the parallel form of step 2).  Four candidates per group are in flight at a time.
//                                          The results pass through LDS to lane = candidate for the count.
//   k_head_compact  every workgroup sums the member counts of the tiles in front of it and of all tiles (one count per work-item, a wave
//                   reduction, the wave totals through LDS), packs its members to base + position (ballot), reads the four coordinates of
//                   members only, and writes the tail elements of its own range that lie at or beyond the total; workgroup 0 stores count_out.
//                   Positions below the total belong to exactly one member, positions at or beyond it to exactly one tile.
// Wave64.  No atomic, no workgroup waits for another, nothing depends on the order in which workgroups run.  Every load of the head has a
// candidate index < n and an attribute the host validated; every scratch / output index is < n (tile counts: < 256); every LDS index < 256.
#include <hip/hip_runtime.h>

#include "cvgs_geometry.h"

namespace cvgs {

static constexpr int kHeadWaves = kHeadTile / 64;

struct HeadArgs {
    HeadFrame f[CVGS_HEAD_MAX_FRAMES];
};

// step 1: element `idx` of the head, widened
template <int E>
__device__ inline float head_at(const void* head, size_t idx) {
    if (E == CVGS_HEAD_F32) return ((const float*)head)[idx];
    const uint16_t h = ((const uint16_t*)head)[idx];
    return E == CVGS_HEAD_F16 ? head_widen_f16(h) : head_widen_bf16(h);
}

__device__ inline int32_t* head_tile_counts(const HeadFrame& f) { return (int32_t*)f.scratch; }
__device__ inline float* head_dense_scores(const HeadFrame& f) { return (float*)(f.scratch + (size_t)kHeadMaxTiles * 4); }
__device__ inline int32_t* head_dense_codes(const HeadFrame& f) { return (int32_t*)(f.scratch + (size_t)kHeadMaxTiles * 4 + (size_t)f.n * 4); }

// column form: steps 1-4 of candidate i < n by one lane
template <int E>
__device__ inline void head_score_column(const HeadFrame& f, int i, float* score, int* code) {
    const size_t as = (size_t)f.attr_stride, at = (size_t)i * (size_t)f.cand_stride;
    const size_t cls0 = at + (size_t)f.class_attr * as;
    const int C = f.num_classes;
    float best = -INFINITY;
    int cls = 0, c = 0;
    for (; c + 8 <= C; c += 8) { // eight independent loads, then the ordered walk
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = head_at<E>(f.head, cls0 + (size_t)(c + u) * as);
#pragma unroll
        for (int u = 0; u < 8; ++u) head_best_step(v[u], c + u, &best, &cls);
    }
    for (; c < C; ++c) head_best_step(head_at<E>(f.head, cls0 + (size_t)c * as), c, &best, &cls);
    const bool has_obj = f.obj_attr >= 0;
    const float obj = has_obj ? head_at<E>(f.head, at + (size_t)f.obj_attr * as) : 0.0f;
    const size_t b0 = at + (size_t)f.box_attr * as;
    const float c0 = head_at<E>(f.head, b0), c1 = head_at<E>(f.head, b0 + as), c2 = head_at<E>(f.head, b0 + 2 * as), c3 = head_at<E>(f.head, b0 + 3 * as);
    const float s = head_score(best, has_obj, obj);
    *score = s;
    *code = cls | (head_member(s, f.score_thr, c0, c1, c2, c3) ? kHeadMemberBit : 0);
}

// row form (attr_stride == 1): the wave's 64 candidates, G lanes each, four candidates per group in flight; results to LDS slot = local index
template <int E>
__device__ inline void head_score_rows(const HeadFrame& f, int first, int tid, float* s_score, int* s_code) {
    const int lane = tid & 63, wave = tid >> 6;
    const int G = f.group, per = 64 / G, gl = lane & (G - 1), sub = lane / G;
    const int C = f.num_classes, n = f.n;
    const size_t cs = (size_t)f.cand_stride;
    const bool has_obj = f.obj_attr >= 0;
    const size_t safe = (size_t)f.class_attr; // candidate 0's first class score: always inside the head
    for (int p0 = 0; p0 < G; p0 += 4) { // 64 candidates = G passes of `per`; G is a multiple of 4
        float b[4], obj[4], co[4];
        int k[4], loc[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { // every load of the four passes is issued before the first comparison (no branch in between)
            loc[u] = wave * 64 + (p0 + u) * per + sub;
            const int i = first + loc[u];
            ok[u] = i < n;
            const size_t at = (size_t)i * cs;
            const float v = head_at<E>(f.head, ok[u] && gl < C ? at + (size_t)(f.class_attr + gl) : safe);
            co[u] = head_at<E>(f.head, ok[u] ? at + (size_t)(f.box_attr + (gl & 3)) : safe);
            obj[u] = head_at<E>(f.head, ok[u] && has_obj ? at + (size_t)f.obj_attr : safe);
            b[u] = -INFINITY;
            k[u] = 0;
            if (ok[u] && gl < C) head_best_step(v, gl, &b[u], &k[u]);
        }
        for (int c0 = G; c0 < C; c0 += G) { // the classes beyond the group's width, in order (wave-uniform trip count)
            const int c = c0 + gl;
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = head_at<E>(f.head, ok[u] && c < C ? (size_t)(first + loc[u]) * cs + (size_t)(f.class_attr + c) : safe);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (ok[u] && c < C) head_best_step(v[u], c, &b[u], &k[u]);
        }
        for (int off = G >> 1; off > 0; off >>= 1) { // butterfly inside the group: every lane ends with the group's maximum
            float ob[4];
            int ok2[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { // the four candidates' exchanges of one step are independent: issued together
                ob[u] = __shfl_xor(b[u], off);
                ok2[u] = __shfl_xor(k[u], off);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (head_best_wins(ob[u], ok2[u], b[u], k[u])) {
                    b[u] = ob[u];
                    k[u] = ok2[u];
                }
        }
        // lanes 0..3 of a group hold its four coordinates (G >= 4); every lane takes part in the exchanges, all issued together
        const int g0 = sub * G;
        float c0[4], c1[4], c2[4], c3[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            c0[u] = __shfl(co[u], g0);
            c1[u] = __shfl(co[u], g0 + 1);
            c2[u] = __shfl(co[u], g0 + 2);
            c3[u] = __shfl(co[u], g0 + 3);
        }
        if (gl == 0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float s = head_score(b[u], has_obj, obj[u]);
                const bool member = ok[u] && head_member(s, f.score_thr, c0[u], c1[u], c2[u], c3[u]);
                s_score[loc[u]] = s;
                s_code[loc[u]] = k[u] | (member ? kHeadMemberBit : 0);
            }
        }
    }
}

template <int E>
__device__ inline void head_score_tile(const HeadFrame& f, int first, int tid, float* s_score, int* s_code, float* score, int* code) {
    const int i = first + tid;
    if (f.group == 0) {
        *score = 0.0f;
        *code = 0;
        if (i < f.n) head_score_column<E>(f, i, score, code);
    } else {
        head_score_rows<E>(f, first, tid, s_score, s_code);
        __syncthreads();
        *score = s_score[tid];
        *code = s_code[tid];
    }
}

__global__ __launch_bounds__(kHeadTile) void k_head_score(const HeadArgs a) {
    const HeadFrame& f = a.f[blockIdx.y];
    const int first = (int)blockIdx.x * kHeadTile;
    if (first >= f.n) return; // (frames of one call may hold different numbers of candidates)
    __shared__ float s_score[kHeadTile];
    __shared__ int s_code[kHeadTile];
    __shared__ int s_wave[kHeadWaves];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float score = 0.0f;
    int code = 0;
    switch (f.elem) { // workgroup-uniform
    case CVGS_HEAD_F32: head_score_tile<CVGS_HEAD_F32>(f, first, tid, s_score, s_code, &score, &code); break;
    case CVGS_HEAD_F16: head_score_tile<CVGS_HEAD_F16>(f, first, tid, s_score, s_code, &score, &code); break;
    default: head_score_tile<CVGS_HEAD_BF16>(f, first, tid, s_score, s_code, &score, &code); break;
    }
    const int i = first + tid;
    const bool member = i < f.n && (code & kHeadMemberBit) != 0;
    if (i < f.n) {
        head_dense_scores(f)[i] = score;
        head_dense_codes(f)[i] = code;
    }
    const unsigned long long ball = __ballot(member);
    if (lane == 0) s_wave[wave] = __popcll(ball);
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < kHeadWaves; ++w) total += s_wave[w];
        head_tile_counts(f)[blockIdx.x] = total; // blockIdx.x < ceil(n / 256) <= 256
    }
}

__device__ inline int head_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <int E>
__device__ inline void head_store_box(const HeadFrame& f, int i, int pos) {
    const size_t as = (size_t)f.attr_stride, b0 = (size_t)i * (size_t)f.cand_stride + (size_t)f.box_attr * as;
    float* o = f.boxes_out + (size_t)pos * 4;
    o[0] = head_at<E>(f.head, b0);
    o[1] = head_at<E>(f.head, b0 + as);
    o[2] = head_at<E>(f.head, b0 + 2 * as);
    o[3] = head_at<E>(f.head, b0 + 3 * as);
}

__global__ __launch_bounds__(kHeadTile) void k_head_compact(const HeadArgs a) {
    const HeadFrame& f = a.f[blockIdx.y];
    const int n = f.n, first = (int)blockIdx.x * kHeadTile;
    if (first >= n) return;
    __shared__ int s_before[kHeadWaves], s_all[kHeadWaves], s_mine[kHeadWaves];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles = (n + kHeadTile - 1) / kHeadTile; // <= 256: one count per work-item
    int cnt = tid < tiles ? head_tile_counts(f)[tid] : 0;
    cnt = cnt < 0 ? 0 : (cnt > kHeadTile ? kHeadTile : cnt); // (what the score launch wrote lies in 0..256)
    const int before = head_wave_sum(tid < (int)blockIdx.x ? cnt : 0), all = head_wave_sum(cnt);
    const int i = first + tid;
    const int code = i < n ? head_dense_codes(f)[i] : 0;
    const bool member = (code & kHeadMemberBit) != 0;
    const unsigned long long ball = __ballot(member);
    if (lane == 0) {
        s_before[wave] = before;
        s_all[wave] = all;
        s_mine[wave] = __popcll(ball);
    }
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kHeadWaves; ++w) {
        base += s_before[w] + (w < wave ? s_mine[w] : 0);
        total += s_all[w];
    }
    if (member) {
        const int pos = base + __popcll(ball & ((1ull << lane) - 1ull));
        if (pos < n) { // (always: members in front of this one number at most i)
            switch (f.elem) {
            case CVGS_HEAD_F32: head_store_box<CVGS_HEAD_F32>(f, i, pos); break;
            case CVGS_HEAD_F16: head_store_box<CVGS_HEAD_F16>(f, i, pos); break;
            default: head_store_box<CVGS_HEAD_BF16>(f, i, pos); break;
            }
            f.scores_out[pos] = head_dense_scores(f)[i];
            f.classes_out[pos] = code & (kHeadMemberBit - 1);
            if (f.index_out) f.index_out[pos] = i;
        }
    }
    if (i < n && i >= total) { // the tail of this tile's own dense range
        float* o = f.boxes_out + (size_t)i * 4;
        o[0] = 0.0f;
        o[1] = 0.0f;
        o[2] = 0.0f;
        o[3] = 0.0f;
        f.scores_out[i] = 0.0f;
        f.classes_out[i] = 0;
        if (f.index_out) f.index_out[i] = -1;
    }
    if (blockIdx.x == 0 && tid == 0) *f.count_out = total;
}

int launch_head(const HeadFrame* frames, int n, void* stream) {
    if (n < 1 || n > CVGS_HEAD_MAX_FRAMES) return (int)hipErrorInvalidValue;
    HeadArgs a;
    int most = 1;
    for (int i = 0; i < CVGS_HEAD_MAX_FRAMES; ++i) {
        a.f[i] = i < n ? frames[i] : HeadFrame{};
        if (i < n && frames[i].n > most) most = frames[i].n;
    }
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((most + kHeadTile - 1) / kHeadTile), (unsigned)n, 1);
    hipLaunchKernelGGL(k_head_score, grid, dim3(kHeadTile, 1, 1), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_head_compact, grid, dim3(kHeadTile, 1, 1), 0, s, a);
    return (int)hipGetLastError();
}

} // namespace cvgs
