// k_select.hip -- detector candidates -> selected boxes on the device (cvgs_boxes_select, include/cvgs_hip_ext.h: THE CONTRACT).
// Two launches per call, up to CVGS_SELECT_MAX_FRAMES frames each, the frames' descriptors in the kernel arguments (2.2 KB):
//   k_select_rank  grid (ceil(max candidates / 256), frame), 256 work-items.  Each work-item prepares its candidate (steps 2-5: the host's
//                  own text, cvgs_geometry.h) and finds its position in the order of step 6 by COUNTING the members that precede it: the
//                  workgroup walks the live candidates in tiles of 256, prepares the tile again, packs the tile's members (score, index)
//                  into LDS in index order -- a ballot per wave, the four wave totals through LDS -- and every member work-item compares
//                  its key with the packed ones (broadcast LDS reads).  Ranks are a permutation of the members, so members of rank <
//                  pre_k store {box, score, index, class} at scratch[rank] without a sort and without an atomic; workgroup 0 stores the
//                  member count.  Nothing depends on the order in which workgroups run.
//   k_select_nms   one wave per frame.  The working list (<= 1024 entries) sits in LDS; the wave walks it in order, tests candidate i
//                  against the kept boxes 64 at a time (a ballot decides), appends it to the kept list in LDS, and at the end writes EVERY
//                  output element, tails included.  44 KB of LDS.
// Wave64.  Every store is a plain per-lane store: scratch[rank] with rank < pre_k, outputs[k] with k < max_out, count_out; every load of a
// candidate has index < live <= max_cand; every LDS index is < 1024 (pre_k, max_out <= 1024: validated on the host).
#include <hip/hip_runtime.h>

#include "cvgs_geometry.h"

namespace cvgs {

static constexpr int kRankBlock = 256;
static constexpr int kRankWaves = kRankBlock / 64;
static constexpr int kMaxPre = CVGS_SELECT_MAX_PRE_NMS;

struct SelectArgs {
    SelectFrame f[CVGS_SELECT_MAX_FRAMES];
};

// steps 2-5 for candidate i (false beyond `live`); *score = the score as read
__device__ inline bool select_load(const SelectFrame& f, int i, int live, float* box, float* score) {
    if (i >= live) return false;
    const float* q = f.boxes + (size_t)i * (size_t)f.box_stride;
    const float s = f.scores[(size_t)i * (size_t)f.score_stride];
    *score = s;
    return select_prepare(f.fmt, q[0], q[1], q[2], q[3], s, f.score_thr, f.xf, f.w, f.h, box);
}

__global__ __launch_bounds__(kRankBlock) void k_select_rank(const SelectArgs a) {
    const SelectFrame& f = a.f[blockIdx.y];
    const int first = (int)blockIdx.x * kRankBlock;
    if (first >= f.max_cand) return; // (frames of one call may hold different numbers of candidates)
    int live = f.count ? *f.count : f.max_cand;
    live = live < 0 ? 0 : (live > f.max_cand ? f.max_cand : live);
    if (first >= live && blockIdx.x != 0) return; // nothing to rank here; workgroup 0 stays for the member count

    __shared__ float s_score[kRankBlock];
    __shared__ int s_idx[kRankBlock];
    __shared__ int s_wave[kRankWaves];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = first + tid;
    float box[4] = {0.f, 0.f, 0.f, 0.f}, score = 0.f;
    const bool member = select_load(f, i, live, box, &score);

    int rank = 0, members = 0;
    for (int t0 = 0; t0 < live; t0 += kRankBlock) {
        const int j = t0 + tid;
        float jbox[4], jscore = 0.f;
        const bool jm = select_load(f, j, live, jbox, &jscore);
        const unsigned long long ball = __ballot(jm);
        if (lane == 0) s_wave[wave] = __popcll(ball);
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kRankWaves; ++w) {
            const int c = s_wave[w];
            base += w < wave ? c : 0;
            total += c;
        }
        if (jm) { // the tile's members, packed in index order
            const int pos = base + __popcll(ball & ((1ull << lane) - 1ull));
            s_score[pos] = jscore;
            s_idx[pos] = j;
        }
        __syncthreads();
        if (member)
            for (int k = 0; k < total; ++k) rank += select_precedes(s_score[k], s_idx[k], score, i) ? 1 : 0;
        members += total;
        __syncthreads();
    }

    int32_t* hdr = (int32_t*)f.scratch;
    if (blockIdx.x == 0 && tid == 0) {
        hdr[0] = members;
        hdr[1] = 0;
    }
    if (member && rank < f.pre_k) {
        float* wf = (float*)(f.scratch + 8);
        int32_t* wi = (int32_t*)(f.scratch + 8);
        const size_t k = (size_t)f.pre_k;
        wf[rank] = box[0];
        wf[k + rank] = box[1];
        wf[2 * k + rank] = box[2];
        wf[3 * k + rank] = box[3];
        wf[4 * k + rank] = score;
        wi[5 * k + rank] = i;
        wi[6 * k + rank] = f.classes ? f.classes[(size_t)i * (size_t)f.class_stride] : 0;
    }
}

__global__ __launch_bounds__(64) void k_select_nms(const SelectArgs a) {
    const SelectFrame& f = a.f[blockIdx.x];
    __shared__ float s_xa[kMaxPre], s_ya[kMaxPre], s_xb[kMaxPre], s_yb[kMaxPre]; // the working list
    __shared__ int s_cls[kMaxPre];
    __shared__ float k_xa[kMaxPre], k_ya[kMaxPre], k_xb[kMaxPre], k_yb[kMaxPre]; // the kept boxes, in the order kept
    __shared__ int k_cls[kMaxPre], k_src[kMaxPre];                               // ... their class and their place in the working list
    const int lane = (int)threadIdx.x;
    const size_t pk = (size_t)f.pre_k;
    const int32_t* hdr = (const int32_t*)f.scratch;
    const float* wf = (const float*)(f.scratch + 8);
    const int32_t* wi = (const int32_t*)(f.scratch + 8);
    int n_work = hdr[0];
    n_work = n_work < 0 ? 0 : (n_work > f.pre_k ? f.pre_k : n_work);
    for (int k = lane; k < n_work; k += 64) {
        s_xa[k] = wf[k];
        s_ya[k] = wf[pk + k];
        s_xb[k] = wf[2 * pk + k];
        s_yb[k] = wf[3 * pk + k];
        s_cls[k] = wi[6 * pk + k];
    }
    __syncthreads();

    int kept = 0; // wave-uniform: a ballot decides every step
    for (int i = 0; i < n_work && kept < f.max_out; ++i) {
        const float ixa = s_xa[i], iya = s_ya[i], ixb = s_xb[i], iyb = s_yb[i];
        const int ic = s_cls[i];
        bool sup = false;
        for (int k = lane; k < kept; k += 64)
            sup = sup || (k_cls[k] == ic && select_suppresses(k_xa[k], k_ya[k], k_xb[k], k_yb[k], ixa, iya, ixb, iyb, f.iou_thr));
        if (__ballot(sup) == 0ull) {
            if (lane == 0) {
                k_xa[kept] = ixa;
                k_ya[kept] = iya;
                k_xb[kept] = ixb;
                k_yb[kept] = iyb;
                k_cls[kept] = ic;
                k_src[kept] = i;
            }
            ++kept;
        }
        __syncthreads(); // one wave: orders the kept list's stores in front of the next step's loads
    }

    for (int k = lane; k < f.max_out; k += 64) { // every element, tails included
        const bool v = k < kept;
        float* o = f.boxes_out + (size_t)k * 4;
        o[0] = v ? k_xa[k] : 0.f;
        o[1] = v ? k_ya[k] : 0.f;
        o[2] = v ? k_xb[k] : 0.f;
        o[3] = v ? k_yb[k] : 0.f;
        const int src = v ? k_src[k] : 0;
        if (f.scores_out) f.scores_out[k] = v ? wf[4 * pk + src] : 0.f;
        if (f.index_out) f.index_out[k] = v ? wi[5 * pk + src] : -1;
    }
    if (lane == 0) *f.count_out = kept;
}

int launch_select(const SelectFrame* frames, int n, void* stream) {
    if (n < 1 || n > CVGS_SELECT_MAX_FRAMES) return (int)hipErrorInvalidValue;
    SelectArgs a;
    int most = 1;
    for (int i = 0; i < CVGS_SELECT_MAX_FRAMES; ++i) {
        a.f[i] = i < n ? frames[i] : SelectFrame{};
        if (i < n && frames[i].max_cand > most) most = frames[i].max_cand;
    }
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_select_rank, dim3((unsigned)((most + kRankBlock - 1) / kRankBlock), (unsigned)n, 1), dim3(kRankBlock, 1, 1), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_select_nms, dim3((unsigned)n, 1, 1), dim3(64, 1, 1), 0, s, a);
    return (int)hipGetLastError();
}

} // namespace cvgs
