// The shared selection text (cvgpuspeedup_amd/csrc/cvgs_geometry.h: select_prepare, select_precedes, select_suppresses) in a stand-alone
// program, for AddressSanitizer + UBSan (tests/test_box_select.py builds and runs it; no library, no HIP, no LD_PRELOAD).  It reads the
// test's seeded cases with the host entry's outputs from a text file of unsigned integers (floats as their bit patterns), drives the text
// the way k_select.hip does -- ranks by COUNTING predecessors into a working list of exactly pre_k slots, a kept list of exactly max_out
// slots -- and compares.  Exit 0: every case equal; 1: a difference; 2: a malformed file.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../cvgpuspeedup_amd/csrc/cvgs_geometry.h"

using namespace cvgs;

static bool rd(FILE* f, uint32_t* v) { return std::fscanf(f, "%u", v) == 1; }
static float as_f(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static uint32_t as_u(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fp = std::fopen(argv[1], "r");
    if (!fp) return 2;
    uint32_t n_cases = 0;
    if (!rd(fp, &n_cases)) return 2;
    int bad = 0;
    for (uint32_t c = 0; c < n_cases; ++c) {
        uint32_t h[14]; // fmt W H score_thr iou_thr pre_k max_out xf0 xf1 xf2 xf3 n live has_classes
        for (uint32_t& v : h)
            if (!rd(fp, &v)) return 2;
        const int fmt = (int)h[0], W = (int)h[1], H = (int)h[2], pre_k = (int)h[5], max_out = (int)h[6], n = (int)h[11], live = (int)h[12];
        const float score_thr = as_f(h[3]), iou_thr = as_f(h[4]);
        const float xf[4] = {as_f(h[7]), as_f(h[8]), as_f(h[9]), as_f(h[10])};
        std::vector<float> boxes((size_t)n * 4), scores((size_t)n);
        std::vector<int32_t> cls((size_t)n);
        for (int i = 0; i < n; ++i) {
            uint32_t v[6];
            for (uint32_t& x : v)
                if (!rd(fp, &x)) return 2;
            for (int e = 0; e < 4; ++e) boxes[(size_t)i * 4 + e] = as_f(v[e]);
            scores[(size_t)i] = as_f(v[4]);
            cls[(size_t)i] = h[13] ? (int32_t)v[5] : 0;
        }
        uint32_t want_kept = 0;
        if (!rd(fp, &want_kept)) return 2;
        std::vector<uint32_t> want((size_t)max_out * 6);
        for (uint32_t& v : want)
            if (!rd(fp, &v)) return 2;

        // steps 2-5
        std::vector<float> prep((size_t)n * 4);
        std::vector<char> member((size_t)n, 0);
        for (int i = 0; i < live; ++i)
            member[(size_t)i] = select_prepare(fmt, boxes[(size_t)i * 4], boxes[(size_t)i * 4 + 1], boxes[(size_t)i * 4 + 2], boxes[(size_t)i * 4 + 3], scores[(size_t)i],
                                               score_thr, xf, W, H, &prep[(size_t)i * 4]);
        // step 6 by counting, as k_select_rank does
        std::vector<int> work((size_t)pre_k, -1);
        int members = 0;
        for (int i = 0; i < live; ++i) {
            if (!member[(size_t)i]) continue;
            ++members;
            int rank = 0;
            for (int j = 0; j < live; ++j)
                if (member[(size_t)j] && select_precedes(scores[(size_t)j], j, scores[(size_t)i], i)) ++rank;
            if (rank < pre_k) {
                if (work[(size_t)rank] != -1) { std::printf("case %u: rank %d taken twice\n", c, rank); ++bad; }
                work[(size_t)rank] = i;
            }
        }
        const int n_work = members < pre_k ? members : pre_k;
        // step 7
        std::vector<int> kept((size_t)max_out, -1);
        int n_kept = 0;
        for (int w = 0; w < n_work && n_kept < max_out; ++w) {
            const int i = work[(size_t)w];
            if (i < 0) { std::printf("case %u: hole in the working list at %d\n", c, w); ++bad; break; }
            const float* bi = &prep[(size_t)i * 4];
            bool sup = false;
            for (int k = 0; k < n_kept && !sup; ++k) {
                const int j = kept[(size_t)k];
                const float* bj = &prep[(size_t)j * 4];
                sup = cls[(size_t)j] == cls[(size_t)i] && select_suppresses(bj[0], bj[1], bj[2], bj[3], bi[0], bi[1], bi[2], bi[3], iou_thr);
            }
            if (!sup) kept[(size_t)n_kept++] = i;
        }
        // step 8 against the host entry's outputs
        bool same = (uint32_t)n_kept == want_kept;
        for (int k = 0; k < max_out && same; ++k) {
            const int i = k < n_kept ? kept[(size_t)k] : -1;
            for (int e = 0; e < 4; ++e) same = same && want[(size_t)k * 6 + e] == (i >= 0 ? as_u(prep[(size_t)i * 4 + e]) : 0u);
            same = same && want[(size_t)k * 6 + 4] == (i >= 0 ? as_u(scores[(size_t)i]) : 0u) && want[(size_t)k * 6 + 5] == (uint32_t)i;
        }
        if (!same) { std::printf("case %u differs from the host entry (kept %d, want %u)\n", c, n_kept, want_kept); ++bad; }
    }
    std::fclose(fp);
    std::printf("%u cases, %d bad\n", n_cases, bad);
    return bad ? 1 : 0;
}
