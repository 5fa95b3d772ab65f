// The shared head-decoding text (cvgpuspeedup_amd/csrc/cvgs_geometry.h: head_best_step, head_best_wins, head_score, head_member, the two
// widenings) in a stand-alone program, for AddressSanitizer + UBSan (tests/test_head_decode.py builds and runs it; no library, no HIP,
// no LD_PRELOAD).  It reads the test's seeded cases (widened values as bit patterns) with the host entry's outputs from a text file of
// unsigned integers and drives the text the way k_head.hip does: the best class by groups of G lanes walking classes gl, gl + G, .. and
// a butterfly under head_best_wins (every G the kernels use, and G = 1: the column form); member counts per tile of 256; the prefix over
// tiles; packed positions and the tiles' tails into buffers of exactly N slots.  It also holds the fp16 widening to the compiler's own
// conversion on all 65536 patterns.  Exit 0: every case equal; 1: a difference; 2: a malformed file.
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

// step 2 the way a group of G lanes does it
static void best_by_group(const float* cls_scores, int C, int G, float* best, int* cls) {
    std::vector<float> b((size_t)G, -INFINITY);
    std::vector<int> k((size_t)G, 0);
    for (int gl = 0; gl < G; ++gl)
        for (int c = gl; c < C; c += G) head_best_step(cls_scores[c], c, &b[(size_t)gl], &k[(size_t)gl]);
    for (int off = G >> 1; off > 0; off >>= 1) {
        std::vector<float> nb(b);
        std::vector<int> nk(k);
        for (int gl = 0; gl < G; ++gl)
            if (head_best_wins(b[(size_t)(gl ^ off)], k[(size_t)(gl ^ off)], b[(size_t)gl], k[(size_t)gl])) {
                nb[(size_t)gl] = b[(size_t)(gl ^ off)];
                nk[(size_t)gl] = k[(size_t)(gl ^ off)];
            }
        b = nb;
        k = nk;
    }
    *best = b[0];
    *cls = k[0];
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    int bad = 0;
#if defined(__FLT16_MANT_DIG__)
    for (uint32_t h = 0; h < 65536; ++h) { // the fp16 widening against the compiler's (NaN: both NaN)
        _Float16 x;
        const uint16_t hb = (uint16_t)h;
        std::memcpy(&x, &hb, 2);
        const float want = (float)x, got = head_widen_f16(hb);
        if (want != want ? got == got : as_u(want) != as_u(got)) { std::printf("fp16 pattern %04x widens to %08x, want %08x\n", h, as_u(got), as_u(want)); ++bad; }
    }
#endif
    if (as_u(head_widen_bf16(0x3f80)) != 0x3f800000u || as_u(head_widen_bf16(0xff80)) != 0xff800000u) ++bad;

    FILE* fp = std::fopen(argv[1], "r");
    if (!fp) return 2;
    uint32_t n_cases = 0;
    if (!rd(fp, &n_cases)) return 2;
    for (uint32_t c = 0; c < n_cases; ++c) {
        uint32_t h[7]; // n a box_attr obj_attr+1 class_attr num_classes thr
        for (uint32_t& v : h)
            if (!rd(fp, &v)) return 2;
        const int n = (int)h[0], a = (int)h[1], box_attr = (int)h[2], obj_attr = (int)h[3] - 1, class_attr = (int)h[4], C = (int)h[5];
        const float thr = as_f(h[6]);
        std::vector<float> w((size_t)n * (size_t)a);
        for (float& v : w) {
            uint32_t u;
            if (!rd(fp, &u)) return 2;
            v = as_f(u);
        }
        uint32_t want_count = 0;
        if (!rd(fp, &want_count)) return 2;
        std::vector<uint32_t> want((size_t)n * 7);
        for (uint32_t& v : want)
            if (!rd(fp, &v)) return 2;

        // the score launch: steps 2-4 per candidate, member counts per tile
        const int tiles = (n + 255) / 256;
        std::vector<float> score((size_t)n);
        std::vector<int> code((size_t)n);
        std::vector<int> tile_count((size_t)tiles, 0);
        for (int i = 0; i < n; ++i) {
            const float* row = &w[(size_t)i * (size_t)a];
            float best = 0.f;
            int cls = -1;
            best_by_group(row + class_attr, C, 1, &best, &cls);
            for (int G = 4; G <= 64; G *= 2) {
                float gb = 0.f;
                int gk = -1;
                best_by_group(row + class_attr, C, G, &gb, &gk);
                if (as_u(gb) != as_u(best) || gk != cls) { std::printf("case %u candidate %d: a group of %d lanes finds (%08x, %d), one lane (%08x, %d)\n", c, i, G, as_u(gb), gk, as_u(best), cls); ++bad; }
            }
            const bool has_obj = obj_attr >= 0;
            const float s = head_score(best, has_obj, has_obj ? row[obj_attr] : 0.0f);
            const bool member = head_member(s, thr, row[box_attr], row[box_attr + 1], row[box_attr + 2], row[box_attr + 3]);
            score[(size_t)i] = s;
            code[(size_t)i] = cls | (member ? 1 << 16 : 0);
            tile_count[(size_t)(i / 256)] += member ? 1 : 0;
        }
        // the compact launch, tile by tile in REVERSE order (nothing may depend on the order): buffers of exactly n slots
        std::vector<float> bo((size_t)n * 4, -77.f), so((size_t)n, -77.f);
        std::vector<int32_t> ko((size_t)n, -77), io((size_t)n, -77);
        std::vector<char> written((size_t)n, 0);
        int count = -1;
        for (int t = tiles - 1; t >= 0; --t) {
            int base = 0, total = 0;
            for (int j = 0; j < tiles; ++j) {
                base += j < t ? tile_count[(size_t)j] : 0;
                total += tile_count[(size_t)j];
            }
            int pos = base;
            for (int i = t * 256; i < n && i < t * 256 + 256; ++i) {
                if (code[(size_t)i] & (1 << 16)) {
                    const float* row = &w[(size_t)i * (size_t)a];
                    if (written[(size_t)pos]++) { std::printf("case %u: position %d written twice\n", c, pos); ++bad; }
                    for (int e = 0; e < 4; ++e) bo[(size_t)pos * 4 + e] = row[box_attr + e];
                    so[(size_t)pos] = score[(size_t)i];
                    ko[(size_t)pos] = code[(size_t)i] & 0xffff;
                    io[(size_t)pos] = i;
                    ++pos;
                }
                if (i >= total) {
                    if (written[(size_t)i]++) { std::printf("case %u: tail position %d written twice\n", c, i); ++bad; }
                    for (int e = 0; e < 4; ++e) bo[(size_t)i * 4 + e] = 0.f;
                    so[(size_t)i] = 0.f;
                    ko[(size_t)i] = 0;
                    io[(size_t)i] = -1;
                }
            }
            if (t == 0) count = total;
        }
        bool same = (uint32_t)count == want_count;
        for (int j = 0; j < n && same; ++j) {
            same = written[(size_t)j] == 1;
            for (int e = 0; e < 4; ++e) same = same && want[(size_t)j * 7 + e] == as_u(bo[(size_t)j * 4 + e]);
            same = same && want[(size_t)j * 7 + 4] == as_u(so[(size_t)j]) && want[(size_t)j * 7 + 5] == (uint32_t)ko[(size_t)j] && want[(size_t)j * 7 + 6] == (uint32_t)io[(size_t)j];
        }
        if (!same) { std::printf("case %u differs from the host entry (count %d, want %u)\n", c, count, want_count); ++bad; }
    }
    std::fclose(fp);
    std::printf("%u cases, %d bad\n", n_cases, bad);
    return bad ? 1 : 0;
}
