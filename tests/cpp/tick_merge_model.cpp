// tick_merge_model.cpp -- cvgs_tick_merge.cpp (may a captured tick ride in the previous tick's launch, and the bookkeeping of the node that
// takes it) held to a brute-force model, without a GPU and without HIP.  A stand-alone program: tests/test_tick_merge_model.py builds it with
// the host compiler and -fsanitize=address,undefined from this file, ../../cvgpuspeedup_amd/csrc/cvgs_tick_merge.cpp and
// ../../cvgpuspeedup_amd/csrc/cvgs_tick_overlap.cpp, and runs it.
//
// Random sequences of {tick, foreign node, new capture id} are played on a model of a capturing stream: a DAG of nodes, each holding the
// ticks that run in it at once, and the stream's dependency set.  Ticks differ in size (under / over the floor), footprint (byte sets in a
// 4 KiB arena), kernel function, argument block, chain count and largest batch.  Checked, for every tick:
//   * the decision is EXACTLY the model's: merged iff the stream's dependency set is the open node of this capture, function and argument
//     block equal the node's, the tick is independent (byte sets) of every tick the node holds, and the chains fit the cap;
//   * a merged tick's first segment is the node's chain count before it (segment order is call order), the node's chain count never
//     exceeds the cap and its largest batch is the maximum of its ticks';
//   * ordering: everything the stream had ordered in front of the tick is ordered in front of its node, or shares the node with it and is
//     independent of it, or (the lanes) is a tick independent of it;
//   * ticks under the floor follow the lane rule unchanged: in sequences of small ticks only, every plan equals a plain TickLanes' plan.
// Prints summary lines; exit status 0 only if every check held.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cvgpuspeedup_amd/csrc/cvgs_tick_merge.h"

using namespace cvgs;

namespace {

struct Rng { // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    int below(int n) { return (int)(next() % (uint64_t)n); }
};

constexpr int kArena = 4096;
uint8_t* const kBase = (uint8_t*)(uintptr_t)0x10000; // addresses only: nothing is dereferenced
constexpr int64_t kFloor = 1000;                      // the model's size floor, in pixels

struct ModelTick {
    TickFootprint fp;
    std::vector<uint8_t> rd = std::vector<uint8_t>(kArena, 0), wr = std::vector<uint8_t>(kArena, 0);
    bool unknown = false;
    int fn = 0, key = 0, chains = 1, max_batch = 1;
    int64_t pixels = 0;
    int node = -1, first_seg = 0;
};

void add_range(ModelTick& t, bool write, int lo, int len) {
    if (write) t.fp.write(kBase + lo, kBase + lo + len);
    else t.fp.read(kBase + lo, kBase + lo + len);
    for (int b = lo; b < lo + len; ++b) (write ? t.wr : t.rd)[(size_t)b] = 1;
}

// per chain a source hull and a table segment (reads) and a tensor (write), inside a window of the arena
void draw_ranges(Rng& r, ModelTick& t, int window_lo, int window_len, int max_len) {
    const int n = 1 + r.below(3);
    for (int c = 0; c < n; ++c)
        for (int k = 0; k < 3; ++k) {
            const int len = 1 + r.below(max_len);
            add_range(t, k == 2, window_lo + r.below(window_len - len + 1), len);
        }
}

bool model_independent(const ModelTick& a, const ModelTick& b) {
    if (a.unknown || b.unknown) return false;
    for (int i = 0; i < kArena; ++i)
        if ((a.wr[(size_t)i] && (b.rd[(size_t)i] || b.wr[(size_t)i])) || (b.wr[(size_t)i] && a.rd[(size_t)i])) return false;
    return true;
}

int g_failures = 0;
#define CHECK(cond, ...)                                                                                                                    \
    do {                                                                                                                                    \
        if (!(cond)) {                                                                                                                      \
            if (++g_failures <= 20) { std::printf("FAIL %s:%d  ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); }       \
        }                                                                                                                                   \
    } while (0)

struct Node {
    std::vector<int> parents;
    std::vector<int> ticks; // the ticks that run in this node, in call order; empty: a foreign node
    unsigned long long capture = 0;
};
struct Graph {
    std::vector<Node> nodes;
    std::vector<std::vector<uint8_t>> reach; // reach[a][b]: a is ordered after b
    int add(const std::vector<int>& parents, unsigned long long capture) {
        Node n;
        n.parents = parents;
        n.capture = capture;
        nodes.push_back(n);
        std::vector<uint8_t> row(nodes.size(), 0);
        for (int p : parents) {
            row[(size_t)p] = 1;
            for (size_t k = 0; k < reach[(size_t)p].size(); ++k)
                if (reach[(size_t)p][k]) row[k] = 1;
        }
        reach.push_back(row);
        return (int)nodes.size() - 1;
    }
    bool after(int a, int b) const { return (size_t)b < reach[(size_t)a].size() && reach[(size_t)a][(size_t)b]; }
};
TickNode handle(int node) { return (TickNode)(uintptr_t)(0x1000 + 8 * (size_t)node); }
int node_of(TickNode h) { return (int)(((uintptr_t)h - 0x1000) / 8); }

const unsigned char kKeys[3][6] = {{1, 2, 3, 4, 5, 6}, {1, 2, 3, 4, 5, 7}, {9, 2, 3, 4, 5, 6}};
const int kFns[2] = {11, 22};

void sequences(uint64_t seed, int n_sequences) {
    Rng r{seed};
    long n_ticks = 0, n_big = 0, n_merged = 0, n_lane = 0, n_overlapped = 0, n_foreign = 0, n_captures = 0, n_small_only = 0, n_small_compared = 0, most_chains = 0, full_nodes = 0;
    long why[(int)TickMerge::n_reasons] = {0};
    for (int s = 0; s < n_sequences; ++s) {
        Graph g;
        TickCaptureRules rules; // one stream
        const bool small_only = s % 5 == 4;
        TickLanes shadow;       // small_only: a plain TickLanes fed the same ticks
        n_small_only += small_only;
        const int cap = s % 3 == 0 ? 64 : kTickMergeMaxChains;
        std::vector<ModelTick> ticks;
        std::vector<int> stream_deps;
        unsigned long long capture = 1 + (unsigned long long)s * 1000;
        ++n_captures;
        // the model's idea of the open node
        int open = -1, open_fn = 0, open_key = 0, open_chains = 0, open_batch = 0;
        unsigned long long open_capture = 0;
        const int n_windows = 3 + r.below(6), window = kArena / 8;
        const int steps = 6 + r.below(40);
        for (int step = 0; step < steps; ++step) {
            const int kind = r.below(20);
            if (kind == 0) { // a new capture on the same stream: another id, an empty dependency set
                ++capture;
                ++n_captures;
                stream_deps.clear();
                continue;
            }
            if (kind == 1) { // a foreign node, in order behind the stream's dependency set, which it replaces
                stream_deps.assign(1, g.add(stream_deps, capture));
                ++n_foreign;
                continue;
            }
            ModelTick t;
            // mostly a window of the rotation, sometimes anywhere (may meet an earlier tick), sometimes unstated
            if (kind < 16) draw_ranges(r, t, ((int)ticks.size() % n_windows) * window, window, 48);
            else draw_ranges(r, t, 0, n_windows * window, 96);
            if (kind == 19) {
                t.fp.unstated();
                t.unknown = true;
            }
            t.fn = kFns[r.below(12) == 0];
            t.key = r.below(8) == 0 ? 1 + r.below(2) : 0;
            t.chains = 1 + r.below(r.below(4) == 0 ? 48 : 16);
            t.max_batch = 1 + r.below(60);
            t.pixels = small_only || r.below(6) == 0 ? r.below((int)kFloor) : kFloor + r.below(100000);
            const bool admitted = small_only || r.below(24) != 0;

            std::vector<TickNode> found;
            for (int d : stream_deps) found.push_back(handle(d));
            std::vector<int> required; // everything the stream has ordered in front of this tick
            for (int n = 0; n < (int)g.nodes.size(); ++n)
                for (int d : stream_deps)
                    if (d == n || g.after(d, n)) {
                        required.push_back(n);
                        break;
                    }
            const int me = (int)ticks.size();
            int nd;
            if (rules.route(true, admitted, t.pixels, kFloor) == TickPath::lanes) {
                CHECK(t.pixels < kFloor || !admitted, "sequence %d: a tick of %lld pixels took the lanes", s, (long long)t.pixels);
                ++n_lane;
                open = -1;
                const TickLanes::Plan p = rules.lanes.plan(capture, found.data(), found.size(), t.fp);
                if (small_only) {
                    const TickLanes::Plan q = shadow.plan(capture, found.data(), found.size(), t.fp);
                    CHECK(p.why == q.why && p.deps == q.deps && p.beside == q.beside, "sequence %d: a small tick's plan differs from a plain TickLanes'", s);
                    ++n_small_compared;
                }
                if (p.why == TickOverlap::overlapped) {
                    std::vector<int> deps;
                    for (TickNode h : p.deps) deps.push_back(node_of(h));
                    nd = g.add(deps, capture);
                    stream_deps.assign(1, nd);
                    stream_deps.push_back(node_of(p.beside));
                    rules.lanes.committed(p, handle(nd), t.fp);
                    if (small_only) shadow.committed(p, handle(nd), t.fp);
                    ++n_overlapped;
                } else {
                    nd = g.add(stream_deps, capture);
                    rules.lanes.in_order(capture, found.data(), found.size(), handle(nd), t.fp);
                    if (small_only) shadow.in_order(capture, found.data(), found.size(), handle(nd), t.fp);
                    stream_deps.assign(1, nd);
                }
                g.nodes[(size_t)nd].ticks.push_back(me);
            } else {
                CHECK(t.pixels >= kFloor && admitted, "sequence %d: a tick under the floor took the merge path", s);
                ++n_big;
                TickMergeTick mt;
                mt.fn = &kFns[t.fn == kFns[1]];
                mt.key = kKeys[t.key];
                mt.key_bytes = sizeof(kKeys[0]);
                mt.chains = t.chains;
                mt.max_batch = t.max_batch;
                mt.fp = &t.fp;
                const TickMerge got = rules.merge.plan(capture, found.data(), found.size(), mt, cap);
                ++why[(int)got];
                bool want = open >= 0 && open_capture == capture && stream_deps.size() == 1 && stream_deps[0] == open && open_fn == t.fn && open_key == t.key &&
                            open_chains + t.chains <= cap && !t.unknown;
                if (want)
                    for (int o : g.nodes[(size_t)open].ticks) want = want && model_independent(ticks[(size_t)o], t);
                CHECK((got == TickMerge::merged) == want, "sequence %d tick %d: decision '%s', the model says %s", s, me, tick_merge_text(got), want ? "merge" : "do not merge");
                // the refusals the issue names, each on its own
                if (open < 0 || open_capture != capture) CHECK(got == TickMerge::first_tick || got == TickMerge::unstated, "sequence %d: another capture must start a new node", s);
                else if (stream_deps.size() != 1 || stream_deps[0] != open) CHECK(got == TickMerge::foreign_node || got == TickMerge::unstated, "sequence %d: a foreign dependency must start a new node", s);
                else if (open_fn != t.fn || open_key != t.key) CHECK(got == TickMerge::different_launch || got == TickMerge::unstated, "sequence %d: a differing argument block must start a new node", s);
                if (got == TickMerge::merged) {
                    nd = open;
                    t.first_seg = rules.merge.merged(mt);
                    CHECK(t.first_seg == open_chains, "sequence %d tick %d: first segment %d, the node held %d chains", s, me, t.first_seg, open_chains);
                    open_chains += t.chains;
                    open_batch = std::max(open_batch, t.max_batch);
                    g.nodes[(size_t)nd].ticks.push_back(me);
                    ++n_merged;
                } else {
                    if (got == TickMerge::full) ++full_nodes;
                    nd = g.add(stream_deps, capture);
                    rules.merge.opened(capture, handle(nd), mt);
                    stream_deps.assign(1, nd);
                    g.nodes[(size_t)nd].ticks.push_back(me);
                    open = nd, open_capture = capture, open_fn = t.fn, open_key = t.key, open_chains = t.chains, open_batch = t.max_batch;
                }
                CHECK(rules.merge.chains() == open_chains && rules.merge.chains() <= cap, "sequence %d: the node holds %d chains (model %d, cap %d)", s, rules.merge.chains(), open_chains, cap);
                CHECK(rules.merge.max_batch() == open_batch, "sequence %d: largest batch %d, the model says %d", s, rules.merge.max_batch(), open_batch);
                CHECK(rules.merge.node() == handle(open) && rules.merge.ticks() == (int)g.nodes[(size_t)open].ticks.size(), "sequence %d: the open node", s);
                most_chains = std::max(most_chains, (long)open_chains);
            }
            t.node = nd;
            ticks.push_back(t);
            ++n_ticks;
            // ordering
            for (int p : required) {
                if (p != nd && g.after(nd, p)) continue;
                CHECK(!g.nodes[(size_t)p].ticks.empty(), "sequence %d tick %d: not ordered behind foreign node %d", s, me, p);
                for (int o : g.nodes[(size_t)p].ticks)
                    if (o != me) CHECK(model_independent(ticks[(size_t)o], ticks[(size_t)me]), "sequence %d: tick %d may run with tick %d, which it is not independent of", s, me, o);
            }
            // segments in call order, back to back
            int at = 0;
            for (int o : g.nodes[(size_t)nd].ticks) {
                if (rules.merge.node() != handle(nd)) break; // (a node of the lanes)
                CHECK(ticks[(size_t)o].first_seg == at, "sequence %d: segments of node %d out of call order", s, nd);
                at += ticks[(size_t)o].chains;
            }
        }
    }
    std::printf("merge: %d sequences (%ld of small ticks only), %ld captures, %ld ticks: %ld over the floor (%ld merged), %ld under it (%ld overlapped, %ld plans compared), "
                "%ld foreign nodes; most chains in a node %ld, %ld nodes found full\n",
                n_sequences, n_small_only, n_captures, n_ticks, n_big, n_merged, n_lane, n_overlapped, n_small_compared, n_foreign, most_chains, full_nodes);
    for (int k = 0; k < (int)TickMerge::n_reasons; ++k)
        if (why[k]) std::printf("  %6ld  %s\n", why[k], tick_merge_text((TickMerge)k));
    CHECK(n_merged * 4 >= n_big, "the sequences must exercise the merge: %ld of %ld ticks", n_merged, n_big);
    CHECK(n_overlapped * 5 >= n_lane && n_small_compared > 0, "the sequences must exercise the lanes: %ld of %ld ticks", n_overlapped, n_lane);
    CHECK(most_chains > 64 && most_chains <= kTickMergeMaxChains && full_nodes > 0, "the cap must be reached");
    for (TickMerge must : {TickMerge::unstated, TickMerge::first_tick, TickMerge::foreign_node, TickMerge::different_launch, TickMerge::dependent, TickMerge::full})
        CHECK(why[(int)must] > 0, "every refusal must occur: '%s' did not", tick_merge_text(must));
}

} // namespace

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 0) : 0xC0FFEEull;
    const int n = argc > 2 ? std::atoi(argv[2]) : 3000;
    sequences(seed, n);
    std::printf(g_failures ? "FAILED: %d checks\n" : "OK\n", g_failures);
    return g_failures ? 1 : 0;
}
