// tick_overlap_model.cpp -- cvgs_tick_overlap.cpp (the decision whether a captured tick may run beside the ticks before it, and the two-lane
// bookkeeping) held to two brute-force models, without a GPU and without HIP.  A stand-alone program: tests/test_tick_overlap_model.py builds it
// with the host compiler and -fsanitize=address,undefined from this file and ../../cvgpuspeedup_amd/csrc/cvgs_tick_overlap.cpp, and runs it.
//
//   independence   ticks_independent against byte SETS: every range of a footprint marks its bytes in a 4 KiB arena; two ticks are independent
//                  iff no byte one of them writes is read or written by the other.  Seeded small footprints; the model must answer "independent"
//                  and "not independent" in at least a quarter of the cases each (asserted), unknown ranges are drawn on top.
//   lanes          TickLanes over random sequences of {overlappable tick, dependent tick, foreign node, new capture id}, played on a model
//                  of a capturing stream (a DAG of nodes, the stream's dependency set, set / add as the capture calls do them):
//                    * width: among any three ticks of a capture two are ordered, so at no time can a tick run beside more than one
//                      other (the earlier ticks a tick is NOT ordered after all lie on one chain of the DAG: the other lane);
//                    * safety: every tick is ordered after every earlier tick of its capture it is not independent of (byte sets again);
//                    * the final frontier reaches every node of the capture.
// Prints one summary line per part; exit status 0 only if every check held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cvgpuspeedup_amd/csrc/cvgs_tick_overlap.h"

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

struct ModelTick {
    TickFootprint fp;
    std::vector<uint8_t> rd = std::vector<uint8_t>(kArena, 0), wr = std::vector<uint8_t>(kArena, 0);
    bool unknown = false;
};

void add_range(ModelTick& t, bool write, int lo, int len) {
    if (write) t.fp.write(kBase + lo, kBase + lo + len);
    else t.fp.read(kBase + lo, kBase + lo + len);
    for (int b = lo; b < lo + len; ++b) (write ? t.wr : t.rd)[(size_t)b] = 1;
}

// a tick of `chains` chains inside a window of the arena: per chain a source hull, a table segment (reads) and a tensor (write)
ModelTick draw_tick(Rng& r, int window_lo, int window_len, int max_len) {
    ModelTick t;
    const int chains = 1 + r.below(3);
    for (int c = 0; c < chains; ++c)
        for (int k = 0; k < 3; ++k) {
            const int len = 1 + r.below(max_len);
            const int lo = window_lo + r.below(window_len - len + 1);
            add_range(t, k == 2, lo, len);
        }
    return t;
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

// ---- part 1 ----------------------------------------------------------------------------------------------------------------------------
void independence(uint64_t seed, int cases) {
    Rng r{seed};
    int indep = 0, dep = 0, unknown_cases = 0;
    for (int i = 0; i < cases; ++i) {
        // ranges of up to 96 bytes, six to eighteen per pair, anywhere in the arena: about half the pairs meet
        ModelTick a = draw_tick(r, 0, kArena, 96), b = draw_tick(r, 0, kArena, 96);
        const bool want = model_independent(a, b);
        (want ? indep : dep)++;
        CHECK(ticks_independent(a.fp, b.fp) == want, "case %d: ticks_independent=%d, byte sets say %d", i, (int)!want, (int)want);
        CHECK(ticks_independent(b.fp, a.fp) == want, "case %d: not symmetric", i);
        // the sum of two footprints against a third: what the lanes ask
        ModelTick c = draw_tick(r, 0, kArena, 96);
        TickFootprint sum;
        sum.merge(a.fp);
        sum.merge(b.fp);
        sum.merge(a.fp); // (identical ranges are kept once)
        CHECK(sum.size() <= a.fp.size() + b.fp.size(), "case %d: merge kept a range twice", i);
        CHECK(ticks_independent(sum, c.fp) == (model_independent(a, c) && model_independent(b, c)), "case %d: summed footprint", i);
        // an unknown range: null end, empty or reversed extent, or said outright
        if (i % 4 == 0) {
            ++unknown_cases;
            TickFootprint u = a.fp;
            switch ((i / 4) % 5) {
            case 0: u.read(nullptr, kBase + 8); break;
            case 1: u.write(kBase + 8, nullptr); break;
            case 2: u.read(kBase + 64, kBase + 64); break;
            case 3: u.write(kBase + 64, kBase + 32); break;
            default: u.unstated(); break;
            }
            TickFootprint far; // touches nothing a or u could meet
            far.write(kBase + 2 * kArena, kBase + 2 * kArena + 16);
            CHECK(u.unknown && !ticks_independent(u, far) && !ticks_independent(far, u), "case %d: an unknown range must answer 'not independent'", i);
            CHECK(ticks_independent(a.fp, far), "case %d: disjoint control", i);
        }
    }
    std::printf("independence: %d cases, byte sets say independent %d / not %d, %d with an unknown range\n", cases, indep, dep, unknown_cases);
    CHECK(4 * indep >= cases && 4 * dep >= cases, "the generator must give both outcomes in at least a quarter of the cases each (%d / %d of %d)", indep, dep, cases);
}

// ---- part 2: a capturing stream as a DAG ---------------------------------------------------------------------------------------------------
struct Node {
    std::vector<int> parents;
    int tick = -1; // index into ticks, -1: a foreign node
    unsigned long long capture = 0;
};
struct Graph {
    std::vector<Node> nodes;
    std::vector<std::vector<uint8_t>> reach; // reach[a][b]: a is ordered after b (b is an ancestor of a)
    int add(const std::vector<int>& parents, int tick, unsigned long long capture) {
        Node n;
        n.parents = parents;
        n.tick = tick;
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
    bool ordered(int a, int b) const { return a == b || after(a, b) || after(b, a); }
};
TickNode handle(int node) { return (TickNode)(uintptr_t)(0x1000 + 8 * (size_t)node); }
int node_of(TickNode h) { return (int)(((uintptr_t)h - 0x1000) / 8); }

void lanes(uint64_t seed, int sequences) {
    Rng r{seed};
    long n_ticks = 0, n_overlapped = 0, n_foreign = 0, n_captures = 0, max_partners = 0;
    long why[(int)TickOverlap::n_reasons] = {0};
    for (int s = 0; s < sequences; ++s) {
        Graph g;
        TickLanes state; // one stream
        std::vector<ModelTick> ticks;
        std::vector<int> tick_node;
        std::vector<int> stream_deps; // the stream's dependency set (node indices)
        unsigned long long capture = 1 + (unsigned long long)s * 1000;
        int capture_first_node = 0;
        ++n_captures;
        // each sequence owns a few disjoint windows of the arena: a tick drawn in a window of its own is independent of the others
        // ("overlappable"), one drawn in a window another tick used may not be ("dependent")
        const int n_windows = 2 + r.below(5), window = kArena / 8;
        const int steps = 4 + r.below(28);
        auto end_capture = [&] { // the final frontier reaches every node of the capture
            for (int n = capture_first_node; n < (int)g.nodes.size(); ++n) {
                bool reached = false;
                for (int d : stream_deps) reached = reached || d == n || g.after(d, n);
                CHECK(reached, "sequence %d: node %d of capture %llu is not behind the final frontier", s, n, capture);
            }
        };
        for (int step = 0; step < steps; ++step) {
            const int kind = r.below(16);
            if (kind == 0) { // a new capture on the same stream: another id, an empty dependency set
                end_capture();
                ++capture;
                ++n_captures;
                stream_deps.clear();
                capture_first_node = (int)g.nodes.size();
                continue;
            }
            if (kind == 1) { // a foreign node: captured in order behind the stream's dependency set, which it replaces
                const int n = g.add(stream_deps, -1, capture);
                stream_deps.assign(1, n);
                ++n_foreign;
                continue;
            }
            // a tick: mostly a window of the rotation (tick i takes window i % n_windows), sometimes anywhere, sometimes unstated
            ModelTick t = kind < 12 ? draw_tick(r, ((int)ticks.size() % n_windows) * window, window, 48) : draw_tick(r, 0, n_windows * window, 96);
            if (kind == 15) {
                t.fp.unstated();
                t.unknown = true;
            }
            std::vector<TickNode> found;
            for (int d : stream_deps) found.push_back(handle(d));
            const TickLanes::Plan p = state.plan(capture, found.data(), found.size(), t.fp);
            ++why[(int)p.why];
            int n;
            if (p.why == TickOverlap::overlapped) {
                std::vector<int> deps; // hipStreamSetCaptureDependencies, the launch, hipStreamAddCaptureDependencies
                for (TickNode h : p.deps) deps.push_back(node_of(h));
                for (int d : deps) CHECK(d >= capture_first_node && d < (int)g.nodes.size(), "sequence %d: a dependency outside the capture", s);
                n = g.add(deps, (int)ticks.size(), capture);
                stream_deps.assign(1, n);
                CHECK(p.beside != nullptr, "sequence %d: overlapped without a tick to run beside", s);
                stream_deps.push_back(node_of(p.beside));
                state.committed(p, handle(n), t.fp);
                ++n_overlapped;
            } else {
                n = g.add(stream_deps, (int)ticks.size(), capture);
                state.in_order(capture, found.data(), found.size(), handle(n), t.fp);
                stream_deps.assign(1, n);
            }
            { // the state's frontier is the stream's, unless the state was dropped
                const std::vector<TickNode> f = state.frontier();
                if (!f.empty()) {
                    CHECK(f.size() == stream_deps.size(), "sequence %d: frontier of %zu, stream holds %zu", s, f.size(), stream_deps.size());
                    for (TickNode h : f) {
                        bool in = false;
                        for (int d : stream_deps) in = in || d == node_of(h);
                        CHECK(in, "sequence %d: the state's frontier names a node the stream does not hold", s);
                    }
                }
            }
            ticks.push_back(t);
            tick_node.push_back(n);
            ++n_ticks;
            // safety and width, against every earlier tick of this capture
            const int me = (int)ticks.size() - 1;
            std::vector<int> partners; // earlier ticks this one is not ordered after
            for (int o = 0; o < me; ++o) {
                if (g.nodes[(size_t)tick_node[(size_t)o]].capture != capture) continue;
                if (g.after(n, tick_node[(size_t)o])) continue;
                partners.push_back(o);
                CHECK(model_independent(ticks[(size_t)o], ticks[(size_t)me]), "sequence %d: tick %d may run beside tick %d, which it is not independent of", s, me, o);
            }
            for (size_t i = 0; i < partners.size(); ++i)
                for (size_t j = i + 1; j < partners.size(); ++j)
                    CHECK(g.ordered(tick_node[(size_t)partners[i]], tick_node[(size_t)partners[j]]),
                          "sequence %d: ticks %d, %d and %d may all run at once", s, partners[i], partners[j], me);
            if ((long)partners.size() > max_partners) max_partners = (long)partners.size();
        }
        end_capture();
        // no tick is concurrent with more than one other: among every three ticks of a capture, two are ordered
        const auto cap_of = [&](size_t t) { return g.nodes[(size_t)tick_node[t]].capture; };
        for (size_t a = 0; a < tick_node.size(); ++a)
            for (size_t b = a + 1; b < tick_node.size(); ++b) {
                if (cap_of(a) != cap_of(b) || g.ordered(tick_node[a], tick_node[b])) continue;
                for (size_t c = b + 1; c < tick_node.size() && cap_of(c) == cap_of(a); ++c)
                    CHECK(g.ordered(tick_node[a], tick_node[c]) || g.ordered(tick_node[b], tick_node[c]), "sequence %d: ticks %zu, %zu, %zu form three lanes", s, a, b, c);
            }
    }
    std::printf("lanes: %d sequences, %ld captures, %ld ticks (%ld overlapped), %ld foreign nodes; longest run of ticks beside one lane %ld\n", sequences, n_captures, n_ticks,
                n_overlapped, n_foreign, max_partners);
    for (int k = 0; k < (int)TickOverlap::n_reasons; ++k)
        if (why[k]) std::printf("  %6ld  %s\n", why[k], tick_overlap_text((TickOverlap)k));
    CHECK(n_overlapped * 5 >= n_ticks, "the sequences must exercise the overlap: %ld of %ld ticks", n_overlapped, n_ticks);
    CHECK(why[(int)TickOverlap::dependent] > 0 && why[(int)TickOverlap::foreign_node] > 0 && why[(int)TickOverlap::unstated] > 0 && why[(int)TickOverlap::first_tick] > 0,
          "every refusal must occur");
}

} // namespace

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 0) : 0xC0FFEEull;
    const int cases = argc > 2 ? std::atoi(argv[2]) : 4000;
    const int sequences = argc > 3 ? std::atoi(argv[3]) : 1500;
    independence(seed, cases);
    lanes(seed + 1, sequences);
    std::printf(g_failures ? "FAILED: %d checks\n" : "OK\n", g_failures);
    return g_failures ? 1 : 0;
}
