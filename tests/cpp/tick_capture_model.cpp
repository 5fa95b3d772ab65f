// tick_capture_model.cpp -- cvgs_tick_capture.h (the driver that takes ONE captured tick through the lane rule or the merge rule: routing,
// refusals, the capture calls and what follows when the runtime refuses one, counters, the note) played on a fake capturing stream, without a
// GPU and without HIP.  A stand-alone program: tests/test_tick_capture_model.py builds it with the host compiler and
// -fsanitize=address,undefined from this file, ../../cvgpuspeedup_amd/csrc/cvgs_tick_merge.cpp and ../../cvgpuspeedup_amd/csrc/cvgs_tick_overlap.cpp.
//
// The fake stream is a DAG of nodes with recorded parents, a capture id and a dependency set (the frontier); it can be told to refuse the
// next set_deps, add_deps or rewrite_node.  Random sequences mix ticks over and under the merge floor, ticks over the lanes' size limit, ticks
// that are not admitted (routed, and the K4 kind the merge rule is never asked about), foreign nodes, new capture ids, eager ticks, "another
// stream holds this capture", unstated footprints, launches that fail and refused runtime calls.  Checked after every call:
//   * ordering and independence: whatever the stream had ordered in front of a tick is ordered in front of its node, or is a tick that an
//     exact byte-set model (written here, bit per byte) proves independent of it; any two ticks of a capture that share a node or are left
//     unordered are independent by that model;
//   * frontier: every node captured so far is reachable from the stream's dependency set -- after each refused call too; the driver reports
//     an error only when the restoring set_deps was refused as well, and then holds no state;
//   * bookkeeping: after a routed tick at most one rule's state is live; one counter moves per captured tick, none for an eager or a failed
//     one; the pool's lock is held from begin() to launched() / abandon() and at no other time;
//   * the route and the refusals the driver makes itself are the expected ones, and every reason of both rules occurs;
//   * two pinned sequences give literally the expected notes.
// Prints summary lines; exit status 0 only if every check held.
#include <algorithm>
#include <bitset>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../cvgpuspeedup_amd/csrc/cvgs_tick_capture.h"

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

constexpr int kArena = 1024;
uint8_t* const kBase = (uint8_t*)(uintptr_t)0x10000; // addresses only: nothing is dereferenced
constexpr int64_t kFloor = 1000;                      // the model's merge floor, in pixels ...
constexpr int64_t kLaneLimit = 600;                   // ... and its limit for a tick beside another

int g_failures = 0;
#define CHECK(cond, ...)                                                                                                                    \
    do {                                                                                                                                    \
        if (!(cond)) {                                                                                                                      \
            if (++g_failures <= 20) { std::printf("FAIL %s:%d  ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); }       \
        }                                                                                                                                   \
    } while (0)

struct ModelTick {
    TickFootprint fp;
    std::bitset<kArena> rd, wr;
    bool unknown = false;
    int fn = 0, key = 0, chains = 1, max_batch = 1;
    int64_t pixels = 0;
    bool admitted = true, routed = true;
    int node = -1;
    unsigned long long capture = 0;
};
void add_range(ModelTick& t, bool write, int lo, int len) {
    if (write) t.fp.write(kBase + lo, kBase + lo + len);
    else t.fp.read(kBase + lo, kBase + lo + len);
    for (int b = lo; b < lo + len; ++b) (write ? t.wr : t.rd).set((size_t)b);
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
    return (a.wr & (b.rd | b.wr)).none() && (b.wr & a.rd).none();
}

struct Node {
    std::vector<int> parents;
    std::vector<int> ticks; // the ticks that run in this node, in call order; empty: a foreign node
};
struct Graph {
    std::vector<Node> nodes;
    std::vector<std::vector<uint8_t>> reach; // reach[a][b]: a is ordered after b
    int add(const std::vector<int>& parents) {
        Node n;
        n.parents = parents;
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

struct FakeLaunch { int chains = 0, max_batch = 0; };
struct FakeStream {
    using Launch = FakeLaunch;
    bool capturing = true;
    unsigned long long id = 1;
    std::vector<int> deps;
    int refuse_set = 0, refuse_add = 0, refuse_rewrite = 0; // refuse that many of the next calls ...
    int refused = 0;                                         // ... and how many were
    int tick_chains = 0, tick_batch = 0, rewritten = -1, infos = 0;
    bool info(unsigned long long& id_out, std::vector<TickNode>& out) {
        ++infos;
        out.clear();
        if (!capturing) return false;
        id_out = id;
        for (int d : deps) out.push_back(handle(d));
        return true;
    }
    bool set_deps(const TickNode* nodes, size_t n) {
        if (refuse_set) { --refuse_set; ++refused; return false; }
        deps.clear();
        return add(nodes, n);
    }
    bool add_deps(const TickNode* nodes, size_t n) {
        if (refuse_add) { --refuse_add; ++refused; return false; }
        return add(nodes, n);
    }
    bool rewrite_node(TickNode node, FakeLaunch& l) {
        if (refuse_rewrite) { --refuse_rewrite; ++refused; return false; }
        l.chains += tick_chains;
        l.max_batch = std::max(l.max_batch, tick_batch);
        rewritten = node_of(node);
        return true;
    }
private:
    bool add(const TickNode* nodes, size_t n) {
        for (size_t i = 0; i < n; ++i)
            if (std::find(deps.begin(), deps.end(), node_of(nodes[i])) == deps.end()) deps.push_back(node_of(nodes[i]));
        return true;
    }
};
struct FakePool {
    std::mutex m;
    std::map<int, TickCaptured<FakeLaunch>> states;
    bool others = false;
    int locks = 0;
    std::unique_lock<std::mutex> captured_lock() { ++locks; return std::unique_lock<std::mutex>(m); }
    TickCaptured<FakeLaunch>& captured(int key) { return states[key]; }
    bool captured_on_other_streams(int, unsigned long long) const { return others; }
    bool locked() {
        if (!m.try_lock()) return true;
        m.unlock();
        return false;
    }
};
using Capture = TickCapture<FakeStream, FakePool, int>;

const unsigned char kKeys[3][6] = {{1, 2, 3, 4, 5, 6}, {1, 2, 3, 4, 5, 7}, {9, 2, 3, 4, 5, 6}};
const int kFns[2] = {11, 22};

struct Counts { uint64_t overlapped, in_order, merged; };
Counts counts() {
    return Counts{g_tick_captures.overlapped.load(), g_tick_captures.in_order.load(), g_tick_captures.merged.load()};
}

// One stream, its pool and the model of what has been captured on it.
struct World {
    Graph g;
    FakeStream s;
    FakePool pool;
    TickNote note;
    TickCaptureConfig cfg;
    std::vector<ModelTick> ticks;
    int capture_first = 0; // the first node of the running capture

    enum Outcome { eager, abandoned, captured, merged, error };
    // what to do to this tick: refuse runtime calls, fail the launch, keep the probe from building a record
    struct Hazards { bool set = false, add = false, rewrite = false, restore = false, launch = false, no_record = false; };

    bool frontier_holds() const {
        for (int n = capture_first; n < (int)g.nodes.size(); ++n) {
            bool held = false;
            for (int d : s.deps) held = held || d == n || g.after(d, n);
            if (!held) return false;
        }
        return true;
    }

    Outcome play(ModelTick t, const Hazards& h, int seq) {
        const std::vector<int> found = s.deps;
        std::vector<int> required; // everything the stream has ordered in front of this tick
        for (int n = 0; n < (int)g.nodes.size(); ++n)
            for (int d : found)
                if (d == n || g.after(d, n)) { required.push_back(n); break; }
        const Counts c0 = counts();
        const int locks0 = pool.locks;
        TickCaptured<FakeLaunch>& st = pool.captured(0);
        const bool lanes_held = st.lanes.holds(s.id), merge_held = st.merge.holds(s.id);
        s.refuse_set = h.set, s.refuse_add = h.add, s.refuse_rewrite = h.rewrite;
        s.tick_chains = t.chains, s.tick_batch = t.max_batch, s.rewritten = -1;
        const int refused0 = s.refused;
        TickFacts facts;
        facts.routed = t.routed, facts.admitted = t.admitted, facts.pixels = t.pixels, facts.chains = t.chains, facts.max_batch = t.max_batch;
        const bool merge_path = s.capturing && t.routed && cfg.merge_on && t.admitted && t.pixels >= cfg.merge_min_pixels;
        t.capture = s.id;
        Outcome out = captured;
        int nd = -1;
        {
            Capture cap(s, pool, 0, note);
            const TickBegin how = cap.begin(
                facts, cfg, [&](TickFootprint& fp) { fp = t.fp; },
                [&](FakeLaunch& l, std::vector<unsigned char>& key) -> const void* {
                    CHECK(merge_path, "sequence %d: the probe ran for a tick of the lanes", seq);
                    l.chains = t.chains, l.max_batch = t.max_batch;
                    key.assign(kKeys[t.key], kKeys[t.key] + sizeof(kKeys[0]));
                    if (h.no_record) t.unknown = true; // (the driver must treat the tick as one nothing is known about)
                    return h.no_record ? nullptr : &kFns[t.fn == kFns[1]];
                });
            if (!s.capturing) {
                CHECK(how == TickBegin::launch_in_order && cap.launched() == nullptr, "sequence %d: an eager tick", seq);
                const Counts c1 = counts();
                CHECK(pool.locks == locks0 && !pool.locked() && c1.overlapped == c0.overlapped && c1.in_order == c0.in_order && c1.merged == c0.merged &&
                          st.lanes.holds(s.id) == lanes_held && st.merge.holds(s.id) == merge_held, "sequence %d: an eager tick moved something", seq);
                CHECK(note.path == TickNote::Path::lanes && note.lane == TickOverlap::not_capturing, "sequence %d: an eager tick's note", seq);
                return eager;
            }
            CHECK(pool.locks == locks0 + 1, "sequence %d: the lock is taken once per tick", seq);
            if (how == TickBegin::merged) {
                CHECK(!pool.locked(), "sequence %d: a merged tick holds the lock", seq);
                CHECK(merge_path && found.size() == 1 && s.rewritten == found[0] && s.deps == found, "sequence %d: a merged tick joins the node the stream names", seq);
                CHECK(note.path == TickNote::Path::merge && note.merge == TickMerge::merged && note.chains == st.merge.chains() && st.launch && st.launch->chains == st.merge.chains() &&
                          st.launch->max_batch == st.merge.max_batch(), "sequence %d: a merged tick's note and the stored launch", seq);
                CHECK(!h.rewrite && !pool.others, "sequence %d: merged although refused", seq);
                nd = found[0];
                out = merged;
            } else {
                CHECK(pool.locked(), "sequence %d: the lock is held across the launch", seq);
                if (how == TickBegin::launch_in_order) CHECK(s.deps == found, "sequence %d: an in-order tick finds the stream changed", seq);
                else CHECK(!merge_path && !h.set && !pool.others, "sequence %d: behind a lane although refused", seq);
                if (h.launch) {
                    cap.abandon();
                    const Counts c1 = counts();
                    CHECK(s.deps == found && !pool.locked(), "sequence %d: a failed launch leaves the stream as found", seq);
                    CHECK(c1.overlapped == c0.overlapped && c1.in_order == c0.in_order && c1.merged == c0.merged, "sequence %d: a failed launch is counted", seq);
                    CHECK(merge_path ? !st.merge.holds(s.id) : !st.lanes.holds(s.id), "sequence %d: a failed launch keeps the routed rule's state", seq);
                    CHECK(t.routed ? !st.lanes.holds(s.id) && !st.merge.holds(s.id) : st.merge.holds(s.id) == merge_held, "sequence %d: a failed launch and the other rule's state", seq);
                    return abandoned;
                }
                nd = g.add(s.deps); // the launch: a node behind the stream's dependency set, which it replaces
                s.deps.assign(1, nd);
                if (h.restore && how == TickBegin::launch_behind) s.refuse_set = 1;
                const char* err = cap.launched();
                CHECK(!pool.locked(), "sequence %d: the lock is held after launched()", seq);
                if (err) {
                    CHECK(how == TickBegin::launch_behind && h.add && h.restore && s.refused - refused0 == 2, "sequence %d: an error without two refused calls", seq);
                    CHECK(!st.lanes.holds(s.id) && !st.merge.holds(s.id), "sequence %d: state recorded beside an error", seq);
                    CHECK(std::strcmp(err, "captured tick: the stream's capture dependencies could not be restored") == 0, "sequence %d: the error's text", seq);
                    out = error;
                } else {
                    CHECK(!(h.add && h.restore && how == TickBegin::launch_behind), "sequence %d: two refused calls and no error", seq);
                }
            }
        }
        CHECK(!pool.locked(), "sequence %d: the lock outlives the driver", seq);
        s.refuse_set = s.refuse_add = s.refuse_rewrite = 0;
        const int refused_now = s.refused - refused0;
        const Counts c1 = counts();
        if (out == merged) CHECK(c1.merged == c0.merged + 1 && c1.overlapped == c0.overlapped && c1.in_order == c0.in_order, "sequence %d: a merged tick's counters", seq);
        else CHECK(c1.merged == c0.merged && c1.overlapped + c1.in_order == c0.overlapped + c0.in_order + 1, "sequence %d: one counter per captured tick", seq);
        CHECK((c1.overlapped > c0.overlapped) == (note.path == TickNote::Path::lanes && note.lane == TickOverlap::overlapped), "sequence %d: the overlapped counter and the note", seq);
        // the route, and the refusals that are the driver's own
        CHECK((note.path == TickNote::Path::merge) == merge_path, "sequence %d: a tick of %lld pixels took the wrong path", seq, (long long)t.pixels);
        if (!merge_path) {
            const TickOverlap want = !cfg.overlap_on ? TickOverlap::switched_off : !t.admitted ? TickOverlap::not_k1_tables : t.pixels > cfg.overlap_max_pixels ? TickOverlap::large_tick : note.lane;
            CHECK(note.lane == want, "sequence %d: '%s', expected '%s'", seq, tick_overlap_text(note.lane), tick_overlap_text(want));
            CHECK((note.lane == TickOverlap::capture_call_failed) == (refused_now > 0), "sequence %d: %d refused capture calls, the note says '%s'", seq, refused_now, tick_overlap_text(note.lane));
            CHECK(!(pool.others && note.lane == TickOverlap::overlapped), "sequence %d: overlapped although another stream holds the capture", seq);
            if (t.routed) CHECK(!st.merge.holds(s.id), "sequence %d: both rules hold state", seq);
            else CHECK(st.merge.holds(s.id) == merge_held && !st.lanes.holds(s.id), "sequence %d: an unrouted tick touched the merge rule or left lanes", seq);
        } else {
            CHECK((note.merge == TickMerge::graph_call_failed) == (refused_now > 0), "sequence %d: a refused rewrite, the note says '%s'", seq, tick_merge_text(note.merge));
            CHECK(!st.lanes.holds(s.id), "sequence %d: both rules hold state", seq);
            if (out == captured) CHECK(st.merge.node() == handle(nd) && st.launch && st.launch->chains == t.chains && st.merge.chains() == t.chains, "sequence %d: the open node is not the tick's", seq);
            if (h.no_record) CHECK(note.merge == TickMerge::unstated, "sequence %d: a tick without a record must be unstated", seq);
        }
        CHECK(st.merge.chains() <= cfg.merge_max_chains || !st.merge.holds(s.id), "sequence %d: %d chains in a node", seq, st.merge.chains());
        // ordering, independence, frontier
        const int me = (int)ticks.size();
        t.node = nd;
        g.nodes[(size_t)nd].ticks.push_back(me);
        ticks.push_back(t);
        for (int p : required)
            if (p != nd && !g.after(nd, p)) CHECK(!g.nodes[(size_t)p].ticks.empty(), "sequence %d tick %d: not ordered behind foreign node %d", seq, me, p);
        for (int o = 0; o < me; ++o) {
            const ModelTick& e = ticks[(size_t)o];
            if (e.capture != t.capture || (e.node != nd && (g.after(nd, e.node) || g.after(e.node, nd)))) continue;
            CHECK(model_independent(e, ticks[(size_t)me]), "sequence %d: tick %d may run with tick %d, which it is not independent of", seq, me, o);
        }
        if (out != error) CHECK(frontier_holds(), "sequence %d tick %d: a captured node is not behind the stream's frontier (%d refused calls)", seq, me, refused_now);
        return out;
    }
};

ModelTick small_tick(int k, int chains) { // independent of its neighbours: a window of its own
    ModelTick t;
    add_range(t, false, 64 * k, 16);
    add_range(t, false, 64 * k + 16, 8);
    add_range(t, true, 64 * k + 32, 32);
    t.chains = chains;
    t.max_batch = 3;
    t.pixels = 384;
    return t;
}

// the two pinned sequences: first in the process, so the counters are theirs
void pinned_notes() {
    const char* lanes[4] = {"tick: in order: no earlier tick of this capture on the stream [captured ticks: 0 overlapped, 1 in order]",
                            "tick: captured beside the previous tick [captured ticks: 1 overlapped, 1 in order]",
                            "tick: captured beside the previous tick [captured ticks: 2 overlapped, 1 in order]",
                            "tick: captured beside the previous tick [captured ticks: 3 overlapped, 1 in order]"};
    World a;
    for (int k = 0; k < 4; ++k) {
        a.play(small_tick(k, 2), World::Hazards(), -1);
        CHECK(tick_note_text(a.note) == lanes[k], "four small ticks, tick %d: '%s'", k, tick_note_text(a.note).c_str());
    }
    const char* merge[3] = {"tick: in order, not merged: no earlier tick of this capture on the stream [merged ticks: 0] [captured ticks: 3 overlapped, 2 in order]",
                            "tick: merged into the previous tick's launch (4 chains) [merged ticks: 1] [captured ticks: 3 overlapped, 2 in order]",
                            "tick: merged into the previous tick's launch (6 chains) [merged ticks: 2] [captured ticks: 3 overlapped, 2 in order]"};
    World b;
    b.cfg.merge_min_pixels = 1;
    for (int k = 0; k < 3; ++k) {
        b.play(small_tick(k, 2), World::Hazards(), -2);
        CHECK(tick_note_text(b.note) == merge[k], "three merged ticks, tick %d: '%s'", k, tick_note_text(b.note).c_str());
    }
    b.s.capturing = false;
    b.play(small_tick(3, 2), World::Hazards(), -2);
    CHECK(tick_note_text(b.note) == "tick: eager launch [captured ticks: 3 overlapped, 2 in order]", "an eager tick: '%s'", tick_note_text(b.note).c_str());
    TickNote plain;
    CHECK(!plain && tick_note_text(plain).empty(), "an empty note");
    plain.plain = "not fused: one chain";
    CHECK(plain && tick_note_text(plain) == "not fused: one chain", "a plain note");
    std::printf("notes: %d pinned notes compared\n", 4 + 3 + 1 + 2);
}

void sequences(uint64_t seed, int n_sequences) {
    Rng r{seed};
    long n_ticks = 0, n_eager = 0, n_abandoned = 0, n_big = 0, n_merged = 0, n_small = 0, n_overlapped = 0, n_not_admitted = 0, n_unrouted = 0, n_foreign = 0, n_captures = 0;
    long most_chains = 0, seq_one = 0, seq_two = 0, n_errors = 0;
    long lane_why[(int)TickOverlap::n_reasons] = {0}, merge_why[(int)TickMerge::n_reasons] = {0};
    const Counts start = counts();
    long n_counted = 0;
    for (int s = 0; s < n_sequences; ++s) {
        World w;
        w.cfg.merge_min_pixels = kFloor;
        w.cfg.overlap_max_pixels = kLaneLimit;
        w.cfg.merge_max_chains = s % 3 == 0 ? 64 : kTickMergeMaxChains;
        w.cfg.overlap_on = s % 11 != 5;
        w.cfg.merge_on = s % 13 != 7;
        w.s.id = 1 + (unsigned long long)s * 1000;
        ++n_captures;
        const bool small_only = s % 5 == 4, fill = s % 7 == 3; // fill: compatible independent ticks of 16 chains until the node is full
        const int n_windows = fill ? 16 : 3 + r.below(6), window = fill ? kArena / 16 : kArena / 8;
        const int steps = fill ? 12 : 6 + r.below(40);
        const int small_share = s % 4 == 1 ? 5 : 1; // of six ticks: a sequence stays mostly on one side of the floor, so that a rule gets to work
        int refused_in_sequence = 0;
        for (int step = 0; step < steps; ++step) {
            const int kind = fill ? 5 : r.below(24);
            if (kind == 0) { // a new capture on the same stream: another id, an empty dependency set
                ++w.s.id;
                ++n_captures;
                w.s.deps.clear();
                w.capture_first = (int)w.g.nodes.size();
                continue;
            }
            if (kind == 1) { // a foreign node, in order behind the stream's dependency set, which it replaces
                w.s.deps.assign(1, w.g.add(w.s.deps));
                ++n_foreign;
                CHECK(w.frontier_holds(), "sequence %d: a foreign node", s);
                continue;
            }
            ModelTick t;
            // mostly a window of the rotation, sometimes anywhere (may meet an earlier tick), sometimes unstated
            if (kind < 18) draw_ranges(r, t, ((int)w.ticks.size() % n_windows) * window, window, fill ? 8 : 24);
            else draw_ranges(r, t, 0, n_windows * window, 48);
            if (kind == 23) {
                t.fp.unstated();
                t.unknown = true;
            }
            t.fn = kFns[!fill && r.below(16) == 0];
            t.key = !fill && r.below(10) == 0 ? 1 + r.below(2) : 0;
            t.chains = fill ? 16 : 1 + r.below(r.below(4) == 0 ? 48 : 16);
            t.max_batch = 1 + r.below(60);
            t.pixels = fill                              ? kFloor + 5
                       : small_only || r.below(6) < small_share ? (r.below(8) == 0 ? kLaneLimit + 1 + r.below((int)(kFloor - kLaneLimit - 1)) : 1 + r.below((int)kLaneLimit))
                                                         : kFloor + r.below(100000);
            t.admitted = fill || r.below(20) != 0;
            t.routed = t.admitted || r.below(2) == 0; // not admitted and not routed: a K4 tick
            World::Hazards h;
            if (!fill && r.below(10) == 0) {
                const int which = r.below(6);
                h.set = which == 0, h.add = which == 1 || which == 2, h.restore = which == 2, h.rewrite = which == 3, h.launch = which == 4, h.no_record = which == 5;
            }
            w.pool.others = !fill && r.below(24) == 0;
            w.s.capturing = fill || kind != 2;
            const int refused0 = w.s.refused;
            const World::Outcome out = w.play(t, h, s);
            w.s.capturing = true;
            refused_in_sequence += w.s.refused - refused0;
            ++n_ticks;
            if (out == World::eager) { ++n_eager; ++lane_why[(int)TickOverlap::not_capturing]; continue; }
            if (out == World::abandoned) { ++n_abandoned; continue; }
            ++n_counted;
            if (w.note.path == TickNote::Path::merge) {
                ++n_big;
                ++merge_why[(int)w.note.merge];
                n_merged += out == World::merged;
                most_chains = std::max(most_chains, (long)w.pool.captured(0).merge.chains());
            } else {
                ++lane_why[(int)w.note.lane];
                if (!t.admitted) { ++n_not_admitted; n_unrouted += !t.routed; }
                else if (t.pixels < kFloor) { ++n_small; n_overlapped += w.note.lane == TickOverlap::overlapped; }
            }
            if (out == World::error) { ++n_errors; break; } // (the capture is lost: its caller ends it)
        }
        seq_one += refused_in_sequence == 1;
        seq_two += refused_in_sequence == 2;
    }
    const Counts end = counts();
    CHECK((long)(end.overlapped + end.in_order + end.merged - start.overlapped - start.in_order - start.merged) == n_counted, "the counters' sum is not the number of captured ticks");
    std::printf("capture: %d sequences, %ld captures, %ld ticks (%ld eager, %ld with a failed launch): %ld over the floor (%ld merged), %ld under it and admitted (%ld overlapped), "
                "%ld not admitted (%ld never routed), %ld foreign nodes; most chains in a node %ld; refused calls: %ld sequences with one, %ld with two, %ld errors returned\n",
                n_sequences, n_captures, n_ticks, n_eager, n_abandoned, n_big, n_merged, n_small, n_overlapped, n_not_admitted, n_unrouted, n_foreign, most_chains, seq_one, seq_two, n_errors);
    for (int k = 0; k < (int)TickOverlap::n_reasons; ++k) std::printf("  lanes %6ld  %s\n", lane_why[k], tick_overlap_text((TickOverlap)k));
    for (int k = 0; k < (int)TickMerge::n_reasons; ++k) std::printf("  merge %6ld  %s\n", merge_why[k], tick_merge_text((TickMerge)k));
    for (int k = 0; k < (int)TickOverlap::n_reasons; ++k) CHECK(lane_why[k] > 0, "every reason must occur: '%s' did not", tick_overlap_text((TickOverlap)k));
    for (int k = 0; k < (int)TickMerge::n_reasons; ++k) CHECK(merge_why[k] > 0, "every reason must occur: '%s' did not", tick_merge_text((TickMerge)k));
    CHECK(n_merged * 4 >= n_big, "the sequences must exercise the merge: %ld of %ld ticks", n_merged, n_big);
    CHECK(n_overlapped * 5 >= n_small, "the sequences must exercise the lanes: %ld of %ld ticks", n_overlapped, n_small);
    CHECK(most_chains == kTickMergeMaxChains, "the cap must be reached and never passed: %ld", most_chains);
    CHECK(seq_one > 0 && seq_two > 0 && n_errors > 0 && n_eager > 0 && n_abandoned > 0 && n_unrouted > 0, "refused calls, errors, eager ticks, failed launches and unrouted ticks must occur");
}

} // namespace

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 0) : 0xC0FFEEull;
    const int n = argc > 2 ? std::atoi(argv[2]) : 3000;
    pinned_notes();
    sequences(seed, n);
    std::printf(g_failures ? "FAILED: %d checks\n" : "OK\n", g_failures);
    return g_failures ? 1 : 0;
}
