// cvgs_tick_capture.h -- ONE captured tick driven through the two rules (cvgs_tick_overlap.h: two lanes; cvgs_tick_merge.h: one merged node).
// Pure host logic, header only, no HIP header: the capture is reached through a small stream type the caller supplies, so
// tests/cpp/tick_capture_model.cpp plays it on a fake stream -- failed capture calls included, which no GPU test can provoke.
//
// Stream (cvgs_api.cpp: the HIP adaptor; the model: a DAG with a frontier):
//   Launch                    the library's own copy of a kernel node's launch (default-constructible)
//   info(id, deps)            is a capture active?  Its id and the stream's dependency set (false: no dependencies)
//   set_deps / add_deps(nodes, n)  replace / extend the dependency set; false: the runtime refused
//   rewrite_node(node, l)     the node's launch `l` with this tick's segments appended; false: refused, `l` and the node as they were
// Pool (cvgs_api.cpp: ManyPool): captured_lock(), captured(key) -> TickCaptured<Launch>&, captured_on_other_streams(key, id).
//
// launch_tick's part is three steps: begin(); launch, unless the answer is `merged`; launched(), or abandon() when the launch failed.
// The pool's lock is held from begin() to the end of launched() / abandon(); an eager stream touches neither lock nor state nor counter.
#pragma once

#include <atomic>
#include <cstdio>
#include <memory>
#include <mutex>
#include <string>

#include "cvgs_tick_merge.h"

namespace cvgs {

// The largest tick (output pixels) that is captured beside another.  What the overlap hides is the launch's fixed 3.9 us; two ticks side by
// side share the memory system and pay for it.  Measured on the headline's crops (50 per frame to 64 x 128): ticks of 16 frames gain 3 %,
// ticks of 64 frames lose 2 % (profiles/tick_overlap_abab.txt).  The line is drawn between the two: 1600 planes of 64 x 128.
constexpr int64_t kTickOverlapMaxPixels = 1600ll * 64 * 128;

struct TickCaptureConfig {
    bool overlap_on = true, merge_on = true;        // CVGS_TICK_OVERLAP, CVGS_TICK_MERGE
    int64_t merge_min_pixels = kTickMergeMinPixels; // CVGS_TICK_MERGE_MIN_PIXELS
    int merge_max_chains = kTickMergeMaxChains;     // CVGS_TICK_MERGE_MAX_CHAINS, within [2, kTickMergeMaxChains]
    int64_t overlap_max_pixels = kTickOverlapMaxPixels;
};

// Process-wide: captured ticks by how they were captured (an eager tick is not counted).
struct TickCaptureCounters { std::atomic<uint64_t> overlapped{0}, in_order{0}, merged{0}; };
inline TickCaptureCounters g_tick_captures;

// What a successful cvgs_execute_many leaves for cvgs_last_error(): which rule took the tick and what it answered.
struct TickNote {
    enum class Path { none, lanes, merge };
    Path path = Path::none;
    const char* plain = nullptr; // path none: not a tick note -- a text given as it is ("not fused: ..."), or no note at all
    TickOverlap lane = TickOverlap::not_capturing;
    TickMerge merge = TickMerge::first_tick;
    int chains = 0;              // merged: the chains the node holds now
    explicit operator bool() const { return path != Path::none || plain; }
};
inline std::string tick_note_text(const TickNote& n, const TickCaptureCounters& c = g_tick_captures) {
    char tail[160], chains[32] = "";
    if (n.path == TickNote::Path::none) return n.plain ? n.plain : "";
    if (n.path == TickNote::Path::lanes) {
        std::snprintf(tail, sizeof(tail), " [captured ticks: %llu overlapped, %llu in order]", (unsigned long long)c.overlapped.load(), (unsigned long long)c.in_order.load());
        return std::string("tick: ") + tick_overlap_text(n.lane) + tail;
    }
    // the merge path: its own words, and the third counter in front of the two
    if (n.merge == TickMerge::merged) std::snprintf(chains, sizeof(chains), " (%d chains)", n.chains);
    std::snprintf(tail, sizeof(tail), "%s [merged ticks: %llu] [captured ticks: %llu overlapped, %llu in order]", chains, (unsigned long long)c.merged.load(),
                  (unsigned long long)c.overlapped.load(), (unsigned long long)c.in_order.load());
    return std::string("tick: ") + tick_merge_text(n.merge) + tail;
}

// Both rules of one stream and the library's copy of the open node's launch, from which the node is rewritten when a tick joins it.  Tied
// to ONE capture id -- never to the node's address, which a later capture may recycle.
template <class Launch>
struct TickCaptured : TickCaptureRules {
    std::unique_ptr<Launch> launch;
};

// What launch_tick states about the tick.
struct TickFacts {
    bool routed = true;    // false: a family the merge rule is never asked about (K4) -- its state is not even dropped
    bool admitted = false; // a K1 tick over device tables, nothing pooled or host-staged rides on the launch
    int64_t pixels = 0;    // output pixels: planes x width x height
    int chains = 0, max_batch = 0;
};

enum class TickBegin {
    launch_in_order, // launch the tick on the stream as it is
    launch_behind,   // the same: the stream's dependency set is already the lane's
    merged           // the tick rides in the previous tick's node: nothing to launch, nothing held
};

template <class Stream, class Pool, class Key>
class TickCapture {
public:
    using Launch = typename Stream::Launch;
    TickCapture(Stream& stream, Pool& pool, Key key, TickNote& note) : s_(stream), pool_(pool), key_(key), note_(note) {}
    ~TickCapture() { abandon(); }

    // footprint(fp): the bytes the tick reads and writes.  probe(launch, key): what the tick would launch, nothing enqueued -- fills the
    // record and the bytes every tick of a node must share, returns the kernel function or null (no record: a node nothing joins).
    // Never fails: every refusal and every refused runtime call leaves the stream as found and the tick in order.
    template <class Footprint, class Probe>
    TickBegin begin(const TickFacts& t, const TickCaptureConfig& cfg, Footprint&& footprint, Probe&& probe) {
        if (!s_.info(id_, found_)) return TickBegin::launch_in_order; // eager
        lock_ = pool_.captured_lock();
        state_ = &pool_.captured(key_);
        path_ = t.routed ? state_->route(cfg.merge_on, t.admitted, t.pixels, cfg.merge_min_pixels) : TickPath::lanes;
        if (path_ == TickPath::merge) {
            mine_.reset(new Launch());
            const void* fn = probe(*mine_, key_bytes_);
            footprint(fp_);
            if (!fn) fp_.unstated();
            tick_ = TickMergeTick{fn, key_bytes_.data(), key_bytes_.size(), t.chains, t.max_batch, &fp_};
            merge_why_ = state_->merge.plan(id_, found_.data(), found_.size(), tick_, cfg.merge_max_chains);
            if (merge_why_ == TickMerge::merged && pool_.captured_on_other_streams(key_, id_)) merge_why_ = TickMerge::other_streams;
            if (merge_why_ == TickMerge::merged && !(state_->launch && s_.rewrite_node(state_->merge.node(), *state_->launch))) merge_why_ = TickMerge::graph_call_failed;
            if (merge_why_ != TickMerge::merged) return TickBegin::launch_in_order;
            state_->merge.merged(tick_);
            note_ = TickNote{TickNote::Path::merge, nullptr, TickOverlap::not_capturing, TickMerge::merged, state_->merge.chains()};
            g_tick_captures.merged.fetch_add(1, std::memory_order_relaxed);
            release();
            return TickBegin::merged;
        }
        if (!cfg.overlap_on) lane_why_ = TickOverlap::switched_off;
        else if (!t.admitted) lane_why_ = TickOverlap::not_k1_tables;
        else if (t.pixels > cfg.overlap_max_pixels) lane_why_ = TickOverlap::large_tick;
        else {
            footprint(fp_);
            planned_ = state_->lanes.plan(id_, found_.data(), found_.size(), fp_);
            lane_why_ = planned_.why == TickOverlap::overlapped && pool_.captured_on_other_streams(key_, id_) ? TickOverlap::other_streams : planned_.why;
        }
        if (lane_why_ != TickOverlap::overlapped) {
            if (lane_why_ == TickOverlap::switched_off || lane_why_ == TickOverlap::not_k1_tables || lane_why_ == TickOverlap::large_tick) fp_.unstated(); // nothing may run beside this one
            return TickBegin::launch_in_order;
        }
        if (!s_.set_deps(planned_.deps.data(), planned_.deps.size())) {
            lane_why_ = TickOverlap::capture_call_failed;
            (void)s_.set_deps(found_.data(), found_.size()); // as found
            return TickBegin::launch_in_order;
        }
        rewritten_ = true;
        return TickBegin::launch_behind;
    }

    // The tick has been captured (or launched eagerly): the rule's state follows the stream, the note and a counter say how it went.
    // Null, or the one error: the frontier could not be put back, the capture would no longer order later work behind both lanes.
    const char* launched() {
        if (!state_) { // eager
            note_ = TickNote{TickNote::Path::lanes, nullptr, TickOverlap::not_capturing, TickMerge::first_tick, 0};
            return nullptr;
        }
        // the tick's node: the stream's dependency set names it
        unsigned long long id_now = 0;
        std::vector<TickNode> now;
        const TickNode node = s_.info(id_now, now) && id_now == id_ && now.size() == 1 ? now[0] : nullptr;
        const char* error = nullptr;
        if (path_ == TickPath::merge) {
            state_->merge.opened(id_, node, tick_); // a node of its own, which the next tick may join
            state_->launch.swap(mine_);             // the launch just captured is the record's (built by the probe from the same arguments)
        } else if (!rewritten_) {
            state_->lanes.in_order(id_, found_.data(), found_.size(), node, fp_);
        } else if (node && s_.add_deps(&planned_.beside, 1)) { // the other lane's last tick joins the frontier again
            state_->lanes.committed(planned_, node, fp_);
        } else { // put the whole frontier back by hand: everything found before the tick, and the tick (whatever the stream holds now)
            std::vector<TickNode> all(found_);
            all.insert(all.end(), now.begin(), now.end());
            if (!s_.set_deps(all.data(), all.size())) error = "captured tick: the stream's capture dependencies could not be restored";
            state_->lanes.drop();
            lane_why_ = TickOverlap::capture_call_failed;
        }
        (lane_why_ == TickOverlap::overlapped ? g_tick_captures.overlapped : g_tick_captures.in_order).fetch_add(1, std::memory_order_relaxed);
        note_ = TickNote{path_ == TickPath::merge ? TickNote::Path::merge : TickNote::Path::lanes, nullptr, lane_why_, merge_why_, 0};
        release();
        return error;
    }

    // The launch was refused or failed: the stream's dependency set as found, the routed rule's state dropped, nothing counted.
    void abandon() {
        if (!state_) return;
        if (rewritten_) (void)s_.set_deps(found_.data(), found_.size());
        if (path_ == TickPath::merge) state_->merge.drop();
        else state_->lanes.drop();
        release();
    }

private:
    void release() {
        state_ = nullptr;
        rewritten_ = false;
        if (lock_.owns_lock()) lock_.unlock();
    }
    Stream& s_;
    Pool& pool_;
    Key key_;       // the stream's key in the pool
    TickNote& note_;
    std::unique_lock<std::mutex> lock_;
    TickCaptured<Launch>* state_ = nullptr; // non-null: a capture is active and the lock is held
    TickPath path_ = TickPath::lanes;
    bool rewritten_ = false;                // the stream's dependency set is the lane's, not the one found
    unsigned long long id_ = 0;
    std::vector<TickNode> found_;
    TickFootprint fp_;
    TickLanes::Plan planned_;
    TickOverlap lane_why_ = TickOverlap::not_capturing;
    TickMerge merge_why_ = TickMerge::first_tick;
    TickMergeTick tick_;                    // the merge path: the tick, the record the probe built and the bytes its node must share
    std::unique_ptr<Launch> mine_;
    std::vector<unsigned char> key_bytes_;
};

} // namespace cvgs
