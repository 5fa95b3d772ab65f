// cvgs_tick_overlap.h -- may a fused tick captured on a stream run BESIDE the ticks captured before it, and behind which graph nodes?
// Pure host logic (no HIP header, no allocation policy of its own): the driver in cvgs_tick_capture.h feeds it the byte ranges a tick reads
// and writes and the capture's dependency sets as opaque node handles, and does what the answer says; tests/cpp/tick_overlap_model.cpp holds
// it to a byte-set model and to an ordering model without a GPU.
//
// THE SHAPE: two lanes, never more.  Consecutive overlappable ticks A B C D ... alternate between two chains of graph nodes: B is captured
// behind what stood in front of A (P), C behind A only, D behind B only.  The stream's frontier always holds both lanes' last ticks, so
// whatever is captured afterwards (and the end of the capture) waits for both.  A lane is ordered inside itself and behind P; it is NOT
// ordered against the other lane, so a tick joins lane L only if it is proven independent of EVERY tick the other lane has taken since the
// lanes parted (the sum of their footprints; the immediate predecessor is one of them).  Anything else -- a tick that cannot be proven
// independent, a node of another origin in the dependency set, another capture -- is captured in order behind the whole frontier, which
// joins the lanes; the next tick may part them again.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace cvgs {

struct TickRange { uintptr_t lo, hi; }; // [lo, hi)

// The bytes a fused tick touches: reads (every chain's stated source hull, every chain's plane-table segment) and writes (every chain's
// tensor range, out2, mirrors).  A range that cannot be stated (null end, hi <= lo, a vouched-but-unstated table, a chain with no hull)
// makes the whole footprint unknown: it is independent of nothing.
struct TickFootprint {
    std::vector<TickRange> reads, writes;
    bool unknown = false;
    void read(const void* lo, const void* hi) { add(reads, lo, hi); }
    void write(const void* lo, const void* hi) { add(writes, lo, hi); }
    void unstated() { unknown = true; }
    // the union of two footprints (identical ranges are kept once: a rotation of resident frames repeats them)
    void merge(const TickFootprint& o);
    void clear() { reads.clear(); writes.clear(); unknown = false; }
    size_t size() const { return reads.size() + writes.size(); }
private:
    void add(std::vector<TickRange>& to, const void* lo, const void* hi);
};

// No write range of either meets a read or a write range of the other; false when either is unknown.
bool ticks_independent(const TickFootprint& prev, const TickFootprint& cur);

// Why a tick was, or was not, captured beside its predecessor (tick_overlap_text: the words of the note cvgs_last_error() gives).
enum class TickOverlap {
    overlapped,
    not_capturing,    // eager launches are untouched (not counted)
    switched_off,     // CVGS_TICK_OVERLAP=0
    not_k1_tables,    // another family, another carrier, or pooled / host-staged state rides on the launch
    unstated,         // a chain with no stated hull (vouched tables included), a target without a known extent
    first_tick,       // nothing of this capture to run beside yet
    foreign_node,     // the stream's dependency set is not the frontier the previous tick left
    dependent,        // not proven independent of the other lane's ticks
    large_tick,       // the launch's fixed cost is too small a share of a tick this size for the overlap to pay
    other_streams,    // ticks of the same capture already run on another stream: the caller has placed them, two lanes stay two
    capture_call_failed,
    n_reasons
};
const char* tick_overlap_text(TickOverlap r);

using TickNode = const void*; // an opaque graph node handle

// The lanes of ONE capture on ONE stream.  plan() decides from the dependency set found on the stream and the tick's footprint; the caller
// captures the tick behind `deps` and reports the node with committed() -- or, when a capture call failed, captures it in order and says so
// with in_order().  Every path leaves the state describing the frontier the stream really has.
class TickLanes {
public:
    static constexpr size_t kMaxSummed = 4096; // ranges a lane's summed footprint may hold before the lanes are joined

    struct Plan {
        TickOverlap why = TickOverlap::first_tick;
        std::vector<TickNode> deps;   // overlapped: capture the tick behind exactly these ...
        TickNode beside = nullptr;    // ... and add this node (the other lane's last tick) to the frontier afterwards
    };
    // found: the stream's dependency set as the capture reports it (any order); fp: this tick's footprint
    Plan plan(unsigned long long capture_id, const TickNode* found, size_t n_found, const TickFootprint& fp);
    // the tick was captured as plan said (overlapped) and is graph node `node`
    void committed(const Plan& p, TickNode node, const TickFootprint& fp);
    // the tick was captured IN ORDER behind the dependency set `found` (a refusal, or a failed capture call) and is graph node `node`;
    // node == nullptr or an unknown footprint: nothing may run beside it, the state is dropped
    void in_order(unsigned long long capture_id, const TickNode* found, size_t n_found, TickNode node, const TickFootprint& fp);
    void drop() { live_ = false; }
    // does the state describe ticks of this capture?
    bool holds(unsigned long long capture_id) const { return live_ && id_ == capture_id; }
    // the frontier the state expects on the stream (for tests): both lanes' last ticks
    std::vector<TickNode> frontier() const;
private:
    struct Lane { TickNode last = nullptr; TickFootprint sum; };
    bool live_ = false;
    unsigned long long id_ = 0;
    std::vector<TickNode> parted_behind_; // P: the dependency set in front of the tick the lanes parted at
    Lane lane_[2];
    int newest_ = 0; // the lane of the newest tick
};

} // namespace cvgs
