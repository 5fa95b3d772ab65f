// cvgs_tick_merge.h -- may a fused K1 tick captured on a stream ride in the LAUNCH of the tick captured before it?
// Pure host logic (no HIP header), beside cvgs_tick_overlap.h whose footprints and node handles it uses: the driver in cvgs_tick_capture.h
// feeds it what the tick would launch (function, the comparable bytes of its argument block, chain count, largest batch, footprint) and the
// capture's dependency set, and has cvgs_api.cpp rewrite the previous tick's graph node when the answer is `merged`;
// tests/cpp/tick_merge_model.cpp holds it to a byte-set model without a GPU.
//
// THE SHAPE: one kernel node takes consecutive ticks until it is full.  The K1 tick kernel reads its chain from seg[blockIdx.z] and leaves
// early on a crop index beyond the chain's batch, so a tick joins a node by appending its segments (call order), growing gridDim.z by its
// chain count and gridDim.y to the larger batch.  All chains of a node run at once, at the place of the node's FIRST tick: a tick joins only
// if it is proven independent of EVERY tick the node holds (their summed footprint), launches the same function over an equal argument block,
// and the stream's dependency set is exactly the node -- then everything ordered before the tick is ordered before the node as well.
// Anything else opens a new node in order behind the stream's frontier.  The graph stays linear.
#pragma once

#include "cvgs_tick_overlap.h"

namespace cvgs {

// Most chains one node takes.  The argument block holds CVGS_MAX_CHAINS = 128 segments; 64 and 128 were measured on the headline and
// tie within the run-to-run spread (profiles/tick_merge_abab.txt: 2.306 us per frame both), so the cap is the block's: fewest launches.
constexpr int kTickMergeMaxChains = 128;
// The smallest tick (output pixels: planes x width x height) that is merged at all; smaller ticks keep the two-lane capture of
// cvgs_tick_overlap.h unchanged (its own size limit, kTickOverlapMaxPixels, stands beside the driver in cvgs_tick_capture.h).  Swept over ticks of 2, 4 and 16 frames of 50 crops to 64 x 128 (a tick of one chain is not a fused tick):
// merging won at every size (3.62 -> 2.53, 2.65 -> 2.30, 2.39 -> 2.30 us per frame), so the floor is the smallest size swept.
constexpr int64_t kTickMergeMinPixels = 100ll * 64 * 128;

enum class TickMerge {
    merged,
    unstated,          // the tick states no hull / no target extent: nothing can be proven about it
    first_tick,        // no node of this capture on the stream to join
    foreign_node,      // the stream's dependency set is not exactly the node the previous tick left
    other_streams,     // ticks of the same capture run on another stream: the caller has placed them
    different_launch,  // another kernel function, or an argument block that differs beyond what a segment carries
    dependent,         // not proven independent of every tick the node holds
    full,              // the node would hold more chains than the cap (or more ranges than its summed footprint may)
    graph_call_failed, // the runtime refused to rewrite the node
    n_reasons
};
const char* tick_merge_text(TickMerge r);

// What a tick would launch.
struct TickMergeTick {
    const void* fn = nullptr;       // the kernel function
    const void* key = nullptr;      // the bytes of its argument block that every tick of a node must share ...
    size_t key_bytes = 0;           // ... (the chain arguments and the geometry, without what each SEGMENT carries: table, tensor, batch, used)
    int chains = 0, max_batch = 0;
    const TickFootprint* fp = nullptr;
};

// The open node of ONE capture on ONE stream.
class TickMergeNode {
public:
    static constexpr size_t kMaxSummed = 4096; // ranges the summed footprint may hold
    // found: the stream's dependency set as the capture reports it; cap: kTickMergeMaxChains, or less
    TickMerge plan(unsigned long long capture_id, const TickNode* found, size_t n_found, const TickMergeTick& t, int cap = kTickMergeMaxChains) const;
    // the node was rewritten as plan() allowed; returns the index of the tick's first segment (the chains the node held before)
    int merged(const TickMergeTick& t);
    // the tick was captured in order as graph node `node` of its own: the next tick may join it.  node == nullptr: nothing is known, the state is dropped
    void opened(unsigned long long capture_id, TickNode node, const TickMergeTick& t);
    void drop() { live_ = false; }
    bool holds(unsigned long long capture_id) const { return live_ && id_ == capture_id; }
    TickNode node() const { return live_ ? node_ : nullptr; }
    int chains() const { return chains_; }
    int max_batch() const { return max_batch_; }
    int ticks() const { return ticks_; }
private:
    bool live_ = false;
    unsigned long long id_ = 0;
    TickNode node_ = nullptr;
    const void* fn_ = nullptr;
    std::vector<unsigned char> key_;
    int chains_ = 0, max_batch_ = 0, ticks_ = 0;
    TickFootprint sum_;
};

// Both rules of ONE stream, and which of them a captured tick follows.  A tick is routed to exactly one rule; the other rule's state is
// dropped, since it would describe a frontier the stream no longer has.
enum class TickPath { lanes, merge };
struct TickCaptureRules {
    TickLanes lanes;
    TickMergeNode merge;
    // merge_on: CVGS_TICK_MERGE; admitted: the lane rule's own admission (a K1 tick over device tables, nothing pooled rides on it);
    // pixels: the tick's output pixels.  Below the floor, switched off or not admitted: the lane code, exactly as it was.
    TickPath route(bool merge_on, bool admitted, int64_t pixels, int64_t min_pixels = kTickMergeMinPixels) {
        if (merge_on && admitted && pixels >= min_pixels) {
            lanes.drop();
            return TickPath::merge;
        }
        merge.drop();
        return TickPath::lanes;
    }
};

} // namespace cvgs
