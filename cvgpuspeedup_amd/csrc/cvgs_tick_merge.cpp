// cvgs_tick_merge.cpp -- the decision and the node bookkeeping of cvgs_tick_merge.h.  Host only, no HIP.
#include "cvgs_tick_merge.h"

#include <algorithm>
#include <cstring>

namespace cvgs {

const char* tick_merge_text(TickMerge r) {
    switch (r) {
    case TickMerge::merged: return "merged into the previous tick's launch";
    case TickMerge::unstated: return "in order, not merged: no hull stated (read.table_src_lo / _hi) or no known target extent";
    case TickMerge::first_tick: return "in order, not merged: no earlier tick of this capture on the stream";
    case TickMerge::foreign_node: return "in order, not merged: something else was captured since the previous tick";
    case TickMerge::other_streams: return "in order, not merged: ticks of this capture run on another stream as well";
    case TickMerge::different_launch: return "in order, not merged: another kernel, program, target shape or geometry than the previous tick's launch";
    case TickMerge::dependent: return "in order, not merged: not independent of the ticks in the previous launch";
    case TickMerge::full: return "in order, not merged: the previous launch is full";
    case TickMerge::graph_call_failed: return "in order, not merged: the graph node could not be rewritten";
    default: return "?";
    }
}

TickMerge TickMergeNode::plan(unsigned long long capture_id, const TickNode* found, size_t n_found, const TickMergeTick& t, int cap) const {
    if (!t.fp || t.fp->unknown) return TickMerge::unstated;
    if (!live_ || id_ != capture_id) return TickMerge::first_tick;
    if (n_found != 1 || found[0] != node_) return TickMerge::foreign_node;
    if (!t.fn || t.fn != fn_ || t.key_bytes != key_.size() || (t.key_bytes && std::memcmp(t.key, key_.data(), t.key_bytes) != 0)) return TickMerge::different_launch;
    if (!ticks_independent(sum_, *t.fp)) return TickMerge::dependent;
    if (t.chains < 1 || chains_ + t.chains > std::min(cap, kTickMergeMaxChains) || sum_.size() + t.fp->size() > kMaxSummed) return TickMerge::full;
    return TickMerge::merged;
}

int TickMergeNode::merged(const TickMergeTick& t) {
    const int first = chains_;
    chains_ += t.chains;
    max_batch_ = std::max(max_batch_, t.max_batch);
    ++ticks_;
    sum_.merge(*t.fp);
    return first;
}

void TickMergeNode::opened(unsigned long long capture_id, TickNode node, const TickMergeTick& t) {
    live_ = false;
    if (!node) return;
    live_ = true;
    id_ = capture_id;
    node_ = node;
    fn_ = t.fn;
    key_.assign((const unsigned char*)t.key, (const unsigned char*)t.key + (t.key ? t.key_bytes : 0));
    chains_ = t.chains;
    max_batch_ = t.max_batch;
    ticks_ = 1;
    sum_.clear();
    if (t.fp) sum_.merge(*t.fp);
    else sum_.unstated(); // (an unknown footprint: the node is kept as the stream's frontier, nothing joins it)
}

} // namespace cvgs
