// cvgs_tick_overlap.cpp -- the decision and the lane bookkeeping of cvgs_tick_overlap.h.  Host only, no HIP.
#include "cvgs_tick_overlap.h"

#include <algorithm>

namespace cvgs {

void TickFootprint::add(std::vector<TickRange>& to, const void* lo, const void* hi) {
    const uintptr_t l = (uintptr_t)lo, h = (uintptr_t)hi;
    if (!l || !h || h <= l) { // nothing stated, or an empty / reversed extent: nothing can be proven about it
        unknown = true;
        return;
    }
    for (const TickRange& r : to)
        if (r.lo == l && r.hi == h) return;
    to.push_back(TickRange{l, h});
}

void TickFootprint::merge(const TickFootprint& o) {
    unknown = unknown || o.unknown;
    for (const TickRange& r : o.reads) add(reads, (const void*)r.lo, (const void*)r.hi);
    for (const TickRange& r : o.writes) add(writes, (const void*)r.lo, (const void*)r.hi);
}

namespace {
bool any_meet(const std::vector<TickRange>& a, const std::vector<TickRange>& b) {
    for (const TickRange& x : a)
        for (const TickRange& y : b)
            if (x.lo < y.hi && y.lo < x.hi) return true;
    return false;
}
bool same_set(const TickNode* a, size_t na, const std::vector<TickNode>& b) {
    if (na != b.size()) return false;
    for (size_t i = 0; i < na; ++i) {
        if (std::find(b.begin(), b.end(), a[i]) == b.end()) return false;
        if (std::find(a, a + i, a[i]) != a + i) return false; // (a node twice: not a set this code left)
    }
    return true;
}
} // namespace

bool ticks_independent(const TickFootprint& prev, const TickFootprint& cur) {
    if (prev.unknown || cur.unknown) return false;
    return !any_meet(prev.writes, cur.writes) && !any_meet(prev.writes, cur.reads) && !any_meet(cur.writes, prev.reads);
}

const char* tick_overlap_text(TickOverlap r) {
    switch (r) {
    case TickOverlap::overlapped: return "captured beside the previous tick";
    case TickOverlap::not_capturing: return "eager launch";
    case TickOverlap::switched_off: return "in order: CVGS_TICK_OVERLAP=0";
    case TickOverlap::not_k1_tables: return "in order: not a K1 tick over device tables, or pooled state rides on the launch";
    case TickOverlap::unstated: return "in order: no hull stated (read.table_src_lo / _hi) or no known target extent";
    case TickOverlap::first_tick: return "in order: no earlier tick of this capture on the stream";
    case TickOverlap::foreign_node: return "in order: something else was captured since the previous tick";
    case TickOverlap::dependent: return "in order: not independent of the ticks it would run beside";
    case TickOverlap::large_tick: return "in order: a tick this large gains nothing beside another";
    case TickOverlap::other_streams: return "in order: ticks of this capture run on another stream as well";
    case TickOverlap::capture_call_failed: return "in order: a capture-dependency call failed";
    default: return "?";
    }
}

std::vector<TickNode> TickLanes::frontier() const {
    std::vector<TickNode> f;
    if (!live_) return f;
    for (const Lane& l : lane_)
        if (l.last) f.push_back(l.last);
    return f;
}

TickLanes::Plan TickLanes::plan(unsigned long long capture_id, const TickNode* found, size_t n_found, const TickFootprint& fp) {
    Plan p;
    if (fp.unknown) { p.why = TickOverlap::unstated; return p; }
    if (!live_ || id_ != capture_id) { p.why = TickOverlap::first_tick; return p; }
    if (!same_set(found, n_found, frontier())) { p.why = TickOverlap::foreign_node; return p; }
    const Lane& beside = lane_[newest_];  // the lane this tick would run beside ...
    const Lane& mine = lane_[1 - newest_]; // ... and the one it continues
    if (!ticks_independent(beside.sum, fp) || mine.sum.size() + fp.size() > kMaxSummed) { p.why = TickOverlap::dependent; return p; }
    p.why = TickOverlap::overlapped;
    if (mine.last) p.deps.push_back(mine.last);
    else p.deps = parted_behind_;
    p.beside = beside.last;
    return p;
}

void TickLanes::committed(const Plan& p, TickNode node, const TickFootprint& fp) {
    (void)p;
    Lane& mine = lane_[1 - newest_];
    mine.last = node;
    mine.sum.merge(fp);
    newest_ = 1 - newest_;
}

void TickLanes::in_order(unsigned long long capture_id, const TickNode* found, size_t n_found, TickNode node, const TickFootprint& fp) {
    live_ = false;
    if (!node || fp.unknown) return;
    live_ = true;
    id_ = capture_id;
    parted_behind_.assign(found, found + n_found);
    lane_[0].last = node;
    lane_[0].sum.clear();
    lane_[0].sum.merge(fp);
    lane_[1].last = nullptr;
    lane_[1].sum.clear();
    newest_ = 0;
}

} // namespace cvgs
