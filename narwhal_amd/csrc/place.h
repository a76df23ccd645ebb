// place.h -- which device object of a multi-device context serves a call (host code, no HIP).
//
// One load table per context, one entry per device object.  A call that is one range goes to the
// device with the fewest outstanding ranges; ties go to the fewest outstanding items, then to the
// lowest index.  The choice and the increment are one step under the table's mutex, so two callers
// that look at the same moment do not both take the same idle device.  The lowest-index tie-break
// is deliberate: a caller that issues one call at a time stays on device 0 (warm lane buffers, key
// cache, BLS signature ring); only overlapping callers spread.
//
// A call that splits into k > 1 ranges takes base = cursor++ mod ndev and runs range j on device
// (base + j) mod ndev: consecutive large calls rotate, so range 0 does not always land on device 0.
//
// A Ticket is the call's hold on its entry: taken before the lane is leased (a caller waiting for
// a lane counts as load), released by its destructor on every path.
//
// mode FIRST (env NWV_PLACE=first) keeps the rule the engine had before this table: a single
// range on device 0, range k on device k.  The counters are kept in both modes.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

namespace nwv {

enum PlaceMode { PLACE_LOAD = 0, PLACE_FIRST = 1 };

// NWV_PLACE as read at nwv_init: "first" keeps device 0 / device k; anything else is by load
inline PlaceMode place_mode_from_env() {
    const char* e = std::getenv("NWV_PLACE");
    return (e && std::strcmp(e, "first") == 0) ? PLACE_FIRST : PLACE_LOAD;
}

// The engines that may share a table (the BLS12-381 engine uses the Ed25519 engine's entries when
// both have the same number of device objects): the load is one per device, the running totals
// are kept per engine.
constexpr int PLACE_ENGINES = 2;

struct PlaceEntry {
    uint64_t out_ranges = 0, out_items = 0;  // outstanding now, all engines
    uint64_t peak = 0;                       // the highest out_ranges seen
    uint64_t ranges[PLACE_ENGINES] = {0, 0}, items[PLACE_ENGINES] = {0, 0};  // running totals placed here
};

class PlaceTable {
  public:
    explicit PlaceTable(size_t ndev = 1, PlaceMode mode = PLACE_LOAD) : e_(ndev ? ndev : 1), mode_(mode) {}
    size_t size() const { return e_.size(); }
    PlaceMode mode() const { return mode_; }

    // A single-range call of `items` items: choose its device and count it there (one step).
    size_t pick(uint64_t items, int engine = 0) {
        std::lock_guard<std::mutex> g(mu_);
        size_t best = 0;
        if (mode_ == PLACE_LOAD)
            for (size_t i = 1; i < e_.size(); i++)
                if (e_[i].out_ranges < e_[best].out_ranges ||
                    (e_[i].out_ranges == e_[best].out_ranges && e_[i].out_items < e_[best].out_items))
                    best = i;
        add(best, items, engine);
        return best;
    }
    // Count one range of `items` items on a device that the caller names (ranges of a split call,
    // staged batches, calls that stay on device 0).
    void acquire(size_t dev, uint64_t items, int engine = 0) {
        std::lock_guard<std::mutex> g(mu_);
        add(dev, items, engine);
    }
    void release(size_t dev, uint64_t items) {
        std::lock_guard<std::mutex> g(mu_);
        PlaceEntry& e = e_[dev];
        e.out_ranges -= e.out_ranges ? 1 : 0;
        e.out_items -= e.out_items < items ? e.out_items : items;
    }
    // The first device of a call that splits into k > 1 ranges (range j: (base + j) mod ndev).
    size_t rotate_base() {
        std::lock_guard<std::mutex> g(mu_);
        return mode_ == PLACE_FIRST ? 0 : (size_t)(cursor_++ % e_.size());
    }
    PlaceEntry get(size_t dev) const {
        std::lock_guard<std::mutex> g(mu_);
        return e_[dev];
    }

  private:
    void add(size_t dev, uint64_t items, int engine) {
        PlaceEntry& e = e_[dev];
        e.out_ranges++;
        e.out_items += items;
        e.ranges[engine]++;
        e.items[engine] += items;
        if (e.out_ranges > e.peak) e.peak = e.out_ranges;
    }
    mutable std::mutex mu_;
    std::vector<PlaceEntry> e_;
    uint64_t cursor_ = 0;
    PlaceMode mode_;
};

// The hold of one range on its load entry; movable, released once.
class Ticket {
  public:
    Ticket() = default;
    // a single-range call, placed by the table
    Ticket(PlaceTable& t, uint64_t items, int engine = 0) : t_(&t), items_(items) { dev_ = t.pick(items, engine); }
    // a range on a named device
    Ticket(PlaceTable& t, size_t dev, uint64_t items, int engine) : t_(&t), dev_(dev), items_(items) {
        t.acquire(dev, items, engine);
    }
    Ticket(Ticket&& o) noexcept : t_(o.t_), dev_(o.dev_), items_(o.items_) { o.t_ = nullptr; }
    Ticket& operator=(Ticket&& o) noexcept {
        if (this != &o) {
            release();
            t_ = o.t_;
            dev_ = o.dev_;
            items_ = o.items_;
            o.t_ = nullptr;
        }
        return *this;
    }
    Ticket(const Ticket&) = delete;
    Ticket& operator=(const Ticket&) = delete;
    ~Ticket() { release(); }
    void release() {
        if (t_) t_->release(dev_, items_);
        t_ = nullptr;
    }
    bool held() const { return t_ != nullptr; }
    size_t dev() const { return dev_; }

  private:
    PlaceTable* t_ = nullptr;
    size_t dev_ = 0;
    uint64_t items_ = 0;
};

// The devices of a call's ranges, each with its ticket: a single range by load, k > 1 ranges
// rotated.  ranges[j] runs on out[j].dev().
inline std::vector<Ticket> place_ranges(PlaceTable& t, const std::vector<std::pair<size_t, size_t>>& ranges,
                                        int engine = 0) {
    std::vector<Ticket> out;
    out.reserve(ranges.size());
    if (ranges.size() == 1) {
        out.emplace_back(t, (uint64_t)(ranges[0].second - ranges[0].first), engine);
    } else if (ranges.size() > 1) {
        const size_t base = t.rotate_base();
        for (size_t j = 0; j < ranges.size(); j++)
            out.emplace_back(t, (base + j) % t.size(), (uint64_t)(ranges[j].second - ranges[j].first), engine);
    }
    return out;
}

}  // namespace nwv
