// lane_pool.h -- which lane of a device object a call leases (host code, no HIP).
//
// Every call holds one lane (a stream with its staging and scratch buffers) of its device object
// for its whole duration.  A device object has two pools:
//
//   ordinary   up to `ordinary_cap` lanes (NWV_LANES for the Ed25519 / BLAKE2b engine, 8 for the
//              BLS12-381 engine), opened on demand: what every call used before there were classes
//   reserved   up to `reserved_cap` lanes (NWV_LATENCY_LANES, default 2, 1..4), opened on demand
//              and only by latency-class calls; the engines create their streams at the device's
//              greatest priority
//
// A call is latency class when its engine's bound (nwv_set_latency_max) is non-zero and the call
// fits it; the engines decide that, the pool only takes the answer.  With the bound at 0 no call
// is latency class, no reserved lane is ever opened, and lease() is the loop the engines had:
// the most recently returned idle lane, else a new lane below the cap, else wait.
//
// A latency-class call takes, in order: an idle reserved lane, a new reserved lane below the cap,
// an idle ordinary lane, a new ordinary lane below the cap; otherwise it waits for the first lane
// of either pool.  Any other call uses the ordinary pool only: it never gets a reserved lane and is
// never woken for one.
//
// Wake-ups: the two classes wait on condition variables of their own.  A returned reserved lane
// signals one latency waiter; a returned ordinary lane signals one waiter of each class that has
// any (the one that finds the lane gone waits again).  So an idle lane and a waiter that may use
// it never coexist without a signal on its way to such a waiter.
//
// The lanes are opened by the caller's `open(reserved)` under the pool's mutex, as the engines did
// before: two callers never open a lane past a cap.  The pool never closes a lane; the engine
// closes all() when the context is freed.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <vector>

namespace nwv {

constexpr size_t LATENCY_LANES_DEFAULT = 2, LATENCY_LANES_MAX = 4;
constexpr size_t LATENCY_DIGEST_BYTES_DEFAULT = (size_t)1 << 20;
constexpr int QOS_COUNTERS = 8;

// NWV_LATENCY_LANES as read at nwv_init: the reserved lanes a device object may open, 1..4
inline size_t latency_lanes_from_env() {
    const char* e = std::getenv("NWV_LATENCY_LANES");
    if (!e || !*e) return LATENCY_LANES_DEFAULT;
    const long v = std::strtol(e, nullptr, 10);
    return (size_t)std::min<long>((long)LATENCY_LANES_MAX, std::max<long>(1, v));
}
// NWV_LATENCY_DIGEST_BYTES as read at nwv_init: a latency-class digest call's input bytes at most
inline size_t latency_digest_bytes_from_env() {
    const char* e = std::getenv("NWV_LATENCY_DIGEST_BYTES");
    if (!e || !*e) return LATENCY_DIGEST_BYTES_DEFAULT;
    return (size_t)std::strtoull(e, nullptr, 10);
}
// NWV_LATENCY_PRIORITY=0 (read at nwv_init) gives reserved lanes default-priority streams: the A/B
// switch that separates what the reservation buys from what the priority buys
inline bool latency_priority_from_env() {
    const char* e = std::getenv("NWV_LATENCY_PRIORITY");
    return !(e && e[0] == '0' && e[1] == 0);
}
// the bound in force for a requested bound n: below the engine's shard minimum, so a latency-class
// call is always a single range
inline size_t latency_clamp(size_t n, size_t shard_min) {
    return shard_min == 0 ? 0 : std::min<size_t>(n, shard_min - 1);
}

template <class L>
class LanePool {
  public:
    // set once, before the first lease
    void set_caps(size_t ordinary_cap, size_t reserved_cap) {
        std::lock_guard<std::mutex> g(mu_);
        ord_cap_ = ordinary_cap ? ordinary_cap : 1;
        res_cap_ = std::min<size_t>(reserved_cap, LATENCY_LANES_MAX);
    }
    // an ordinary lane opened outside lease() (the one a device object opens at init) joins idle
    void adopt(L* lane) {
        std::lock_guard<std::mutex> g(mu_);
        ord_.push_back(lane);
        idle_ord_.push_back(lane);
    }

    // The call's lane; blocks while no lane it may use is idle and none may be opened.  open(reserved)
    // returns the new lane or null (the lease then fails: null, and the call is not counted).
    // *reserved (optional): the lane is of the reserved pool.
    template <class Open>
    L* lease(bool latency, Open&& open, bool* reserved = nullptr) {
        std::unique_lock<std::mutex> lk(mu_);
        bool waited = false, failed = false, res = false;
        L* lane;
        while (!(lane = choose(latency, open, &res, &failed)) && !failed) {
            waited = true;
            if (latency) {
                lat_waiters_++;
                cv_lat_.wait(lk);
                lat_waiters_--;
            } else {
                ord_waiters_++;
                cv_ord_.wait(lk);
                ord_waiters_--;
            }
        }
        if (lane) count(latency, res, waited);
        if (reserved) *reserved = res;
        return lane;
    }
    // lease() for a caller that must not block: null with *would_wait set where lease() would wait
    template <class Open>
    L* try_lease(bool latency, Open&& open, bool* reserved = nullptr, bool* would_wait = nullptr) {
        std::lock_guard<std::mutex> g(mu_);
        bool failed = false, res = false;
        L* lane = choose(latency, open, &res, &failed);
        if (lane) count(latency, res, false);
        if (reserved) *reserved = res;
        if (would_wait) *would_wait = !lane && !failed;
        return lane;
    }
    void give_back(L* lane) {
        bool wake_lat, wake_ord = false;
        {
            std::lock_guard<std::mutex> g(mu_);
            if (std::find(res_.begin(), res_.end(), lane) != res_.end()) {
                idle_res_.push_back(lane);
            } else {
                idle_ord_.push_back(lane);
                wake_ord = ord_waiters_ > 0;
            }
            wake_lat = lat_waiters_ > 0;
        }
        if (wake_lat) cv_lat_.notify_one();
        if (wake_ord) cv_ord_.notify_one();
    }

    // [0] latency-class calls, [1] of those on a reserved lane, [2] of those that waited, [3] all
    // other calls, [4] of those that waited, [5] reserved lanes open, [6] reserved-lane cap,
    // [7] ordinary lanes open
    void counters(uint64_t out[QOS_COUNTERS]) const {
        std::lock_guard<std::mutex> g(mu_);
        for (int k = 0; k < 5; k++) out[k] = n_[k];
        out[5] = res_.size();
        out[6] = res_cap_;
        out[7] = ord_.size();
    }
    size_t idle_count() const {
        std::lock_guard<std::mutex> g(mu_);
        return idle_ord_.size() + idle_res_.size();
    }
    // the first reserved lane opened, or null
    L* first_reserved() const {
        std::lock_guard<std::mutex> g(mu_);
        return res_.empty() ? nullptr : res_.front();
    }
    // every lane ever opened, ordinary ones first (for the engine to close; no lease may be out)
    std::vector<L*> all() const {
        std::lock_guard<std::mutex> g(mu_);
        std::vector<L*> v(ord_);
        v.insert(v.end(), res_.begin(), res_.end());
        return v;
    }
    void clear() {
        std::lock_guard<std::mutex> g(mu_);
        ord_.clear();
        res_.clear();
        idle_ord_.clear();
        idle_res_.clear();
    }

  private:
    // one pass of the rule under mu_: a lane, or null (wait, or *failed: open() returned null)
    template <class Open>
    L* choose(bool latency, Open& open, bool* reserved, bool* failed) {
        *reserved = false;
        if (latency) {
            if (!idle_res_.empty()) {
                *reserved = true;
                return pop(idle_res_);
            }
            if (res_.size() < res_cap_) {
                L* l = open(true);
                if (!l) {
                    *failed = true;
                    return nullptr;
                }
                res_.push_back(l);
                *reserved = true;
                return l;
            }
        }
        if (!idle_ord_.empty()) return pop(idle_ord_);
        if (ord_.size() < ord_cap_) {
            L* l = open(false);
            if (!l) {
                *failed = true;
                return nullptr;
            }
            ord_.push_back(l);
            return l;
        }
        return nullptr;
    }
    static L* pop(std::vector<L*>& v) {
        L* l = v.back();
        v.pop_back();
        return l;
    }
    void count(bool latency, bool reserved, bool waited) {
        if (latency) {
            n_[0]++;
            n_[1] += reserved ? 1 : 0;
            n_[2] += waited ? 1 : 0;
        } else {
            n_[3]++;
            n_[4] += waited ? 1 : 0;
        }
    }

    mutable std::mutex mu_;
    std::condition_variable cv_ord_, cv_lat_;
    size_t ord_waiters_ = 0, lat_waiters_ = 0;
    std::vector<L*> ord_, res_, idle_ord_, idle_res_;
    size_t ord_cap_ = 1, res_cap_ = LATENCY_LANES_DEFAULT;
    uint64_t n_[5] = {0, 0, 0, 0, 0};
};

}  // namespace nwv
