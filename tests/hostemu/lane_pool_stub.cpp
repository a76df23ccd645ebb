// The lease rule of a device object's lane pools (narwhal_amd/csrc/lane_pool.h) behind a C
// interface, with no HIP: tests/test_lane_pool_host.py drives leases, returns, waiters and the
// counters through it.  A stub lane is a number (the order in which the pool opened it) and a use
// count.  Compiled with -DLANE_POOL_STUB_MAIN the file is a stand-alone program that runs the
// holders-against-waiters loop and checks the pool afterwards (the form that test builds with
// -fsanitize=thread).
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../narwhal_amd/csrc/lane_pool.h"

namespace {

struct StubLane {
    int id = -1;
    bool reserved = false;
    int users = 0;       // plain on purpose: two holders of one lane are a data race
    uint64_t leases = 0;
};

struct Pool {
    nwv::LanePool<StubLane> pool;
    std::vector<std::unique_ptr<StubLane>> made;  // by id; appended under the pool's mutex (open)
    int fail_next = 0;                            // the next open() fails (returns null)
    StubLane* open(bool reserved) {
        if (fail_next) {
            fail_next--;
            return nullptr;
        }
        made.emplace_back(new StubLane);
        made.back()->id = (int)made.size() - 1;
        made.back()->reserved = reserved;
        return made.back().get();
    }
    StubLane* lease(bool latency) {
        return pool.lease(latency, [&](bool r) { return open(r); });
    }
};

// a lease taken on a thread of its own (it may block): done once it holds a lane
struct Waiter {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    int lane = -1;
};

// `threads` host threads, each `iters` leases; thread k is latency class when k is odd.  Every
// lease checks that it is the lane's only user.  Returns the leases made, 0 on a double lease.
uint64_t hammer(Pool& p, int threads, int iters) {
    std::atomic<uint64_t> total{0};
    std::atomic<int> bad{0};
    std::vector<std::thread> th;
    for (int k = 0; k < threads; k++)
        th.emplace_back([&, k]() {
            for (int i = 0; i < iters; i++) {
                StubLane* l = p.lease((k & 1) != 0);
                if (!l || ++l->users != 1 || (l->reserved && !(k & 1))) bad++;
                if (l) {
                    l->leases++;
                    if (i % 64 == 0) std::this_thread::yield();
                    --l->users;
                    p.pool.give_back(l);
                }
                total++;
            }
        });
    for (auto& x : th) x.join();
    return bad.load() ? 0 : total.load();
}

}  // namespace

#ifndef LANE_POOL_STUB_MAIN
extern "C" {

void* lp_new(uint64_t ordinary_cap, uint64_t reserved_cap) {
    auto* p = new Pool;
    p->pool.set_caps((size_t)ordinary_cap, (size_t)reserved_cap);
    return p;
}
void lp_free(void* p) { delete static_cast<Pool*>(p); }
void lp_fail_next_open(void* p, int n) { static_cast<Pool*>(p)->fail_next = n; }

// the lane's id, -1 where lease() would wait, -2 where open() failed; *reserved: of the reserved pool
int lp_try_lease(void* h, int latency, int* reserved) {
    Pool& p = *static_cast<Pool*>(h);
    bool res = false, wait = false;
    StubLane* l = p.pool.try_lease(latency != 0, [&](bool r) { return p.open(r); }, &res, &wait);
    if (reserved) *reserved = res ? 1 : 0;
    return l ? l->id : (wait ? -1 : -2);
}
void lp_release(void* h, int id) {
    Pool& p = *static_cast<Pool*>(h);
    p.pool.give_back(p.made[(size_t)id].get());
}
void lp_counters(void* h, uint64_t out[8]) { static_cast<Pool*>(h)->pool.counters(out); }
uint64_t lp_idle(void* h) { return static_cast<Pool*>(h)->pool.idle_count(); }
uint64_t lp_lanes(void* h) { return static_cast<Pool*>(h)->pool.all().size(); }
int lp_first_reserved(void* h) {
    const StubLane* l = static_cast<Pool*>(h)->pool.first_reserved();
    return l ? l->id : -1;
}

// a blocking lease on its own thread
void* lp_lease_async(void* h, int latency) {
    auto* w = new Waiter;
    Pool* p = static_cast<Pool*>(h);
    w->th = std::thread([w, p, latency]() {
        StubLane* l = p->lease(latency != 0);
        std::lock_guard<std::mutex> g(w->mu);
        w->lane = l ? l->id : -2;
        w->done = true;
        w->cv.notify_all();
    });
    return w;
}
// 1 and *lane once the waiter holds a lane (waits up to timeout_ms for it), else 0
int lp_waiter_wait(void* wv, int timeout_ms, int* lane) {
    auto* w = static_cast<Waiter*>(wv);
    std::unique_lock<std::mutex> g(w->mu);
    w->cv.wait_for(g, std::chrono::milliseconds(timeout_ms), [&] { return w->done; });
    if (w->done && lane) *lane = w->lane;
    return w->done ? 1 : 0;
}
// (the waiter must have finished: join and free)
void lp_waiter_free(void* wv) {
    auto* w = static_cast<Waiter*>(wv);
    w->th.join();
    delete w;
}

uint64_t lp_hammer(void* h, int threads, int iters) { return hammer(*static_cast<Pool*>(h), threads, iters); }
uint64_t lp_lane_leases(void* h, int id) { return static_cast<Pool*>(h)->made[(size_t)id]->leases; }

uint64_t lp_env_lanes(void) { return nwv::latency_lanes_from_env(); }
uint64_t lp_env_digest_bytes(void) { return nwv::latency_digest_bytes_from_env(); }
int lp_env_priority(void) { return nwv::latency_priority_from_env() ? 1 : 0; }
uint64_t lp_clamp(uint64_t n, uint64_t shard_min) { return nwv::latency_clamp((size_t)n, (size_t)shard_min); }

}  // extern "C"
#else
int main() {
    const int threads = 8, iters = 4000;
    Pool p;
    p.pool.set_caps(2, 1);  // 3 lanes for 8 threads: most leases wait
    const uint64_t leases = hammer(p, threads, iters);
    uint64_t c[nwv::QOS_COUNTERS];
    p.pool.counters(c);
    uint64_t per_lane = 0;
    for (auto& l : p.made) per_lane += l->leases;
    bool ok = leases == (uint64_t)threads * iters && per_lane == leases;
    ok = ok && c[0] + c[3] == leases && c[0] == leases / 2 && c[1] <= c[0] && c[2] <= c[0] && c[4] <= c[3];
    ok = ok && c[5] == 1 && c[6] == 1 && c[7] >= 1 && c[7] <= 2 && p.pool.idle_count() == c[5] + c[7];
    std::printf("lane pool hammer: %llu leases, %s\n", (unsigned long long)leases, ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}
#endif
