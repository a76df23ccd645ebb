// The aggregate-key ring's bookkeeping (narwhal_amd/csrc/bls_apk_ring.h) behind a C interface, with
// no HIP: tests/test_bls_apk_ring_host.py drives lookups, pins, the second-sighting filter,
// reservations, publishes and resets through it.  Compiled with -DBLSAR_STUB_MAIN the file is a
// stand-alone program that runs the readers-against-writers loop (the form that test builds with
// -fsanitize=thread).
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../narwhal_amd/csrc/bls_apk_ring.h"

namespace {

using nwv::ApkKey;
using nwv::BlsApkRing;

// Two threads look sets up, pin, read the slot's record and unpin, while two threads take a set
// through miss() (noted first, reserved at the next sighting), write the slot's record and publish
// it.  rec[slot] stands for the device record: a plain word, written only between reserve and
// publish and read only under a pin, so a slot handed out while a reader holds it is a data race
// the thread sanitizer sees, and a reader that finds another set's value under its set is counted
// in out[1].  out[0] hits, [1] wrong values read, [2] publishes, [3] misses that got no slot.
void race(BlsApkRing& r, int nsets, int rounds, uint64_t out[4]) {
    std::vector<uint64_t> rec(r.cap(), 0);
    std::atomic<uint64_t> hits{0}, bad{0}, pubs{0}, none{0};
    std::atomic<int> writers_left{2};
    auto key = [](int k) {
        const uint32_t v[3] = {(uint32_t)k + 2, (uint32_t)k, (uint32_t)(3 * k + 1)};  // (unsorted: make sorts)
        return ApkKey::make(v, 3);
    };
    std::vector<std::thread> th;
    for (int t = 0; t < 2; t++)
        th.emplace_back([&, t]() {
            uint32_t x = 12345u + 977u * (uint32_t)t;
            while (writers_left.load() > 0) {
                x = x * 1664525u + 1013904223u;
                const int k = (int)((x >> 8) % (uint32_t)nsets);
                const uint32_t s = r.lookup_pin(key(k));
                if (s == BlsApkRing::NONE) continue;
                if (rec[s] != (uint64_t)k + 1) bad++;
                for (int spin = 0; spin < 20; spin++) std::this_thread::yield();  // the call's kernels run
                if (rec[s] != (uint64_t)k + 1) bad++;
                r.unpin(s);
                hits++;
            }
        });
    for (int t = 0; t < 2; t++)
        th.emplace_back([&, t]() {
            uint32_t x = 99991u + 31u * (uint32_t)t;
            for (int i = 0; i < rounds; i++) {
                x = x * 1664525u + 1013904223u;
                const int k = (int)((x >> 8) % (uint32_t)nsets);
                bool noted;
                const uint32_t s = r.miss(key(k), &noted);
                if (s == BlsApkRing::NONE) {
                    none++;
                    std::this_thread::yield();
                    continue;
                }
                rec[s] = (uint64_t)k + 1;  // the kernel fills the record
                std::this_thread::yield();
                r.publish(s, key(k));
                pubs++;
            }
            writers_left--;
        });
    for (auto& x : th) x.join();
    out[0] = hits.load();
    out[1] = bad.load();
    out[2] = pubs.load();
    out[3] = none.load();
}

}  // namespace

#ifndef BLSAR_STUB_MAIN
extern "C" {

void* bar_new(uint32_t cap, int lg_buckets) {
    auto* r = new BlsApkRing;
    r->init(cap, lg_buckets);
    return r;
}
void bar_free(void* r) { delete static_cast<BlsApkRing*>(r); }
int bar_eligible(uint64_t cnt) { return ApkKey::eligible(cnt) ? 1 : 0; }
// every operation takes the set as an index list in any order; the caller keeps within the limits
uint32_t bar_lookup_pin(void* r, const uint32_t* idx, uint64_t n) {
    return static_cast<BlsApkRing*>(r)->lookup_pin(ApkKey::make(idx, n));
}
int bar_contains(void* r, const uint32_t* idx, uint64_t n) {
    return static_cast<BlsApkRing*>(r)->contains(ApkKey::make(idx, n)) ? 1 : 0;
}
uint32_t bar_miss(void* r, const uint32_t* idx, uint64_t n, int* noted) {
    bool nt = false;
    const uint32_t s = static_cast<BlsApkRing*>(r)->miss(ApkKey::make(idx, n), &nt);
    *noted = nt ? 1 : 0;
    return s;
}
uint32_t bar_reserve(void* r) { return static_cast<BlsApkRing*>(r)->reserve(); }
uint32_t bar_publish(void* r, uint32_t slot, const uint32_t* idx, uint64_t n) {
    return static_cast<BlsApkRing*>(r)->publish(slot, ApkKey::make(idx, n));
}
void bar_release(void* r, uint32_t slot) { static_cast<BlsApkRing*>(r)->release(slot); }
void bar_unpin(void* r, uint32_t slot) { static_cast<BlsApkRing*>(r)->unpin(slot); }
void bar_reset(void* r) { static_cast<BlsApkRing*>(r)->reset(); }
void bar_counts(void* r, uint64_t out[3]) { static_cast<BlsApkRing*>(r)->counts(out); }
uint32_t bar_slot_state(void* r, uint32_t slot) { return static_cast<BlsApkRing*>(r)->slot_state(slot); }
uint64_t bar_filter_used(void* r) { return static_cast<BlsApkRing*>(r)->filter_used(); }
uint64_t bar_hash(const uint32_t* idx, uint64_t n) { return ApkKey::make(idx, n).h; }
uint64_t bar_filter_entry(void* r, const uint32_t* idx, uint64_t n) {
    return static_cast<BlsApkRing*>(r)->filter_entry(ApkKey::make(idx, n).h);
}
void bar_race(void* r, int nsets, int rounds, uint64_t out[4]) { race(*static_cast<BlsApkRing*>(r), nsets, rounds, out); }

}  // extern "C"
#else
int main() {
    BlsApkRing r;
    r.init(4);
    uint64_t out[4];
    race(r, 9, 20000, out);
    uint64_t c[3];
    r.counts(c);
    const bool ok = out[1] == 0 && out[2] > 0 && c[1] == 0 && c[2] == 0;
    std::printf("aggregate-key ring: %llu hits, %llu wrong reads, %llu publishes, %llu without a slot, busy %llu pinned %llu, %s\n",
                (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2],
                (unsigned long long)out[3], (unsigned long long)c[1], (unsigned long long)c[2], ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}
#endif
