// The message ring's bookkeeping (narwhal_amd/csrc/bls_msg_ring.h) behind a C interface, with no
// HIP: tests/test_bls_msg_ring_host.py drives lookups, pins, reservations and publishes through it.
// Compiled with -DBLSMR_STUB_MAIN the file is a stand-alone program that runs the readers-against-
// writers loop (the form that test builds with -fsanitize=thread).
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../narwhal_amd/csrc/bls_msg_ring.h"

namespace {

using nwv::BlsMsgRing;
using nwv::MsgKey;

// Two threads look keys up, pin, read the slot's record and unpin, while two threads reserve a
// slot, write its record and publish it under a key.  rec[slot] stands for the device record: a
// plain word, written only between reserve and publish and read only under a pin, so a slot handed
// out while a reader holds it is a data race the thread sanitizer sees, and a reader that finds
// another key's value under its key is counted in out[1].  out[0] hits, [1] wrong values read,
// [2] publishes, [3] reservations that found no free slot.
void race(BlsMsgRing& r, int nkeys, int rounds, uint64_t out[4]) {
    std::vector<uint64_t> rec(r.cap(), 0);
    std::atomic<uint64_t> hits{0}, bad{0}, pubs{0}, none{0};
    std::atomic<int> writers_left{2};
    auto key = [](int k) {
        uint8_t m[32];
        for (int j = 0; j < 32; j++) m[j] = (uint8_t)(k * 7 + j);
        return MsgKey::make(reinterpret_cast<const uint8_t*>("dst"), 3, m, 32);
    };
    std::vector<std::thread> th;
    for (int t = 0; t < 2; t++)
        th.emplace_back([&, t]() {
            uint32_t x = 12345u + 977u * (uint32_t)t;
            while (writers_left.load() > 0) {
                x = x * 1664525u + 1013904223u;
                const int k = (int)((x >> 8) % (uint32_t)nkeys);
                const uint32_t s = r.lookup_pin(key(k));
                if (s == BlsMsgRing::NONE) continue;
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
                const int k = (int)((x >> 8) % (uint32_t)nkeys);
                const uint32_t s = r.reserve();
                if (s == BlsMsgRing::NONE) {
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

#ifndef BLSMR_STUB_MAIN
extern "C" {

void* bmr_new(uint32_t cap, int lg_buckets) {
    auto* r = new BlsMsgRing;
    r->init(cap, lg_buckets);
    return r;
}
void bmr_free(void* r) { delete static_cast<BlsMsgRing*>(r); }
int bmr_cacheable(uint64_t dst_len, uint64_t msg_len) { return MsgKey::cacheable(dst_len, msg_len) ? 1 : 0; }
// every operation takes the key as (dst, msg); the caller keeps within the limits (bmr_cacheable)
uint32_t bmr_lookup_pin(void* r, const uint8_t* dst, uint64_t dl, const uint8_t* msg, uint64_t ml) {
    return static_cast<BlsMsgRing*>(r)->lookup_pin(MsgKey::make(dst, dl, msg, ml));
}
int bmr_contains(void* r, const uint8_t* dst, uint64_t dl, const uint8_t* msg, uint64_t ml) {
    return static_cast<BlsMsgRing*>(r)->contains(MsgKey::make(dst, dl, msg, ml)) ? 1 : 0;
}
uint32_t bmr_reserve(void* r) { return static_cast<BlsMsgRing*>(r)->reserve(); }
uint32_t bmr_publish(void* r, uint32_t slot, const uint8_t* dst, uint64_t dl, const uint8_t* msg, uint64_t ml) {
    return static_cast<BlsMsgRing*>(r)->publish(slot, MsgKey::make(dst, dl, msg, ml));
}
void bmr_release(void* r, uint32_t slot) { static_cast<BlsMsgRing*>(r)->release(slot); }
void bmr_unpin(void* r, uint32_t slot) { static_cast<BlsMsgRing*>(r)->unpin(slot); }
void bmr_counts(void* r, uint64_t out[3]) { static_cast<BlsMsgRing*>(r)->counts(out); }
uint32_t bmr_slot_state(void* r, uint32_t slot) { return static_cast<BlsMsgRing*>(r)->slot_state(slot); }
uint64_t bmr_hash(const uint8_t* dst, uint64_t dl, const uint8_t* msg, uint64_t ml) {
    return MsgKey::make(dst, dl, msg, ml).hash();
}
void bmr_race(void* r, int nkeys, int rounds, uint64_t out[4]) { race(*static_cast<BlsMsgRing*>(r), nkeys, rounds, out); }

}  // extern "C"
#else
int main() {
    BlsMsgRing r;
    r.init(4);
    uint64_t out[4];
    race(r, 9, 20000, out);
    uint64_t c[3];
    r.counts(c);
    const bool ok = out[1] == 0 && out[2] > 0 && c[1] == 0 && c[2] == 0;
    std::printf("message ring: %llu hits, %llu wrong reads, %llu publishes, %llu full, busy %llu pinned %llu, %s\n",
                (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2],
                (unsigned long long)out[3], (unsigned long long)c[1], (unsigned long long)c[2], ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}
#endif
