// The key cache's bookkeeping (narwhal_amd/csrc/keycache_alloc.h) behind a C interface, with no
// HIP: tests/test_keycache_alloc_host.py drives the key -> slot map, the free lists, the pins, the
// registered-list fingerprint and the hold through it.  Compiled with -DKCALLOC_STUB_MAIN the file
// is a stand-alone program that runs the holders-against-a-retainer loop (the form that test
// builds with -fsanitize=thread).
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../narwhal_amd/csrc/keycache_alloc.h"

namespace {

struct Cache {
    nwv::KeyAlloc a;
    nwv::KeyHold hold;
};

nwv::Key32 key_of(const uint8_t* k) {
    nwv::Key32 r;
    std::memcpy(r.b, k, 32);
    return r;
}

// `holders` threads take and release the hold shared in a loop, overlapping one another, while one
// thread takes it exclusive `retains` times (retiring everything each time, as an epoch change
// does).  inside: bumped by a holder on entry, dropped on exit; it must read 0 whenever the
// retainer is in.  epoch: a plain word that holders read and the retainer writes, so a hold that
// excludes nothing is a data race the thread sanitizer sees.  out[0] retains done, [1] times the
// retainer saw a holder inside, [2] holds taken in all, [3] holds taken while a retain was still
// to come (the callers really did overlap it: the retainer lets at least one hold pass between
// two retains, so this is at least retains - 1).
void race(Cache& c, int holders, int retains, uint64_t out[4]) {
    std::atomic<int> inside{0};
    std::atomic<bool> done{false};
    std::atomic<uint64_t> holds{0}, holds_during{0};
    uint64_t epoch = 0, sink = 0;
    std::vector<std::thread> th;
    std::vector<uint64_t> seen(holders, 0);
    for (int k = 0; k < holders; k++)
        th.emplace_back([&, k]() {
            while (!done.load()) {
                c.hold.lock_shared();
                inside++;
                seen[k] += epoch;
                for (int spin = 0; spin < 50; spin++) std::this_thread::yield();  // the call's kernels run
                inside--;
                c.hold.unlock_shared();
                holds++;
                if (!done.load()) holds_during++;
            }
        });
    uint64_t bad = 0, did = 0;
    for (int r = 0; r < retains; r++) {
        // (an epoch lasts: callers get in between two retains, so every retain meets fresh holders)
        for (const uint64_t last = holds.load(); holds.load() == last;) std::this_thread::yield();
        c.hold.lock();
        if (inside.load() != 0) bad++;
        epoch++;
        uint64_t o[3];
        c.a.retain(nullptr, 0, o);
        if (inside.load() != 0) bad++;
        c.hold.unlock();
        did++;
    }
    done = true;
    for (auto& x : th) x.join();
    for (uint64_t s : seen) sink += s;
    out[0] = did;
    out[1] = bad;
    out[2] = holds.load();
    out[3] = holds_during.load();
    if (sink > (uint64_t)retains * holds.load()) out[1]++;  // (an epoch read above the last one written)
}

}  // namespace

#ifndef KCALLOC_STUB_MAIN
extern "C" {

void* kca_new(uint32_t slots, uint32_t tables) {
    auto* c = new Cache;
    c->a.init_slots(slots);
    if (tables) c->a.init_tables(tables);
    return c;
}
void kca_free(void* c) { delete static_cast<Cache*>(c); }

// the key's slot, or UINT32_MAX
uint32_t kca_find(void* c, const uint8_t* key) { return static_cast<Cache*>(c)->a.find(key_of(key)); }
// What a keyed call does with a key: the slot it has, else a taken slot published at once (the
// record fill is the device's part); UINT32_MAX when the table is full.
uint32_t kca_assign(void* c, const uint8_t* key) {
    nwv::KeyAlloc& a = static_cast<Cache*>(c)->a;
    const nwv::Key32 k = key_of(key);
    uint32_t s = a.find(k);
    if (s != nwv::KeyAlloc::NONE) return s;
    s = a.take_slot();
    if (s != nwv::KeyAlloc::NONE) a.publish(k, s);
    return s;
}
// a slot taken and given back unpublished (a call that goes uncached after all)
uint32_t kca_take_and_give_back(void* c) {
    nwv::KeyAlloc& a = static_cast<Cache*>(c)->a;
    const uint32_t s = a.take_slot();
    if (s != nwv::KeyAlloc::NONE) a.give_back_slot(s);
    return s;
}
// What a registration does with a cached key: the table it has, else a taken table set at once;
// UINT32_MAX when the key is not cached or no table is left.
uint32_t kca_assign_table(void* c, const uint8_t* key) {
    nwv::KeyAlloc& a = static_cast<Cache*>(c)->a;
    const uint32_t s = a.find(key_of(key));
    if (s == nwv::KeyAlloc::NONE) return nwv::KeyAlloc::NONE;
    uint32_t t = a.table_of(s);
    if (t != nwv::KeyAlloc::NONE) return t;
    t = a.take_table();
    if (t != nwv::KeyAlloc::NONE) a.set_table(s, t);
    return t;
}
uint32_t kca_table_of(void* c, uint32_t slot) { return static_cast<Cache*>(c)->a.table_of(slot); }
void kca_pin(void* c, uint32_t slot) { static_cast<Cache*>(c)->a.pin(slot); }
void kca_unpin(void* c, uint32_t slot) { static_cast<Cache*>(c)->a.unpin(slot); }
uint32_t kca_pins(void* c, uint32_t slot) { return static_cast<Cache*>(c)->a.pins(slot); }
void kca_retain(void* c, const uint8_t* keys, uint64_t n, uint64_t out[3]) {
    Cache* k = static_cast<Cache*>(c);
    k->hold.lock();
    k->a.retain(keys, (size_t)n, out);
    k->hold.unlock();
}
// the fingerprint of a fully registered list, stored with the slots its keys have now
void kca_set_registered(void* c, uint64_t fp, const uint8_t* keys, uint64_t n) {
    nwv::KeyAlloc& a = static_cast<Cache*>(c)->a;
    std::vector<uint32_t> s;
    for (uint64_t j = 0; j < n; j++) s.push_back(a.find(key_of(keys + 32 * j)));
    a.set_registered(fp, s.data(), s.size());
}
uint64_t kca_reg_fp(void* c) { return static_cast<Cache*>(c)->a.reg_fp(); }
// out[0] live slots (slot 0 included), [1] live tables, [2] slot high-water mark, [3] table
// high-water mark
void kca_counts(void* c, uint64_t out[4]) {
    const nwv::KeyAlloc& a = static_cast<Cache*>(c)->a;
    out[0] = a.slots_live();
    out[1] = a.tables_live();
    out[2] = a.slot_high_water();
    out[3] = a.table_high_water();
}
void kca_hold_shared(void* c) { static_cast<Cache*>(c)->hold.lock_shared(); }
void kca_release_shared(void* c) { static_cast<Cache*>(c)->hold.unlock_shared(); }
void kca_race(void* c, int holders, int retains, uint64_t out[4]) { race(*static_cast<Cache*>(c), holders, retains, out); }

}  // extern "C"
#else
int main() {
    Cache c;
    c.a.init_slots(8);
    c.a.init_tables(4);
    uint64_t out[4];
    race(c, 4, 1000, out);
    const bool ok = out[0] == 1000 && out[1] == 0 && out[2] > 0;
    std::printf("keycache hold: %llu retains, %llu holds (%llu before the last retain), %llu overlaps seen, %s\n",
                (unsigned long long)out[0], (unsigned long long)out[2], (unsigned long long)out[3],
                (unsigned long long)out[1], ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}
#endif
