// keycache_alloc.h -- which slot and which comb table a cached Ed25519 key has (host code, no HIP).
//
// The device buffers of a key cache (65,536 point records, NWV_COMB_KEYS comb tables) are
// allocated once and never move; this header decides which index of them a key gets, and when an
// index may be given to another key.  Reusing an index is a verification-key swap if anything
// still reads the old one, so three things guard it:
//
//   KeyHold   every call that obtained indices holds the cache shared until its kernels have
//             finished; retain (and the filling part of a registration) holds it exclusive.  A
//             pending exclusive holder stops new shared holders, so a retain completes under
//             continuous overlapping callers.
//   pins      a staged batch replays a captured graph that reads its slot indices from its own
//             device buffer for as long as it lives: it pins its slots, and retain leaves a
//             pinned slot (and its table) alone.
//   order     a slot or table taken from a free list is unpublished: the caller fills it on the
//             device, waits, and only then publishes the key (publish / set_table).
//
// KeyAlloc is not synchronised; its owner (KeyCache::mu) serialises it.  KeyHold is.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <random>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace nwv {

struct Key32 {
    uint8_t b[32];
    bool operator==(const Key32& o) const { return std::memcmp(b, o.b, 32) == 0; }
};
// All 32 key bytes, mixed with a per-process random seed: keys chosen to collide in the map
// would otherwise make every lookup under the cache lock linear.
struct Key32Hash {
    size_t operator()(const Key32& k) const {
        static const uint64_t seed = [] {
            std::random_device rd;
            return ((uint64_t)rd() << 32) ^ rd() ^ 0x9E3779B97F4A7C15ull;
        }();
        uint64_t h = seed;
        for (int i = 0; i < 4; i++) {
            uint64_t w;
            std::memcpy(&w, k.b + 8 * i, 8);
            h = (h ^ w) * 0xFF51AFD7ED558CCDull;
            h ^= h >> 32;
        }
        return (size_t)h;
    }
};

// Shared / exclusive hold with preference for the exclusive side: once an exclusive holder
// waits, new shared holders wait behind it (the ones already in finish first).
//
// The shared side is on every keyed call, so it is one atomic add to take and one to release
// while no exclusive holder is about: state_ counts the shared holders in its low bits and has
// EXCL set from the moment an exclusive holder starts to wait until it releases.  The mutex and
// the condition variable are touched only when EXCL is (or was just) set.
class KeyHold {
  public:
    void lock_shared() {
        for (;;) {
            if (!(state_.fetch_add(1, std::memory_order_acquire) & EXCL)) return;
            // an exclusive holder waits or is in: step back out (it may be waiting for us) and
            // wait for it to finish
            drop_shared();
            std::unique_lock<std::mutex> lk(mu_);
            while (state_.load(std::memory_order_acquire) & EXCL) cv_.wait(lk);
        }
    }
    void unlock_shared() { drop_shared(); }
    void lock() {
        std::unique_lock<std::mutex> lk(mu_);
        while (state_.load(std::memory_order_acquire) & EXCL) cv_.wait(lk);  // one exclusive holder at a time
        state_.fetch_or(EXCL, std::memory_order_acq_rel);  // from here on new shared holders wait
        while (state_.load(std::memory_order_acquire) & ~EXCL) cv_.wait(lk);  // the ones already in drain
    }
    void unlock() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            state_.fetch_and(~EXCL, std::memory_order_release);
        }
        cv_.notify_all();
    }

  private:
    static constexpr uint32_t EXCL = 1u << 31;
    // the last shared holder out wakes a waiting exclusive holder (under the mutex, so the wake-up
    // cannot fall between its check of the count and its wait)
    void drop_shared() {
        if (state_.fetch_sub(1, std::memory_order_release) == (EXCL | 1u)) {
            std::lock_guard<std::mutex> lk(mu_);
            cv_.notify_all();
        }
    }
    std::atomic<uint32_t> state_{0};
    std::mutex mu_;
    std::condition_variable cv_;
};

class KeyAlloc {
  public:
    static constexpr uint32_t NONE = UINT32_MAX;

    // slot 0 is the basepoint's: never handed out, never freed
    void init_slots(uint32_t cap) {
        slot_cap_ = cap;
        slot_hw_ = cap ? 1 : 0;
        pins_.assign(cap, 0);
        if (table_cap_) comb_of_.resize(cap, NONE);
    }
    void init_tables(uint32_t cap) {
        table_cap_ = cap;
        table_hw_ = 0;
        comb_of_.assign(slot_cap_ ? slot_cap_ : (1u << 16), NONE);
    }
    uint32_t slot_cap() const { return slot_cap_; }
    uint32_t table_cap() const { return table_cap_; }
    // live counts (slot 0 included; a slot or table taken and not yet published counts)
    uint32_t slots_live() const { return slot_hw_ - (uint32_t)free_slots_.size(); }
    uint32_t tables_live() const { return table_hw_ - (uint32_t)free_tables_.size(); }
    uint32_t slot_high_water() const { return slot_hw_; }
    uint32_t table_high_water() const { return table_hw_; }
    bool slot_available() const { return !free_slots_.empty() || slot_hw_ < slot_cap_; }
    bool table_available() const { return !free_tables_.empty() || table_hw_ < table_cap_; }

    uint32_t find(const Key32& k) const {
        auto it = slot_.find(k);
        return it == slot_.end() ? NONE : it->second;
    }
    // An unpublished slot: a freed one first, else the next never-used one; NONE when full.
    uint32_t take_slot() {
        if (!free_slots_.empty()) {
            const uint32_t s = free_slots_.back();
            free_slots_.pop_back();
            return s;
        }
        return slot_hw_ < slot_cap_ ? slot_hw_++ : NONE;
    }
    // a taken slot that was not published after all
    void give_back_slot(uint32_t s) {
        if (s && s < slot_hw_) free_slots_.push_back(s);
    }
    // the slot's record is written: the key is now found
    void publish(const Key32& k, uint32_t s) { slot_.emplace(k, s); }

    uint32_t take_table() {
        if (!free_tables_.empty()) {
            const uint32_t t = free_tables_.back();
            free_tables_.pop_back();
            return t;
        }
        return table_hw_ < table_cap_ ? table_hw_++ : NONE;
    }
    void give_back_table(uint32_t t) {
        if (t < table_hw_) free_tables_.push_back(t);
    }
    // the table is written: batches by the slot's key may use it
    void set_table(uint32_t s, uint32_t t) {
        if (s < comb_of_.size()) comb_of_[s] = t;
    }
    uint32_t table_of(uint32_t s) const { return s < comb_of_.size() ? comb_of_[s] : NONE; }

    void pin(uint32_t s) {
        if (s && s < pins_.size()) pins_[s]++;
    }
    void unpin(uint32_t s) {
        if (s && s < pins_.size() && pins_[s]) pins_[s]--;
    }
    uint32_t pins(uint32_t s) const { return s < pins_.size() ? pins_[s] : 0; }

    // the last key list registered with every key combed: its fingerprint and its slots
    uint64_t reg_fp() const { return reg_fp_; }
    void set_registered(uint64_t fp, const uint32_t* slots, size_t n) {
        reg_fp_ = fp;
        reg_slots_.clear();
        reg_slots_.insert(slots, slots + n);
    }

    // Retire every published key that is not among the n keys at keep (n x 32) and whose slot is
    // not pinned: the slot and its table go to the free lists.  out[0] slots retired, out[1]
    // tables retired, out[2] slots kept only because they are pinned.  The caller holds the
    // cache exclusive.
    void retain(const uint8_t* keep, size_t n, uint64_t out[3]) {
        out[0] = out[1] = out[2] = 0;
        std::unordered_set<Key32, Key32Hash> keepset;
        keepset.reserve(n);
        for (size_t j = 0; j < n; j++) {
            Key32 k;
            std::memcpy(k.b, keep + 32 * j, 32);
            keepset.insert(k);
        }
        bool reg_hit = false;
        for (auto it = slot_.begin(); it != slot_.end();) {
            const uint32_t s = it->second;
            if (keepset.count(it->first)) {
                ++it;
                continue;
            }
            if (pins(s)) {
                out[2]++;
                ++it;
                continue;
            }
            const uint32_t t = table_of(s);
            if (t != NONE) {
                comb_of_[s] = NONE;
                free_tables_.push_back(t);
                out[1]++;
            }
            free_slots_.push_back(s);
            out[0]++;
            reg_hit = reg_hit || reg_slots_.count(s);
            it = slot_.erase(it);
        }
        if (reg_hit) {
            reg_fp_ = 0;
            reg_slots_.clear();
        }
    }

  private:
    std::unordered_map<Key32, uint32_t, Key32Hash> slot_;
    std::vector<uint32_t> free_slots_, free_tables_, comb_of_, pins_;
    std::unordered_set<uint32_t> reg_slots_;
    uint32_t slot_cap_ = 0, slot_hw_ = 0, table_cap_ = 0, table_hw_ = 0;
    uint64_t reg_fp_ = 0;
};

}  // namespace nwv
