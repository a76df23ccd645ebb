// bls_apk_ring.h -- the bookkeeping of a device's ring of aggregate BLS keys (host code, no HIP).
//
// A certificate's item sums its signers' keys and then computes the sum's Miller-loop lines step
// by step, where a registered key's item reads a table made at registration.  Signer sets recur (a
// small committee has few quorums, a certificate is validated again, fetched again), so the engine
// keeps, per device, a ring of `cap` records: the affine sum of a set's [h_eff] pk records and that
// point's line table.  This header is the host side of the ring: which set a slot holds, which
// slots a call in flight may still write (busy) or read (pinned), the FIFO cursor that picks the
// next slot to overwrite, and the filter that lets a set in only at its second sighting.  The
// records live in device memory and are never touched here.
//
// Keys.  A set is the item's key-cache slot indices, sorted, duplicates kept ([a, a, b] and [a, b]
// have different sums), of MIN_KEYS to MAX_KEYS entries.  Only the key cache's current epoch gives
// an index list a meaning: reset() drops everything when the cache drops its slots.  The table
// hash is multilinear over the list with per-process random multipliers (as group_keys.h), and
// every table hit is confirmed on the whole list: crafted lists may cost probes, they never alias
// two sets.
//
// Slots.  held / busy / pins, reserve(), publish(), release() and unpin() as bls_msg_ring.h has
// them: reserve() hands out the first slot from the cursor that is neither busy nor pinned,
// unmaps what it held and marks it busy, or returns NONE (not an error: the item computes as
// without the ring); publish() maps a reserved slot once the kernel that wrote it has completed
// and its item has verified, and when another call published the set meanwhile the earlier
// mapping stays.  One plain mutex, taken for a few probes; NO lock is held across GPU work.
//
// The second-sighting filter.  A large committee's quorums almost never recur, and a fill costs a
// kernel, so a set is filled only when it has been seen before: a direct-mapped table of 4 cap
// 64-bit set hashes.  miss() of a set whose hash is in its entry reserves a slot; otherwise it
// writes the hash there (the set is NOTED) and reserves nothing.  Two sets that share an entry
// and a hash make a fill come one sighting early, sets that share an entry push each other out and
// make it come later; neither changes a result, since lookups compare whole lists.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <random>
#include <vector>

namespace nwv {

struct ApkKey {
    static constexpr size_t MIN_KEYS = 2, MAX_KEYS = 1024;
    std::vector<uint32_t> idx;  // sorted
    uint64_t h = 0;             // hash() of idx
    static bool eligible(size_t cnt) { return cnt >= MIN_KEYS && cnt <= MAX_KEYS; }
    // (cnt within the limits)
    static ApkKey make(const uint32_t* idx, size_t cnt) {
        ApkKey k;
        k.idx.assign(idx, idx + cnt);
        std::sort(k.idx.begin(), k.idx.end());
        k.h = hash(k.idx.data(), cnt);
        return k;
    }
    bool operator==(const ApkKey& o) const { return h == o.h && idx == o.idx; }
    // the table hash: multilinear over the length and the entries, per-process random odd multipliers
    static uint64_t hash(const uint32_t* v, size_t cnt) {
        const Salt& s = salt();
        uint64_t h = s.a[MAX_KEYS + 1] + (uint64_t)cnt * s.a[MAX_KEYS];
        for (size_t i = 0; i < cnt; i++) h += ((uint64_t)v[i] + 1) * s.a[i];
        return (h ^ (h >> 31)) * 0xFF51AFD7ED558CCDull;
    }

  private:
    struct Salt {
        uint64_t a[MAX_KEYS + 2];
    };
    static const Salt& salt() {
        static const Salt v = [] {
            std::random_device rd;
            Salt s;
            for (uint64_t& x : s.a) x = (((uint64_t)rd() << 32) ^ rd() ^ 0x9E3779B97F4A7C15ull) | 1;
            return s;
        }();
        return v;
    }
};

class BlsApkRing {
  public:
    static constexpr uint32_t NONE = UINT32_MAX;
    static constexpr uint32_t MAX_SLOTS = 4096;

    // cap slots, all free, an empty filter of 4 cap entries.  The table has 2^k >= 2 cap buckets
    // (chained through the slots); lg_buckets >= 0 fixes k instead (tests: 0 is one bucket).
    void init(uint32_t cap, int lg_buckets = -1) {
        std::lock_guard<std::mutex> g(mu_);
        cap_ = cap;
        int lg = 4;
        while (((size_t)1 << lg) < 2 * (size_t)cap) lg++;
        if (lg_buckets >= 0) lg = lg_buckets;
        lg_ = lg;
        head_.assign((size_t)1 << lg, NONE);
        next_.assign(cap, NONE);
        key_.assign(cap, ApkKey{});
        held_.assign(cap, 0);
        busy_.assign(cap, 0);
        pins_.assign(cap, 0);
        filt_.assign(4 * (size_t)cap, 0);
        fset_.assign(4 * (size_t)cap, 0);
        cursor_ = 0;
    }
    uint32_t cap() const { return cap_; }
    // the filter entry a hash falls into (tests force collisions with it)
    size_t filter_entry(uint64_t h) const { return cap_ ? (size_t)(h % (4 * (uint64_t)cap_)) : 0; }

    // the slot published under the set, pinned for the caller; NONE: a miss
    uint32_t lookup_pin(const ApkKey& k) {
        std::lock_guard<std::mutex> g(mu_);
        const uint32_t s = find(k);
        if (s != NONE) pins_[s]++;
        return s;
    }
    bool contains(const ApkKey& k) {
        std::lock_guard<std::mutex> g(mu_);
        return find(k) != NONE;
    }
    // a set the ring does not hold.  Seen before (its hash is in its filter entry): reserve() for
    // it.  Else the hash is written there, *noted = true and NONE comes back.
    uint32_t miss(const ApkKey& k, bool* noted) {
        std::lock_guard<std::mutex> g(mu_);
        *noted = false;
        if (!cap_) return NONE;
        const size_t e = filter_entry(k.h);
        if (fset_[e] && filt_[e] == k.h) return reserve_locked();
        filt_[e] = k.h;
        fset_[e] = 1;
        *noted = true;
        return NONE;
    }
    // the next slot from the cursor that no call writes or reads, unmapped and marked busy; NONE
    // when every slot is busy or pinned
    uint32_t reserve() {
        std::lock_guard<std::mutex> g(mu_);
        return reserve_locked();
    }
    // a reserved slot, its record complete, mapped under the set.  Returns the slot the set maps to
    // afterwards: `slot`, or the one another call published meanwhile (`slot` is then released).
    uint32_t publish(uint32_t slot, const ApkKey& k) {
        std::lock_guard<std::mutex> g(mu_);
        busy_[slot] = 0;
        const uint32_t other = find(k);
        if (other != NONE) return other;
        key_[slot] = k;
        const size_t b = bucket(k);
        next_[slot] = head_[b];
        head_[b] = slot;
        held_[slot] = 1;
        return slot;
    }
    // a reserved slot given back unpublished
    void release(uint32_t slot) {
        std::lock_guard<std::mutex> g(mu_);
        busy_[slot] = 0;
    }
    void unpin(uint32_t slot) {
        std::lock_guard<std::mutex> g(mu_);
        if (pins_[slot]) pins_[slot]--;
    }
    // the key cache dropped its slots: every mapping and the whole filter go (an index list now
    // names other keys).  The caller holds the key cache exclusively, so no call is in flight; a
    // slot some failed call abandoned busy or pinned stays so.
    void reset() {
        std::lock_guard<std::mutex> g(mu_);
        for (uint32_t t = 0; t < cap_; t++)
            if (held_[t]) unmap(t);
        std::fill(fset_.begin(), fset_.end(), 0);
        std::fill(filt_.begin(), filt_.end(), 0);
        cursor_ = 0;
    }
    // out[0] held, out[1] busy, out[2] pinned slots
    void counts(uint64_t out[3]) {
        std::lock_guard<std::mutex> g(mu_);
        out[0] = out[1] = out[2] = 0;
        for (uint32_t t = 0; t < cap_; t++) {
            out[0] += held_[t] ? 1 : 0;
            out[1] += busy_[t] ? 1 : 0;
            out[2] += pins_[t] ? 1 : 0;
        }
    }
    // one slot's state (tests): bit 0 held, bit 1 busy, bits 8.. the pin count
    uint32_t slot_state(uint32_t slot) {
        std::lock_guard<std::mutex> g(mu_);
        return (held_[slot] ? 1u : 0u) | (busy_[slot] ? 2u : 0u) | (pins_[slot] << 8);
    }
    // filter entries in use (tests)
    size_t filter_used() {
        std::lock_guard<std::mutex> g(mu_);
        size_t n = 0;
        for (uint8_t f : fset_) n += f ? 1 : 0;
        return n;
    }

  private:
    size_t bucket(const ApkKey& k) const { return lg_ ? (size_t)(k.h >> (64 - lg_)) : 0; }
    uint32_t find(const ApkKey& k) const {
        if (!cap_) return NONE;
        for (uint32_t s = head_[bucket(k)]; s != NONE; s = next_[s])
            if (key_[s] == k) return s;  // the whole list
        return NONE;
    }
    uint32_t reserve_locked() {
        for (uint32_t seen = 0, t = cursor_; seen < cap_; seen++, t = t + 1 == cap_ ? 0 : t + 1) {
            if (busy_[t] || pins_[t]) continue;
            if (held_[t]) unmap(t);
            busy_[t] = 1;
            cursor_ = t + 1 == cap_ ? 0 : t + 1;
            return t;
        }
        return NONE;
    }
    void unmap(uint32_t t) {
        uint32_t* p = &head_[bucket(key_[t])];
        while (*p != NONE && *p != t) p = &next_[*p];
        if (*p == t) *p = next_[t];
        next_[t] = NONE;
        held_[t] = 0;
    }
    std::mutex mu_;
    uint32_t cap_ = 0, cursor_ = 0;
    int lg_ = 0;
    std::vector<uint32_t> head_, next_, pins_;
    std::vector<ApkKey> key_;
    std::vector<uint8_t> held_, busy_, fset_;
    std::vector<uint64_t> filt_;
};

}  // namespace nwv
