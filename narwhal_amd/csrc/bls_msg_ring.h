// bls_msg_ring.h -- the bookkeeping of a device's ring of hashed BLS message points (host code, no
// HIP).
//
// A small BLS call spends about a fifth of its time hashing its message to G1, and most protocol
// messages repeat: the votes for a header and the certificate built from them sign one 32-byte
// digest.  The engine keeps, per device, a ring of `cap` records, one RAW hashed point each (the
// sum of the two isogeny maps, before the cofactor is cleared: bls_verify.h w_hash_to_g1), keyed by
// (dst_len, dst, msg_len, msg).  This header is the host side of that ring: which key a slot
// holds, which slots a call in flight may still write (busy) or read (pinned), and the FIFO cursor
// that picks the next slot to overwrite.  The records themselves live in device memory and are
// never touched here.
//
// Keys.  Only messages of at most MAX_MSG bytes under a DST of at most MAX_DST bytes are cached
// (protocol messages are 32-byte digests, NWV_BLS_DST is 43 bytes); a key is the four fields in a
// fixed 136-byte block, zero padded, so equality of blocks is equality of the fields.  The message
// bytes are the peer's, so the table hash is a multilinear hash of the block's 17 words with
// per-process random multipliers (as group_keys.h), and every table hit is confirmed on every
// byte: crafted messages may cost probes, they never alias two messages.
//
// Slots.  held: published under a key (lookups find it).  busy: reserved by a call whose kernels
// may still write the record.  pins: calls whose kernels may still read it.  reserve() hands out
// the first slot from the cursor that is neither busy nor pinned, unmaps what it held and marks it
// busy; with no such slot it returns NONE, which is not an error (the caller computes its hash and
// publishes nothing).  publish() maps a reserved slot under its key once the kernels that wrote it
// have completed; when another call published the same key in the meantime the earlier mapping
// stays and the slot is released, so a key maps to at most one slot.  Every operation takes the
// one mutex for a few table probes; NO lock is held across GPU work -- every verify call both
// reads and reserves, so a lock held until a stream synchronises would serialise concurrent
// callers.  Pins and busy flags are what keep a record from being rewritten under a reader.
//
// A call that fails after its kernels were queued synchronises its streams before it releases or
// unpins; if that fails too it does neither, and its slots stay busy or pinned for good
// (abandoned), so no later call can be handed a slot a late write may still land in.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <random>
#include <vector>

namespace nwv {

struct MsgKey {
    static constexpr size_t MAX_MSG = 64, MAX_DST = 64;
    uint64_t w[17];  // w[0] = dst_len | msg_len << 8; bytes 8..71 dst, 72..135 msg, zero padded
    static bool cacheable(size_t dst_len, size_t msg_len) { return dst_len <= MAX_DST && msg_len <= MAX_MSG; }
    // (dst_len, msg_len within the limits)
    static MsgKey make(const uint8_t* dst, size_t dst_len, const uint8_t* msg, size_t msg_len) {
        MsgKey k;
        std::memset(k.w, 0, sizeof k.w);
        k.w[0] = (uint64_t)dst_len | ((uint64_t)msg_len << 8);
        uint8_t* b = reinterpret_cast<uint8_t*>(k.w);
        if (dst_len) std::memcpy(b + 8, dst, dst_len);
        if (msg_len) std::memcpy(b + 8 + MAX_DST, msg, msg_len);
        return k;
    }
    bool operator==(const MsgKey& o) const { return std::memcmp(w, o.w, sizeof w) == 0; }
    // the table hash: multilinear over the 17 words, per-process random odd multipliers
    uint64_t hash() const {
        const Salt& s = salt();
        uint64_t h = s.a[17];
        for (int i = 0; i < 17; i++) h += w[i] * s.a[i];
        return (h ^ (h >> 31)) * 0xFF51AFD7ED558CCDull;
    }

  private:
    struct Salt {
        uint64_t a[18];
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

class BlsMsgRing {
  public:
    static constexpr uint32_t NONE = UINT32_MAX;
    static constexpr uint32_t MAX_SLOTS = 65536;

    // cap slots, all free.  The table has 2^k >= 2 cap buckets (chained through the slots);
    // lg_buckets >= 0 fixes k instead (tests: 0 puts every key into one bucket).
    void init(uint32_t cap, int lg_buckets = -1) {
        std::lock_guard<std::mutex> g(mu_);
        cap_ = cap;
        int lg = 4;
        while (((size_t)1 << lg) < 2 * (size_t)cap) lg++;
        if (lg_buckets >= 0) lg = lg_buckets;
        lg_ = lg;
        head_.assign((size_t)1 << lg, NONE);
        next_.assign(cap, NONE);
        key_.resize(cap);
        held_.assign(cap, 0);
        busy_.assign(cap, 0);
        pins_.assign(cap, 0);
        cursor_ = 0;
    }
    uint32_t cap() const { return cap_; }

    // the slot published under the key, pinned for the caller; NONE: a miss
    uint32_t lookup_pin(const MsgKey& k) {
        std::lock_guard<std::mutex> g(mu_);
        const uint32_t s = find(k);
        if (s != NONE) pins_[s]++;
        return s;
    }
    // whether the key is published (no pin: an ahead message that is there already is skipped)
    bool contains(const MsgKey& k) {
        std::lock_guard<std::mutex> g(mu_);
        return find(k) != NONE;
    }
    // the next slot from the cursor that no call writes or reads, unmapped and marked busy; NONE
    // when every slot is busy or pinned
    uint32_t reserve() {
        std::lock_guard<std::mutex> g(mu_);
        for (uint32_t seen = 0, t = cursor_; seen < cap_; seen++, t = t + 1 == cap_ ? 0 : t + 1) {
            if (busy_[t] || pins_[t]) continue;
            if (held_[t]) unmap(t);
            busy_[t] = 1;
            cursor_ = t + 1 == cap_ ? 0 : t + 1;
            return t;
        }
        return NONE;
    }
    // a reserved slot, its record complete, mapped under the key.  Returns the slot the key maps to
    // afterwards: `slot`, or the one another call published under the key meanwhile (`slot` is
    // then released unmapped).
    uint32_t publish(uint32_t slot, const MsgKey& k) {
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

  private:
    size_t bucket(const MsgKey& k) const { return lg_ ? (size_t)(k.hash() >> (64 - lg_)) : 0; }
    uint32_t find(const MsgKey& k) const {
        if (!cap_) return NONE;
        for (uint32_t s = head_[bucket(k)]; s != NONE; s = next_[s])
            if (key_[s] == k) return s;  // every byte
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
    std::vector<MsgKey> key_;
    std::vector<uint8_t> held_, busy_;
};

}  // namespace nwv
