// group_keys.h -- the distinct verification keys of a batch that names one key per signature
// (host code, no HIP).
//
// The fastcrypto trait surface hands the engine n (key, signature) pairs; the keyed paths want the
// distinct keys and, per signature, an index into them.  ed25519-consensus' batch::Verifier groups
// its queue the same way, by the raw VerificationKeyBytes, so equality here is byte equality: two
// encodings of one point (a non-canonical y, the sign bit of x = 0) are two keys, as they are to
// the challenge hash.
//
// One pass over the keys through an open-addressed table of 2^k >= 2 n entries (linear probing).
// The caller of a trait chooses the key bytes, so they are hashed with per-process random
// multipliers (a multilinear hash of the four 64-bit words, top bits taken), and every table hit is
// confirmed by comparing all 32 bytes: crafted keys may cost probes, they can never merge two
// keys.  The distinct keys come out in order of first occurrence.
//
// The pass writes 12 bytes per key (a table entry, an index) and compares against the caller's
// own array; the distinct keys are copied out only after a pass that was not given up, so a batch
// of strangers that stops past its limit has copied nothing.
//
// A KeyGrouper keeps its table and its output between calls (one per thread in the engine): once
// they have grown to a size, a call of that size allocates nothing.  The table is not cleared
// between calls; an entry is live only if it carries the current call's stamp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

namespace nwv {

class KeyGrouper {
  public:
    // Group keys[0 .. 32 n).  Returns false, with the output undefined, as soon as more than
    // max_distinct distinct keys have been seen (a caller that gains nothing from that many groups
    // does not pay for the rest of the pass); true otherwise.
    bool group(const uint8_t* keys, size_t n, size_t max_distinct = SIZE_MAX) {
        m_ = 0;
        if (idx_.size() < n) idx_.resize(n);
        if (n == 0) return true;
        if (first_.size() < n) first_.resize(n);
        size_t want = 16;
        int lg = 4;
        while (want < 2 * n) want <<= 1, lg++;
        if (tab_.size() < want) {
            tab_.assign(want, Entry{0, 0});
            lg_ = lg;
            stamp_ = 0;
        }
        if (++stamp_ == 0) {  // the stamp wrapped: old entries would look live again
            std::fill(tab_.begin(), tab_.end(), Entry{0, 0});
            stamp_ = 1;
        }
        // (the whole table is used even when it is larger than this call needs: fewer probes)
        const size_t mask = tab_.size() - 1;
        const int shift = 64 - lg_;
        const Salt& s = salt();
        Entry* tab = tab_.data();
        uint32_t* idx = idx_.data();
        uint32_t* first = first_.data();
        const uint32_t stamp = stamp_;
        size_t m = 0;
        for (size_t i = 0; i < n; i++) {
            const uint8_t* k = keys + 32 * i;
            uint64_t w[4];
            std::memcpy(w, k, 32);
            uint64_t h = s.a[4] + w[0] * s.a[0] + w[1] * s.a[1] + w[2] * s.a[2] + w[3] * s.a[3];
            h = (h ^ (h >> 31)) * 0xFF51AFD7ED558CCDull;
            for (size_t p = (size_t)(h >> shift);; p = (p + 1) & mask) {
                Entry& e = tab[p];
                if (e.stamp != stamp) {  // free: a key not seen before
                    if (m == max_distinct) return false;
                    e.stamp = stamp;
                    e.id = (uint32_t)m;
                    first[m] = (uint32_t)i;
                    idx[i] = (uint32_t)m++;
                    break;
                }
                uint64_t f[4];  // all 32 bytes of the group's first key against this one
                std::memcpy(f, keys + 32 * (size_t)first[e.id], 32);
                if (((f[0] ^ w[0]) | (f[1] ^ w[1]) | (f[2] ^ w[2]) | (f[3] ^ w[3])) == 0) {
                    idx[i] = e.id;
                    break;
                }
            }
        }
        m_ = m;
        if (distinct_.size() < 32 * m) distinct_.resize(32 * m);
        for (size_t j = 0; j < m; j++) std::memcpy(distinct_.data() + 32 * j, keys + 32 * (size_t)first[j], 32);
        return true;
    }
    size_t n_distinct() const { return m_; }
    const uint8_t* distinct() const { return distinct_.data(); }  // n_distinct() x 32, first occurrence order
    const uint32_t* key_idx() const { return idx_.data(); }       // n, into distinct()
    // what the scratch holds now (tests: a second call of no larger size leaves them as they are)
    size_t table_capacity() const { return tab_.size(); }
    size_t out_capacity() const { return distinct_.capacity() + 4 * idx_.capacity() + 4 * first_.capacity(); }

  private:
    struct Entry {
        uint32_t stamp, id;
    };
    struct Salt {
        uint64_t a[5];
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
    std::vector<Entry> tab_;
    int lg_ = 4;
    uint32_t stamp_ = 0;
    std::vector<uint8_t> distinct_;
    std::vector<uint32_t> idx_, first_;
    size_t m_ = 0;
};

}  // namespace nwv
