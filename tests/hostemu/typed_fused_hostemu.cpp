// typed_fused_hostemu.cpp -- TEST-ONLY host build of the pieces of the one-launch typed path
// (nwv_set_typed_fused; tests/test_typed_fused_hostemu.py).  Never part of the product.
//   he_b2_one_block     blake2b.h's one-lane one-block BLAKE2b-256 (blake2b256_one_block)
//   he_typed_verify     k_ed_tiny_fused's signature workgroups, one signature each: the hashing
//                       lane's typed_message (comb.h: the literal, or the digest of a one-block
//                       preimage, stored for the host when the src word asks), then the check of
//                       comb_hostemu.cpp on the emulated wave (the equation and the tables are
//                       k_ed_tiny's; a group of one signature is its workgroup)
//   the stub engine     nwv_types.cpp is linked into this library over engine calls that record
//                       the plan they were given (he_plan) and answer with real BLAKE2b-256 digests
//                       and a stand-in signature rule: a "signature" is valid when its first 32
//                       bytes are message XOR key.  he_set_typed_fused is the engine's setting.
#include "comb_hostemu.cpp"

#include "../../include/nwv_types.h"

namespace {

std::vector<uint8_t> padded(const uint8_t* p, size_t n) {
    std::vector<uint8_t> m(n + 64, 0);
    if (n) std::memcpy(m.data(), p, n);
    return m;
}

// k_blake2b_many's loop (the stub engine's digests: any length)
void b2_any(const uint8_t* p, uint64_t L, uint8_t out[32]) {
    const std::vector<uint8_t> m8 = padded(p, (size_t)L);
    blake2b_state s;
    blake2b_init256(s);
    const uint64_t nblocks = L == 0 ? 1 : (L + 127) / 128;
    for (uint64_t b = 0; b < nblocks; b++) {
        u64p m[16];
        for (int t = 0; t < 16; t++) {
            m[t].lo = msg_word_trim(m8.data(), 128 * b + 8 * t, L);
            m[t].hi = msg_word_trim(m8.data(), 128 * b + 8 * t + 4, L);
        }
        const bool last = b + 1 == nblocks;
        blake2b_compress(s, m, last ? (uint32_t)(L - 128 * b) : 128u, last);
    }
    uint32_t d[8];
    blake2b_digest256(s, d);
    std::memcpy(out, d, 32);
}

int g_setting = 0;
std::vector<uint32_t> g_plan;      // the last engine call, see he_plan
std::vector<uint8_t> g_plan_lits;  // its literals

bool stand_in_valid(const uint8_t* key, const uint8_t* sig, const uint8_t* msg) {
    for (int q = 0; q < 32; q++)
        if (sig[q] != (uint8_t)(msg[q] ^ key[q])) return false;
    return true;
}

}  // namespace

extern "C" {

void he_b2_one_block(const uint8_t* p, uint32_t len, uint8_t out[32]) {
    const std::vector<uint8_t> m = padded(p, len);
    uint32_t d[8];
    blake2b256_one_block(m.data(), len, d);
    std::memcpy(out, d, 32);
}

// src[i]: comb.h's src word of signature i; short_out: [digests][8] words.  Returns he_comb_verify's code.
int he_typed_verify(uint32_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, const uint64_t* off,
                    const uint32_t* len, const uint32_t* src, uint32_t* short_out, uint8_t* verdict) {
    for (uint32_t i = 0; i < n; i++) {
        const std::vector<uint8_t> m = padded(msg + off[i], len[i]);
        uint32_t dbuf[TYPED_DBUF_WORDS];
        uint32_t ml = len[i];
        const uint8_t* mp = typed_message(src[i], m.data(), ml, dbuf, short_out);
        const uint64_t zero = 0;
        const int rc = he_comb_verify(1, pk + 32 * (size_t)i, sig + 64 * (size_t)i, mp, &zero, &ml, verdict + i);
        if (rc) return rc;
    }
    return 0;
}

// ---- the stub engine under nwv_types.cpp ----
void he_set_typed_fused(int on) { g_setting = on; }
int nwv_typed_fused(const nwv_ctx*) { return g_setting; }
int nwv_keycache_register(nwv_ctx*, size_t, const uint8_t*) { return NWV_OK; }
int nwv_blake2b256_many(nwv_ctx*, size_t n, const uint8_t* base, const uint64_t* off, const uint64_t* len,
                        uint8_t* out) {
    for (size_t i = 0; i < n; i++) b2_any(base + off[i], len[i], out + 32 * i);
    return NWV_OK;
}
// the plan: [entry (0 keyed_digests, 1 typed), n_pre, n_lit, n, then len and short flag of every
// preimage, then key index and message index of every signature]
static void record(uint32_t entry, size_t n_pre, const uint64_t* len, const uint8_t* is_short, size_t n_lit,
                   const uint8_t* lits, size_t n, const uint32_t* kidx, const uint32_t* midx) {
    g_plan = {entry, (uint32_t)n_pre, (uint32_t)n_lit, (uint32_t)n};
    for (size_t j = 0; j < n_pre; j++) {
        g_plan.push_back((uint32_t)len[j]);
        g_plan.push_back(is_short ? is_short[j] : 0u);
    }
    for (size_t i = 0; i < n; i++) {
        g_plan.push_back(kidx[i]);
        g_plan.push_back(midx[i]);
    }
    g_plan_lits.assign(lits, lits + 32 * n_lit);
}
static void answer(size_t n_pre, const uint8_t* dig, const uint8_t* lits, const uint8_t* keys, size_t n,
                   const uint32_t* kidx, const uint8_t* sig, const uint32_t* midx, int* all_valid, uint64_t* bits) {
    *all_valid = 1;
    if (bits) std::memset(bits, 0, 8 * ((n + 63) / 64));
    for (size_t i = 0; i < n; i++) {
        const uint8_t* m = midx[i] < n_pre ? dig + 32 * (size_t)midx[i] : lits + 32 * (size_t)(midx[i] - n_pre);
        const bool ok = stand_in_valid(keys + 32 * (size_t)kidx[i], sig + 64 * i, m);
        if (!ok) *all_valid = 0;
        if (ok && bits) bits[i >> 6] |= 1ull << (i & 63);
    }
}
int nwv_ed25519_verify_batch_keyed_digests(nwv_ctx* ctx, size_t n_pre, const uint8_t* base, const uint64_t* off,
                                           const uint64_t* len, uint8_t* dig, size_t, const uint8_t* keys, size_t n,
                                           const uint32_t* kidx, const uint8_t* sig, const uint32_t* didx,
                                           const uint8_t*, int* all_valid, uint64_t* bits) {
    record(0, n_pre, len, nullptr, 0, nullptr, n, kidx, didx);
    nwv_blake2b256_many(ctx, n_pre, base, off, len, dig);
    answer(n_pre, dig, nullptr, keys, n, kidx, sig, didx, all_valid, bits);
    return NWV_OK;
}
int nwv_ed25519_verify_batch_typed(nwv_ctx* ctx, size_t n_pre, const uint8_t* base, const uint64_t* off,
                                   const uint64_t* len, const uint8_t* is_short, uint8_t* dig, size_t n_lit,
                                   const uint8_t* lits, size_t, const uint8_t* keys, size_t n, const uint32_t* kidx,
                                   const uint8_t* sig, const uint32_t* midx, const uint8_t*, int* all_valid,
                                   uint64_t* bits) {
    record(1, n_pre, len, is_short, n_lit, lits, n, kidx, midx);
    nwv_blake2b256_many(ctx, n_pre, base, off, len, dig);
    answer(n_pre, dig, lits, keys, n, kidx, sig, midx, all_valid, bits);
    return NWV_OK;
}
// the last engine call's plan into out (cap words; returns its length) and its literals into lits
int he_plan(uint32_t* out, int cap, uint8_t* lits, int lits_cap) {
    for (int k = 0; k < cap && k < (int)g_plan.size(); k++) out[k] = g_plan[k];
    for (int k = 0; k < lits_cap && k < (int)g_plan_lits.size(); k++) lits[k] = g_plan_lits[k];
    return (int)g_plan.size();
}

// the BLS12-381 layer's engine calls (nwv_types.cpp links them; never called here)
int nwv_bls_keycache_register(nwv_ctx*, size_t, const uint8_t*) { return NWV_OK; }
int nwv_bls_verify_many(nwv_ctx*, size_t, const uint8_t*, size_t n, const uint8_t*, const uint32_t*, const uint32_t*,
                        const uint32_t*, const uint8_t*, const uint64_t*, const uint32_t*, const uint8_t*, size_t,
                        int32_t* status) {
    std::memset(status, 0, 4 * n);
    return NWV_OK;
}
size_t nwv_bls_msg_ring(const nwv_ctx*) { return 0; }
int nwv_bls_verify_many_ahead(nwv_ctx*, size_t, const uint8_t*, size_t n, const uint8_t*, const uint32_t*,
                              const uint32_t*, const uint32_t*, const uint8_t*, const uint64_t*, const uint32_t*,
                              const uint8_t*, size_t, int32_t* status, size_t, const uint8_t*, const uint64_t*,
                              const uint32_t*, const uint32_t*) {
    std::memset(status, 0, 4 * n);
    return NWV_OK;
}
int nwv_bls_aggregate(nwv_ctx*, size_t, const uint8_t*, uint8_t out48[48], int32_t*) {
    std::memset(out48, 0, 48);
    return NWV_OK;
}

}  // extern "C"
