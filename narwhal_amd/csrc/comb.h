// comb.h -- lane-level pieces of the per-signature comb check (comb_kernels.hip k_ed_comb): the
// equation of k_ed_tiny (tiny_kernels.hip), [8] R = [8]([s]B - [k]A) with [s]B - [k]A summed from
// the fixed-base combs of B and of the registered key, for keyed batches above TINY_MAX, and of
// the same check as a per-signature pass behind a rejected batch MSM (k_ed_comb_pass4 / 16).
// Everything here is __host__ __device__: the kernels call these functions and
// tests/hostemu/comb_hostemu.cpp and comb_pass_hostemu.cpp run the same ones on the CPU.
#pragma once
#include "blake2b.h"
#include "ed25519_lane.h"
#include "msm.h"

namespace nwv {

// signatures a workgroup of k_ed_comb takes: hashing lanes, decompression rows, comb waves
static constexpr int COMB_G = 4;

// One signature's scalars: k = SHA-512(R || A || M) mod l and s, as the signed radix-16 digits
// (msm.h comb_digits) that index the comb tables.  s >= l fails the signature (returns false) and
// its digits, which would index past the tables, are zeroed.
NWV_HD bool comb_scalars(const uint32_t Aw[8], const uint32_t Rw[8], const uint32_t Sw[8], const uint8_t* msg,
                         uint32_t mlen, int ds[COMB_TABLES], int dk[COMB_TABLES]) {
    uint32_t k[8], s[8];
    const bool sok = lane_hash(Aw, Rw, Sw, msg, mlen, k) == FLAG_S_OK;
    for (int q = 0; q < 8; q++) s[q] = sok ? Sw[q] : 0u;
    comb_digits(s, ds);
    comb_digits(k, dk);
    return sok;
}

// Digit position j's term of [s]B - [k]A: entry |ds| of table j of B's comb with the sign of ds,
// plus entry |dk| of table j of A's comb with the opposite sign of dk.
NWV_HD ge_p3 comb_term(const uint32_t* bcomb, const uint32_t* acomb, int j, int ds, int dk) {
    ge_p3 P = ge_p3_identity();
    if (ds) {
        const int m = ds < 0 ? -ds : ds;
        P = ge_p1p1_to_p3(ge_madd(P, msm_load_point(bcomb + MSM_PT_WORDS * (COMB_ENTRIES * j + m - 1), ds < 0)));
    }
    if (dk) {
        const int m = dk < 0 ? -dk : dk;
        P = ge_p1p1_to_p3(ge_madd(P, msm_load_point(acomb + MSM_PT_WORDS * (COMB_ENTRIES * j + m - 1), dk > 0)));
    }
    return P;
}

// [8] R = [8] P projectively from p8 = X | Y | Z | T of [8] P (P3_WORDS words) and r8 = X | Y | Z
// of [8] R (ten limbs each): cross product c of the four (P.X RZ, RX P.Z, P.Y RZ, RY P.Z) as
// eight canonical words; the points are equal when products 0 and 1 and products 2 and 3 agree.
NWV_HD void comb_cross(const uint32_t* p8, const uint32_t* r8, int c, uint32_t out[8]) {
    const uint32_t* u = ((c & 1) ? r8 : p8) + (c < 2 ? 0 : 10);
    const uint32_t* v = ((c & 1) ? p8 : r8) + 20;
    fe_freeze(fe_mul(load_fe(u), load_fe(v)), out);
}
NWV_HD bool comb_cross_equal(const uint32_t x[32]) {
    bool id = true;
    for (int q = 0; q < 8; q++) id = id && x[q] == x[8 + q] && x[16 + q] == x[24 + q];
    return id;
}

// ---- typed calls with their digests in the same launch (k_ed_tiny_fused, k_ed_comb_fused) ----
// A signature of a typed call (Header / Vote / Certificate verification, nwv_types.cpp) signs
// either bytes the host already holds (a header's id) or the BLAKE2b-256 of a preimage of at most
// one block (Vote::digest, Certificate::digest: 80 bytes).  The fused kernels take the second kind
// as the preimage itself: the lane that hashes R || A || M compresses it first (blake2b.h
// blake2b256_one_block) and signs over the digest.  Signatures that share a preimage each
// recompute the one compression; nobody waits for anybody.
// src word of signature i: 0 = off[i] / len[i] name the literal message; otherwise they name the
// preimage of short digest (src & ~TYPED_SRC_STORE) - 1, and with TYPED_SRC_STORE this signature
// (the first that uses the digest) also stores it for the host.
static constexpr uint32_t TYPED_SRC_STORE = 0x80000000u;
static constexpr int TYPED_DBUF_WORDS = 16;  // the digest and the aligned over-read behind it
struct TypedFusedArgs {
    const uint32_t* src;   // [n]
    uint32_t* short_out;   // coherent pinned host memory: [short digests][8]
    uint32_t sig_blocks;   // workgroups that check signatures; the rest hash side preimages
};
// The message signature i is checked over: the literal (returned as it is), or the digest of the
// preimage, written to dbuf (TYPED_DBUF_WORDS words the lane owns: LDS on the device) and, when the
// src word asks, to short_out.
NWV_HD const uint8_t* typed_message(uint32_t src, const uint8_t* msg, uint32_t& mlen, uint32_t* dbuf,
                                    uint32_t* short_out) {
    if (src == 0u) return msg;
    uint32_t d[8];
    blake2b256_one_block(msg, mlen, d);
    for (int q = 0; q < 8; q++) dbuf[q] = d[q];
    for (int q = 8; q < TYPED_DBUF_WORDS; q++) dbuf[q] = 0u;
    if ((src & TYPED_SRC_STORE) && short_out) {
        uint32_t* o = short_out + 8 * (size_t)((src & ~TYPED_SRC_STORE) - 1u);
        for (int q = 0; q < 8; q++) o[q] = d[q];
    }
    mlen = 32u;
    return reinterpret_cast<const uint8_t*>(dbuf);
}

// ---- k_ed_comb_pass (comb_kernels.hip): the same check with the comb sum walked by lanes ----
// COMB_PASS_G signatures a workgroup; L lanes a signature (4 or 16), each lane 64 / L consecutive
// digit positions of both combs.
static constexpr int COMB_PASS_G = 16;

// Entry |d| of table j of a comb as a mixed-addition operand, negated when neg; a zero digit gives
// the neutral record (1 | 1 | 0) by selection from entry 1's load, so lanes of a wave never branch
// on a digit.
NWV_HD ge_precomp comb_record(const uint32_t* comb, int j, int d, bool neg) {
    const int m = d < 0 ? -d : d;
    const ge_precomp q = msm_load_point(comb + MSM_PT_WORDS * (COMB_ENTRIES * j + (m ? m - 1 : 0)), neg);
    const bool z = m == 0;
    return ge_precomp{fe_select(q.ypx, fe_one(), z), fe_select(q.ymx, fe_one(), z), fe_select(q.xy2d, fe_zero(), z)};
}

// One lane's share of [s]B - [k]A: positions j0 .. j0 + cnt - 1 (ds, dk: the digits from position
// j0 on).  The sum is seeded from position j0's B record (msm_point_seed; the neutral record seeds
// the identity as (0 : 2 : 2 : 0)), every other record joins by a mixed addition.
NWV_HD ge_p3 comb_lane_sum(const uint32_t* bcomb, const uint32_t* acomb, int j0, int cnt, const int* ds,
                           const int* dk) {
    ge_p3 P = msm_point_seed(comb_record(bcomb, j0, ds[0], ds[0] < 0));
    P = ge_p1p1_to_p3(ge_madd(P, comb_record(acomb, j0, dk[0], dk[0] > 0)));
#pragma unroll 1
    for (int p = 1; p < cnt; p++) {
        P = ge_p1p1_to_p3(ge_madd(P, comb_record(bcomb, j0 + p, ds[p], ds[p] < 0)));
        P = ge_p1p1_to_p3(ge_madd(P, comb_record(acomb, j0 + p, dk[p], dk[p] > 0)));
    }
    return P;
}

// One level of the join of a signature's lane sums: the lane keeps its sum plus its partner's
// (level o: lane t, t a multiple of 2 o, takes lane t + o's).
NWV_HD ge_p3 comb_join(const ge_p3& mine, const ge_p3& theirs) { return p3_add(mine, theirs); }

// [8] R = [8] P projectively from the joined sum P (doubled three times here) and r8 = X | Y | Z of
// [8] R (ten limbs each): comb_cross's four products, compared as canonical words.
NWV_HD bool comb_pass_equal(const ge_p3& P, const uint32_t* r8) {
    const ge_p3 P8 = p3_dbl_n(P, 3);
    const fe rz = load_fe(r8 + 20);
    uint32_t a[8], b[8];
    fe_freeze(fe_mul(P8.X, rz), a);
    fe_freeze(fe_mul(load_fe(r8), P8.Z), b);
    bool eq = true;
    for (int q = 0; q < 8; q++) eq = eq && a[q] == b[q];
    fe_freeze(fe_mul(P8.Y, rz), a);
    fe_freeze(fe_mul(load_fe(r8 + 10), P8.Z), b);
    for (int q = 0; q < 8; q++) eq = eq && a[q] == b[q];
    return eq;
}

}  // namespace nwv
