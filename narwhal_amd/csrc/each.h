// each.h -- lane and row pieces of the one-launch per-signature check for keys WITHOUT a comb
// table (each_kernels.hip k_ed_each_row): the exact ZIP-215 verdict on half-size scalars, as
// lane_straus_check_half (ed25519_lane.h) states it,
//     accept iff A and R decode, s < l and [8]([w]B - [m]R + [c u]A) = identity,
//     (u, v) = sc_half_split(k), m = |v|, w = m s mod l, c = -1 (v > 0) or +1 (v < 0),
// laid out for latency: one signature's variable-base Straus chain over R and A runs on the 16-lane
// rows of one wave (fe_row.h: a doubling or a cached addition in two row-product latencies) instead
// of on one lane, and [w]B comes from the device's fixed-base comb of B (msm.h) with no doublings.
// Everything here is __host__ __device__ and generic over fe_row.h's lane type: the kernel calls
// these functions and tests/hostemu/each_row_hostemu.cpp runs the same ones on the emulated wave.
#pragma once
#include "ed25519_lane.h"
#include "fe_row.h"
#include "msm.h"

namespace nwv {

// signed radix-16 digit positions of a half-size scalar (recode128: 132 bits)
static constexpr int EACH_DIGITS = 33;
// a point's table in LDS: entries 0..8 = identity, P, 2P, ..., 8P in cached row form (row 0 Y+X,
// row 1 Y-X, row 2 2dT, row 3 2Z: 64 words, word = lane, as row_add_cached reads them).  Only the
// positive multiples are stored; -Q is formed when an entry is loaded (each_entry).
static constexpr int EACH_ENTRIES = 9;
static constexpr int EACH_TABLE_WORDS = EACH_ENTRIES * 64;

// One signature's scalars from its challenge k (k < l) and s, by one lane: the coefficients of R
// (-m) and of A (c u) as EACH_DIGITS signed radix-16 digits each, top digit first (dr, da), and
// the comb digits of w = m s mod l (dw, msm.h comb_digits).  sok = s < l; an s >= l fails the
// signature and is zeroed before it becomes table indices.
NWV_HD void each_split_digits(const uint32_t k[8], const uint32_t Sw[8], bool sok, int* dr, int* da, int* dw) {
    uint32_t s[8], u[4], m[4], w[8], yu[5], ym[5];
    for (int q = 0; q < 8; q++) s[q] = sok ? Sw[q] : 0u;
    bool vneg;
    sc_half_split(k, u, m, vneg);
    const uint32_t m8[8] = {m[0], m[1], m[2], m[3], 0, 0, 0, 0};
    sc_mul(m8, s, w);
    recode128(u, yu, 4);
    recode128(m, ym, 4);
#pragma unroll 1
    for (int i = 0; i < EACH_DIGITS; i++) {
        const int du = take_top5(yu, 4);
        da[i] = vneg ? du : -du;      // A's coefficient: -u (v > 0) or +u (v < 0)
        dr[i] = -take_top5(ym, 4);    // R's coefficient: -m
    }
    comb_digits(w, dw);
}
// the same from the signature: k = SHA-512(R || A || M) mod l; returns s < l
NWV_HD bool each_scalars(const uint32_t Aw[8], const uint32_t Rw[8], const uint32_t Sw[8], const uint8_t* msg,
                         uint32_t mlen, int* dr, int* da, int* dw) {
    uint32_t k[8];
    const bool sok = lane_hash(Aw, Rw, Sw, msg, mlen, k) == FLAG_S_OK;
    each_split_digits(k, Sw, sok, dr, da, dw);
    return sok;
}

// Coordinate c (0 y+x, 1 y-x, 2 2dxy) of an MSM point record (msm.h msm_store_point: ten-limb
// words) as 16 canonical limbs: what row_decompress leaves for that coordinate, from the record a
// batch MSM's prep already stored (the reuse form, k_ed_each_row_msm)
NWV_HD void each_record_coord(const uint32_t* e, int c, uint32_t out[16]) { fe_to_limbs16(load_fe(e + 10 * c), out); }

// Digit position j's term of [w]B: entry |d| of table j of B's comb, with the sign of d
NWV_HD ge_p3 each_comb_term(const uint32_t* bcomb, int j, int d) {
    ge_p3 P = ge_p3_identity();
    if (d) {
        const int m = d < 0 ? -d : d;
        P = ge_p1p1_to_p3(ge_madd(P, msm_load_point(bcomb + MSM_PT_WORDS * (COMB_ENTRIES * j + m - 1), d < 0)));
    }
    return P;
}
// Row q (0 Y+X, 1 Y-X, 2 2dT, 3 2Z) of P's cached row form as 16 canonical limbs: the comb sum on
// its way from the ten-limb lane form to the layout the row wave adds
NWV_HD void each_cached_limbs(const ge_p3& P, int q, uint32_t out[16]) {
    const fe a = fe_select(fe_select(fe_select(fe_add(P.Z, P.Z), P.T, q == 2), fe_sub(P.Y, P.X), q == 1),
                           fe_add(P.Y, P.X), q == 0);
    fe_to_limbs16(fe_mul(fe_carry(a), fe_select(fe_one(), fe_d2(), q == 2)), out);
}

namespace rowf {

// cached row form of the identity: Y+X = Y-X = 1, 2dT = 0, 2Z = 2
NWV_HD V each_identity_cached(const RowConsts& k) {
    const V one = sel(limb_is(0), bc(0), bc(1));
    return rowsel(k, one, one, bc(0), one + one);
}

// Table of the point whose affine Niels record (y+x | y-x | 2dxy as 16-limb rows: 48 words, what
// row_decompress leaves) is at rec: entries 0..8 into tab (EACH_TABLE_WORDS words).  P itself is
// the record with 2Z = 2; 2P is one row doubling from (2x : 2y : 2), then j P = (j - 1) P + P,
// each turned into cached form by one row product (row_to_cached): 21 row products a table.
NWV_HD void each_build_table(const uint32_t* rec, uint32_t* tab, const RowConsts& k) {
    const V lane = lane_id() & 63u;
    const V limb = lane & 15u;
    const V one = sel(limb_is(0), bc(0), bc(1));
    const V ypx = ld(rec, limb), ymx = ld(rec, limb + bc(16)), t2d = ld(rec, limb + bc(32));
    st_all(tab, lane, each_identity_cached(k));
    const V q1 = rowsel(k, ypx, ymx, t2d, one + one);
    st_all(tab, lane + bc(64), q1);
    RowP3 d{carry32(sub(ypx, ymx, k), k), carry32(ypx + ymx, k), one + one, bc(0)};  // (T unused by a doubling)
    d = row_dbl(d, k);
    st_all(tab, lane + bc(128), row_to_cached(d, k));
#pragma unroll 1
    for (int j = 3; j < EACH_ENTRIES; j++) {
        d = row_add_cached(d, q1, k);
        st_all(tab, lane + bc(64u * (uint32_t)j), row_to_cached(d, k));
    }
    lds_order();
}

// Entry |d| of a table with the sign of d (-8 <= d <= 8; 0: the identity entry).  The negative of
// a cached point swaps Y+X and Y-X and negates 2dT: rows 0 and 1 read each other's words and row 2
// takes 8p - x, carried.  Selections only; the digit is wave-uniform.
NWV_HD V each_entry(const uint32_t* tab, int d, const RowConsts& k) {
    const bool neg = d < 0;
    const uint32_t m = (uint32_t)(neg ? -d : d);
    const V lane = lane_id() & 63u;
    const V limb = lane & 15u;
    const V swapped = rowsel(k, limb + bc(16), limb, limb + bc(32), limb + bc(48));
    const V v = ld(tab, (neg ? swapped : lane) + bc(64u * m));
    const V nv = carry32(sub(bc(0), v, k), k);
    return sel(neg ? k.r2 : row_is(4), v, nv);
}

// The Straus pass over the EACH_DIGITS digit positions of R's and A's coefficients, top first:
// four doublings, then one cached addition a point (a zero digit adds the identity entry)
NWV_HD RowP3 each_straus(const uint32_t* tab_r, const uint32_t* tab_a, const int* dr, const int* da,
                         const RowConsts& k) {
    const V one = sel(limb_is(0), bc(0), bc(1));
    RowP3 d{bc(0), one, one, bc(0)};
#pragma unroll 1
    for (int i = 0; i < EACH_DIGITS; i++) {
        if (i)
#pragma unroll 1
            for (int r = 0; r < 4; r++) d = row_dbl(d, k);
        d = row_add_cached(d, each_entry(tab_r, dr[i], k), k);
        d = row_add_cached(d, each_entry(tab_a, da[i], k), k);
    }
    return d;
}

// d + [w]B (wsum: its cached row form, 64 words), then [8]: row 0 writes X | Y | Z limbs to out[0, 48)
NWV_HD void each_finish(RowP3 d, const uint32_t* wsum, uint32_t* out, const RowConsts& k) {
    const V lane = lane_id() & 63u;
    const V limb = lane & 15u;
    d = row_add_cached(d, ld(wsum, lane), k);
#pragma unroll 1
    for (int r = 0; r < 3; r++) d = row_dbl(d, k);
    lds_order();
    const M r0 = row_is(0);
    st(out, limb, d.X, r0);
    st(out, limb + bc(16), d.Y, r0);
    st(out, limb + bc(32), d.Z, r0);
    lds_order();
}

}  // namespace rowf

// (X : Y : Z) from each_finish is the identity: X = 0 and Y = Z, on canonical limbs (one lane)
NWV_HD bool each_is_identity(const uint32_t* out) {
    const fe X = fe_from_limbs16(out), Y = fe_from_limbs16(out + 16), Z = fe_from_limbs16(out + 32);
    return fe_is_zero(X) && fe_is_zero(fe_sub(Y, Z));
}

}  // namespace nwv
