// bls_verify.h -- the per-item steps of BLS12-381 min_sig verification,
// shared by the gfx950 kernels (bls_kernels.hip) and the CPU test build (tests/hostemu).
//
// An item is fastcrypto's AggregateAuthenticator::verify (types/src/primary.rs:531-534) =
// blst fast_aggregate_verify(sig, pks, msg): the aggregate signature decodes and lies in G1, the
// public keys (decoded and validated once, as fastcrypto does at deserialisation) are summed,
// the sum is not the identity, and e(-sig, g2) e(H(msg), apk) = 1.  Verifier::verify
// (Header::verify :179-182, Vote::verify :325-327) is the one-key case.  Status codes are the
// oracle's (oracle/bls_oracle.h ORB_*), checked in its order.
#pragma once
#include "bls_group.h"
#include "bls_wave.h"

namespace bls {

// device records (u32 words, Montgomery limbs)
constexpr int G1_REC_WORDS = 2 * NL + 1;   // x, y, flags (bit 0 = identity)
constexpr int G2_REC_WORDS = 4 * NL + 1;   // x.c0, x.c1, y.c0, y.c1, flags

NWV_HD void st_g1(uint32_t* o, const fp& x, const fp& y, bool inf) {
    st_fp(o, x);
    st_fp(o + NL, y);
    o[2 * NL] = inf ? 1u : 0u;
}
NWV_HD void st_g2(uint32_t* o, const fp2& x, const fp2& y, bool inf) {
    st_fp(o, x.c0);
    st_fp(o + NL, x.c1);
    st_fp(o + 2 * NL, y.c0);
    st_fp(o + 3 * NL, y.c1);
    o[4 * NL] = inf ? 1u : 0u;
}
NWV_HD void ld_g2(const uint32_t* o, fp2& x, fp2& y) {
    x.c0 = ld_fp(o);
    x.c1 = ld_fp(o + NL);
    y.c0 = ld_fp(o + 2 * NL);
    y.c1 = ld_fp(o + 3 * NL);
}

// a public key as fastcrypto deserialises and blst validates it: decodes, is not the identity,
// lies in G2
NWV_HD int32_t key_decode(const uint8_t* pk96, uint32_t* rec) {
    fp2 x, y;
    bool inf;
    int32_t st = g2_decompress(x, y, inf, pk96);
    if (st == ST_OK && inf) st = ST_PK_INFINITY;
    if (st == ST_OK && !g2_in_group(x, y)) st = ST_NOT_IN_GROUP;
    if (st != ST_OK) x = y = f2_zero();
    st_g2(rec, x, y, st != ST_OK);
    return st;
}
// a signature: decodes; unless it is the identity it lies in G1 (blst sig_groupcheck)
NWV_HD int32_t sig_decode(const uint8_t* sig48, uint32_t* rec) {
    fp x, y;
    bool inf;
    int32_t st = g1_decompress(x, y, inf, sig48);
    if (st == ST_OK && !inf && !g1_in_group(x, y)) st = ST_NOT_IN_GROUP;
    if (st != ST_OK || inf) x = y = fp_zero();
    st_g1(rec, x, y, inf);
    return st;
}
// H(msg) as an affine record
NWV_HD void h2c_record(const uint8_t* msg, uint32_t n, const uint8_t* dst, uint32_t dl, uint32_t* rec) {
    const jac<fp> h = hash_to_g1(msg, n, dst, dl);
    fp x = fp_zero(), y = fp_zero();
    if (!h.inf) g1_to_affine(x, y, h);
    st_g1(rec, x, y, h.inf);
}
// apk = sum of the item's keys (records of validated keys), affine; status as the oracle orders it
NWV_HD int32_t apk_record(const uint32_t* key_recs, const int32_t* key_status, const uint32_t* idx, uint32_t cnt,
                          uint32_t* rec) {
    if (cnt == 0) {
        st_g2(rec, f2_zero(), f2_zero(), true);
        return ST_AGGR_MISMATCH;
    }
    jac<fp2> acc;
    acc.inf = true;
    acc.x = acc.y = acc.z = f2_zero();
    for (uint32_t i = 0; i < cnt; i++) {
        const uint32_t k = idx[i];
        if (key_status[k] != ST_OK) {
            st_g2(rec, f2_zero(), f2_zero(), true);
            return key_status[k];
        }
        fp2 x, y;
        ld_g2(key_recs + (size_t)k * G2_REC_WORDS, x, y);
        acc = jac_add(acc, jac_from_affine(x, y));
    }
    fp2 x = f2_zero(), y = f2_zero();
    if (!acc.inf) g2_to_affine(x, y, acc);
    st_g2(rec, x, y, acc.inf);
    return acc.inf ? ST_PK_INFINITY : ST_OK;
}
// e(-sig, g2) e(H, apk) == 1 (an identity signature contributes e(O, g2) = 1)
NWV_HD bool pairing_check(const uint32_t* sig_rec, const uint32_t* h_rec, const uint32_t* apk_rec) {
    fp px[2], py[2];
    fp2 qx[2], qy[2];
    int n = 0;
    if (!sig_rec[2 * NL]) {
        px[n] = ld_fp(sig_rec);
        py[n] = fp_neg(ld_fp(sig_rec + NL));
        qx[n] = k_g2x();
        qy[n] = k_g2y();
        n++;
    }
    if (!h_rec[2 * NL]) {
        px[n] = ld_fp(h_rec);
        py[n] = ld_fp(h_rec + NL);
        ld_g2(apk_rec, qx[n], qy[n]);
        n++;
    }
    return f12_is_one(final_exp(miller_loop2(n, px, py, qx, qy)));
}

// ---- the batch check: a random linear combination over a call's items -----------------------
// Every item i that decoded and passed the group checks carries a 64-bit coefficient r_i (odd, so
// nonzero: blst's own multi-verification draws 64-bit coefficients too); the call accepts iff
//   prod_i e([r_i] H_i, apk_i) * e(-sum_i [r_i] sig_i, g2) == 1,
// computed in stages: every item's [r_i] H_i and [r_i] sig_i; the G1 sum S of the latter (a
// tree); the Miller loops of ([r_i] H_i, apk_i) and of (-S, g2), all in one grid; a product tree;
// ONE final exponentiation.  H_i, sig_i lie in G1 and apk_i in G2 (prime order r), so an invalid item makes
// the product differ from 1 except with probability ~2^-63 over the coefficients; when it is not
// 1 the engine runs the per-item check (pairing_check) to name the failing items exactly.
constexpr int F12_REC_WORDS = 12 * NL;     // Fp12, tower order c0.c0.c0 .. c1.c2.c1
constexpr int G1J_REC_WORDS = 3 * NL + 1;  // Jacobian X, Y, Z, flags (bit 0 = identity)

NWV_HD void st_f12(uint32_t* o, const fp12& e) {
    const fp* c[12] = {&e.c0.c0.c0, &e.c0.c0.c1, &e.c0.c1.c0, &e.c0.c1.c1, &e.c0.c2.c0, &e.c0.c2.c1,
                       &e.c1.c0.c0, &e.c1.c0.c1, &e.c1.c1.c0, &e.c1.c1.c1, &e.c1.c2.c0, &e.c1.c2.c1};
    for (int k = 0; k < 12; k++) st_fp(o + NL * k, *c[k]);
}
NWV_HD fp12 ld_f12(const uint32_t* o) {
    fp12 e;
    fp* c[12] = {&e.c0.c0.c0, &e.c0.c0.c1, &e.c0.c1.c0, &e.c0.c1.c1, &e.c0.c2.c0, &e.c0.c2.c1,
                 &e.c1.c0.c0, &e.c1.c0.c1, &e.c1.c1.c0, &e.c1.c1.c1, &e.c1.c2.c0, &e.c1.c2.c1};
    for (int k = 0; k < 12; k++) *c[k] = ld_fp(o + NL * k);
    return e;
}
NWV_HD void st_g1j(uint32_t* o, const jac<fp>& p) {
    st_fp(o, p.x);
    st_fp(o + NL, p.y);
    st_fp(o + 2 * NL, p.z);
    o[3 * NL] = p.inf ? 1u : 0u;
}
NWV_HD jac<fp> ld_g1j(const uint32_t* o) {
    jac<fp> p;
    p.x = ld_fp(o);
    p.y = ld_fp(o + NL);
    p.z = ld_fp(o + 2 * NL);
    p.inf = o[3 * NL] != 0;
    return p;
}

// r_i = the first 8 bytes of SHA-256(seed || i_be32), forced odd
NWV_HD uint64_t rlc_scalar(const uint8_t* seed32, uint32_t i) {
    uint32_t h[8], blk[16];
    sha256_iv(h);
    for (int k = 0; k < 8; k++)
        blk[k] = ((uint32_t)seed32[4 * k] << 24) | ((uint32_t)seed32[4 * k + 1] << 16) |
                 ((uint32_t)seed32[4 * k + 2] << 8) | (uint32_t)seed32[4 * k + 3];
    blk[8] = i;
    blk[9] = 0x80000000u;  // padding after the 36 message bytes
    for (int k = 10; k < 15; k++) blk[k] = 0;
    blk[15] = 36 * 8;
    sha256_block(h, blk);
    return (((uint64_t)h[0] << 32) | h[1]) | 1u;
}

// ---- the same checks over a group of lanes (bls_group.h): what the kernels run --------------
// e(-sig, g2) e(H, apk) == 1 (pairing_check), every lane of the group gets the verdict
G_HD bool g_pairing_check(const GCtx& g, const uint32_t* sig_rec, const uint32_t* h_rec, const uint32_t* apk_rec) {
    fp px[2], py[2];
    fp2 qx[2], qy[2];
    int n = 0;
    if (!sig_rec[2 * NL]) {
        px[n] = ld_fp(sig_rec);
        py[n] = fp_neg(ld_fp(sig_rec + NL));
        qx[n] = k_g2x();
        qy[n] = k_g2y();
        n++;
    }
    if (!h_rec[2 * NL]) {
        px[n] = ld_fp(h_rec);
        py[n] = ld_fp(h_rec + NL);
        ld_g2(apk_rec, qx[n], qy[n]);
        n++;
    }
    const G12 f = n == 2 ? g_miller<2>(g, px, py, qx, qy)
                : n == 1 ? g_miller<1>(g, px, py, qx, qy) : g_one(g);
    return g_is_one(g, g_final_exp(g, f));
}

// stage 1, item i (one group): P_i = [r] H (affine record, identity flag) and s_i = [r] sig
// (Jacobian).  On the GPU the two scalar multiplications run side by side: lanes 0-3 take [r] H,
// lanes 4-7 [r] sig; lane 0 stores P_i, lane 4 s_i.
G_HD void g_rlc_points(const GCtx& g, const uint32_t* sig_rec, const uint32_t* h_rec, uint64_t r, uint32_t* p_out,
                       uint32_t* s_out) {
    jac<fp> inf;
    inf.inf = true;
    inf.x = inf.y = inf.z = fp_zero();
#ifdef BLS_GDEV
    const bool sig_lane = (g.slot & 4) != 0;
    const uint32_t* src = sig_lane ? sig_rec : h_rec;
    jac<fp> m = inf;
    if (!src[2 * NL]) m = jac_mul64(jac_from_affine(ld_fp(src), ld_fp(src + NL)), r);
    if (g.slot == 4) st_g1j(s_out, m);
    if (g.slot == 0) st_g1j(p_out, m);  // Jacobian: no inversion (g_rlc_ml)
#else
    jac<fp> s = inf, h = inf;
    if (!sig_rec[2 * NL]) s = jac_mul64(jac_from_affine(ld_fp(sig_rec), ld_fp(sig_rec + NL)), r);
    if (!h_rec[2 * NL]) h = jac_mul64(jac_from_affine(ld_fp(h_rec), ld_fp(h_rec + NL)), r);
    st_g1j(s_out, s);
    st_g1j(p_out, h);
#endif
}
// an item outside the batch (failed an earlier check): identity P_i, s_i
G_HD void g_rlc_neutral(const GCtx& g, uint32_t* p_out, uint32_t* s_out) {
    jac<fp> s;
    s.inf = true;
    s.x = s.y = s.z = fp_zero();
#ifdef BLS_GDEV
    if (g.slot != 0) return;
#endif
    st_g1j(s_out, s);
    st_g1j(p_out, s);
}
// stage 3: f = the Miller loop of (P, Q) in W order, 1 for an identity P; P a Jacobian record
// (X, Y, Z), Q = apk (affine record) or g2 for the combination's signature side.  With
// x_P = X / Z^2, y_P = Y / Z^3 every line is evaluated times Z^3 (l0 Z^3 + l1 X Z v + l4 Y v w):
// f picks up a factor in Fp*, which the final exponentiation maps to 1, and no P is inverted.
G_HD void g_rlc_ml(const GCtx& g, const uint32_t* p_rec, const uint32_t* apk_rec, uint32_t* f_out) {
    G12 f = g_one(g);
    const jac<fp> P = ld_g1j(p_rec);
    if (!P.inf) {
        const fp px = fp_mul(P.x, P.z), py = P.y, z3 = fp_mul(fp_sqr(P.z), P.z);
        fp2 qx, qy;
        ld_g2(apk_rec, qx, qy);
        f = g_miller<1, true>(g, &px, &py, &qx, &qy, &z3);
    }
    g_store(g, f_out, f);
}
// the combination's signature side as one more item: P = -S (affine record) and Q = g2, so the
// Miller-loop grid runs one code path on every group (a different path on one group of a wave
// would serialise the wave: measured 2x)
NWV_HD void rlc_sig_item(const uint32_t* s_rec, uint32_t* p_out, uint32_t* q_out) {
    jac<fp> S = ld_g1j(s_rec);
    S.y = fp_neg(S.y);  // -S, still Jacobian (g_rlc_ml)
    st_g1j(p_out, S);
    st_g2(q_out, k_g2x(), k_g2y(), false);
}
// the trees: f_a <- f_a f_b (a group), s_a <- s_a + s_b (a lane)
G_HD void g_rlc_ffold(const GCtx& g, uint32_t* fa, const uint32_t* fb) {
    const G12 f = g_mul(g, g_load(g, fa), g_load(g, fb));
    g_store(g, fa, f);
}
NWV_HD void rlc_sfold(uint32_t* sa, const uint32_t* sb) { st_g1j(sa, jac_add(ld_g1j(sa), ld_g1j(sb))); }
// stage 5: the batch verdict, FE(f) == 1
G_HD bool g_rlc_final(const GCtx& g, const uint32_t* f_rec) { return g_is_one(g, g_final_exp(g, g_load(g, f_rec))); }

// ---- the same check on one whole wave (bls_wave.h) -------------------------------------------
// the line table of an affine Q (a G2 record): (l0, l1, l4) of every Miller-loop step, NSTEPS x 6
// slots of 14 words -- what the loop computes from T when no table is given
// (the steps alone: QB holds Q with Z = 1)
template <class W>
NWV_HD void w_key_lines_steps(const W& w, uint32_t* out) {
    using namespace wave;
    w.put_words(REG_TB, w.wm + SW * REG_QB, 6);
    w.sync();
    const char* steps = BLS_WAVE_STEPS_STR;
#pragma unroll 1
    for (int k = 0; k < NSTEPS; k++) {
        w.run(steps[k] == 'a' ? P_LINES_ADD : P_LINES_DBL);
        w.get_words(REG_LB, out + (size_t)k * 6 * SW, 6);
        w.sync();
    }
}
template <class W>
NWV_HD void w_key_lines(const W& w, const uint32_t* q_rec, uint32_t* out) {
    using namespace wave;
    init_slots(w);
    w.zero(REG_QB, 6);
    w.sync();
    w.put_words(REG_QB, q_rec, 4);
    w.put_fp(REG_QB + 4, k_one());
    w.sync();
    w_key_lines_steps(w, out);
}
// The fill of an aggregate-key ring slot (bls_apk_ring.h) on a wave: a key-side item's Jacobian
// key sum (blsw_apk_item's record: the sum of its keys' [h_eff] pk records) made affine with one
// Fp2 inversion -- every lane forms the norm, the wave inverts it -- written to `rec` as a G2
// record with canonical limbs (one sum, one record, by whichever route it was added up), and that
// point's line table to `lines`: what registration keeps for one key (k_bls_key_heff,
// k_blsw_key_lines), for the set.  st: the item's key status; a sum that is not OK (a bad key, the
// identity) is not handed on: nothing is written and false comes back.
template <class W>
NWV_HD bool w_apk_fill(const W& w, const uint32_t* aj, int32_t st, uint32_t* rec, uint32_t* lines) {
    using namespace wave;
    if (st != ST_OK || aj[6 * NL] != 0) return false;
    const fp2 X = ld_f2(aj), Y = ld_f2(aj + 2 * NL), Z = ld_f2(aj + 4 * NL);
    const fp n = w.inv(fp_add(fp_sqr(Z.c0), fp_sqr(Z.c1)));
    const fp2 zi = {fp_mul(Z.c0, n), fp_neg(fp_mul(Z.c1, n))}, zi2 = f2_sqr(zi);
    fp2 x = f2_mul(X, zi2), y = f2_mul(Y, f2_mul(zi2, zi));
    x.c0 = fp_canon(x.c0);
    x.c1 = fp_canon(x.c1);
    y.c0 = fp_canon(y.c0);
    y.c1 = fp_canon(y.c1);
    w.lanes(1, [&](int) { st_g2(rec, x, y, false); });
    init_slots(w);
    w.zero(REG_QB, 6);
    w.sync();
    w.put_fp(REG_QB, x.c0);
    w.put_fp(REG_QB + 1, x.c1);
    w.put_fp(REG_QB + 2, y.c0);
    w.put_fp(REG_QB + 3, y.c1);
    w.put_fp(REG_QB + 4, k_one());
    w.sync();
    w_key_lines_steps(w, lines);
    return true;
}

// e(-sig, g2) e(H, apk) == 1 from the item's records (sig, H affine G1 records, apk an affine G2
// record); qlines = apk's precomputed line table (a cached key) or null.  The identity signature
// enters as P = (0, 0): its lines reduce to their l0 in Fp2, which the final exponentiation maps
// to 1 (e(O, g2) = 1); every l0 of g2's table is nonzero (checked by the generator).
template <class W>
NWV_HD bool w_pairing_check(const W& w, const uint32_t* sig_rec, const uint32_t* h_rec, const uint32_t* apk_rec,
                            const uint32_t* qlines) {
    using namespace wave;
    init_slots(w);
    w.zero(REG_PA, 2);
    w.zero(REG_PB, 3);
    w.zero(REG_QB, 6);
    w.sync();
    if (!sig_rec[2 * NL]) {
        w.put_words(REG_PA, sig_rec, 1);
        w.put_fp(REG_PA + 1, fp_neg(ld_fp(sig_rec + NL)));
    }
    if (!h_rec[2 * NL]) w.put_words(REG_PB, h_rec, 2);
    w.put_fp(REG_PB + 2, k_one());
    w.put_words(REG_QB, apk_rec, 4);
    w.put_fp(REG_QB + 4, k_one());
    w.sync();
    return wave::pairing_check(w, qlines);
}

// H(msg) on a wave: lanes 0 and 1 each expand the message and map u_0 / u_1 with SSWU (x as a
// fraction: no inversion); the two isogeny maps (homogeneous), their sum and [h_eff] run as
// stage programs.  out: X, Y, Z (x = X / Z, y = Y / Z) and an identity flag (3 NL + 1 words).
constexpr int G1H_REC_WORDS = 3 * NL + 1;
// U as a homogeneous record: X, Y, Z and the identity flag
template <class W>
NWV_HD void w_g1h_store(const W& w, uint32_t* out) {
    using namespace wave;
    w.get_words(REG_U, out, 3);
    w.sync();
    const bool inf = fp_is_zero(w.get(REG_U + 2));
    w.lanes(1, [&](int) { out[3 * NL] = inf ? 1u : 0u; });
}
// raw_out (optional): the RAW record, the sum of the two maps before [h_eff], written before the
// chain runs -- what the message ring keeps (with clear = false it equals `out`)
template <class W>
NWV_HD void w_hash_to_g1(const W& w, const uint8_t* msg, uint32_t n, const uint8_t* dst, uint32_t dl, uint32_t* out,
                         bool clear = true, uint32_t* raw_out = nullptr) {
    using namespace wave;
    init_slots(w);
    w.lanes(2, [&](int j) {
        uint32_t uw[32];
        expand_xmd_128w(uw, msg, n, dst, dl);
        const fp u0 = fp_from_be64w(uw), u1 = fp_from_be64w(uw + 16);  // constant offsets, then a select
        fp xn, xd, y;
        map_sswu_frac(xn, xd, y, fp_sel(j == 0, u0, u1));
        w.set(REG_S + 3 * j, xn);
        w.set(REG_S + 3 * j + 1, xd);
        w.set(REG_S + 3 * j + 2, y);
    });
    w.sync();
    w.run(P_ISO2_ADD);
    if (raw_out) {
        w_g1h_store(w, raw_out);
        w.sync();
    }
    if (clear) g1_chain(w, BLS_H_EFF);  // (else U holds the sum of the two maps)
    w_g1h_store(w, out);
}
// [h_eff] of a stored raw record (w_hash_to_g1's raw_out): the chain alone, out as
// w_hash_to_g1(clear = true) writes it
template <class W>
NWV_HD void w_g1_clear_raw(const W& w, const uint32_t* raw, uint32_t* out) {
    using namespace wave;
    init_slots(w);
    w.put_words(REG_U, raw, 3);
    w.put_words(REG_V, raw, 3);
    w.sync();
    g1_chain(w, BLS_H_EFF);
    w_g1h_store(w, out);
}
// The hash role of one item of a call that uses the message ring (k_blsw_pre_r).  src: the ring
// record of the item's message, or null (a miss); pub: the ring record a miss also fills, or null;
// key_side: the item takes the raw form (its keys carry h_eff), else the cleared one.
//   hit,  key side : out <- the record            hit,  else : out <- [h_eff] record
//   miss, key side : out <- raw (pub <- raw)      miss, else : pub <- raw, then out <- [h_eff] raw
template <class W>
NWV_HD void w_hash_ring_item(const W& w, const uint8_t* msg, uint32_t n, const uint8_t* dst, uint32_t dl,
                             const uint32_t* src, uint32_t* pub, bool key_side, uint32_t* out) {
    if (!src) {
        w_hash_to_g1(w, msg, n, dst, dl, out, !key_side, pub);
        return;
    }
    if (key_side)
        w.lanes(64, [&](int j) {
            for (int t = j; t < G1H_REC_WORDS; t += 64) out[t] = src[t];
        });
    else
        w_g1_clear_raw(w, src, out);
}

// the signature's G1 membership on a wave (sig_decode's g1_in_group): [x^2] P = -phi(P) with
// complete formulas; P = the affine record (not the identity)
template <class W>
NWV_HD bool w_g1_in_group(const W& w, const uint32_t* rec) {
    using namespace wave;
    init_slots(w);
    w.put_words(REG_V, rec, 2);
    w.put_words(REG_U, rec, 2);
    w.put_words(REG_S, rec, 2);
    w.put_fp(REG_V + 2, k_one());
    w.put_fp(REG_U + 2, k_one());
    w.sync();
    g1_chain(w, BLS_X_ABS);
    w.run(P_COPY_U_TO_V);
    g1_chain(w, BLS_X_ABS);
    w.run(P_G1_PHI_CHECK);
    return fp_is_zero(w.get(REG_S + 2)) && fp_is_zero(w.get(REG_S + 3));
}

// the general form: H as an affine record (G1_REC_WORDS) or w_hash_to_g1's homogeneous one
// (h_hom), apk as an affine G2 record or a Jacobian one (X, Y, Z; q_jac: k_blsw_apk's)
template <class W>
NWV_HD bool w_pairing_check_g(const W& w, const uint32_t* sig_rec, const uint32_t* h_rec, bool h_hom,
                              const uint32_t* q_rec, bool q_jac, const uint32_t* qlines, bool pc_bank = false) {
    using namespace wave;
    if (pc_bank) init_slots_pc(w);  // a bank of NSLOTS_PC slots (the packed kernel's)
    else init_slots(w);
    w.zero(REG_PA, 2);
    w.zero(REG_PB, 3);
    w.zero(REG_QB, 6);
    w.sync();
    if (!sig_rec[2 * NL]) {
        w.put_words(REG_PA, sig_rec, 1);
        w.put_fp(REG_PA + 1, fp_neg(ld_fp(sig_rec + NL)));
    }
    const bool h_inf = h_rec[(h_hom ? 3 : 2) * NL] != 0;
    if (!h_inf) w.put_words(REG_PB, h_rec, h_hom ? 3 : 2);  // H = O (never from a hash): only l0 remain
    if (h_inf || !h_hom) w.put_fp(REG_PB + 2, k_one());
    w.put_words(REG_QB, q_rec, q_jac ? 6 : 4);
    if (!q_jac) w.put_fp(REG_QB + 4, k_one());
    w.sync();
    return wave::pairing_check(w, qlines, !pc_bank);  // a PC bank holds the one-step programs only
}
// w_pairing_check with H in homogeneous coordinates (w_hash_to_g1's record)
template <class W>
NWV_HD bool w_pairing_check_h(const W& w, const uint32_t* sig_rec, const uint32_t* hh_rec, const uint32_t* apk_rec,
                              const uint32_t* qlines) {
    return w_pairing_check_g(w, sig_rec, hh_rec, true, apk_rec, false, qlines);
}

// ---- the batch check on the wave engine: one final exponentiation per GROUP of items ----------
// A large call's OK-status items are split into consecutive groups; group g accepts iff
//   (prod_{i in g} f([r_i] H_i, apk_i)) f(-S_g, g2), S_g = sum_{i in g} [r_i] sig_i,
// raised to the final exponent is 1 (f = the Miller loop alone, wave::miller_script; r_i =
// rlc_scalar).  Stages: wb_points per item (a lane for each of the two); a per-group tree of rlc_sfold;
// wb_sig_item per group; the Miller loops of the n items and of one signature item per group on
// the packed wave kernel; w_ffold_step trees over the F records; w_group_final on each group's
// last wave.  An item outside the batch (a failed status, an identity signature) enters with
// neutral points and its F record is written as 1.
//
// An F record: the 12 F slots as the wave holds them, then the number of Miller outputs folded
// into it (1 from a Miller wave whose script ran, 0 otherwise), then a pad word.  A group's last
// wave accepts only when that count is the group's items + 1, so a Miller launch that found no
// script or a tree level that did not run rejects the group.
constexpr int FB_REC_WORDS = 12 * NL + 2;
constexpr int G2J_REC_WORDS = 6 * NL + 1;  // a Jacobian G2 record: X, Y, Z (Fp2 each), identity flag
constexpr uint32_t WB_FAN = 17;  // records one wave multiplies at a tree level (16 items + their signature item)

// item i's points: p_out = [r] H as a homogeneous record (X Z, Y, Z^3 of the Jacobian multiple: the
// form pair_flat takes with h_hom, no inversion), s_out = [r] sig (Jacobian record).  The two
// multiplications are independent: the kernel gives each a lane of its own.
// a Jacobian point as that homogeneous record; the identity as the neutral record
NWV_HD void wb_store_hom(uint32_t* p_out, const jac<fp>& h) {
    if (h.inf) {
        st_g1j(p_out, h);
        return;
    }
    st_fp(p_out, fp_mul(h.x, h.z));
    st_fp(p_out + NL, h.y);
    st_fp(p_out + 2 * NL, fp_mul(fp_sqr(h.z), h.z));
    p_out[3 * NL] = 0u;
}
NWV_HD void wb_point_h(const uint32_t* h_rec, uint64_t r, uint32_t* p_out) {
    jac<fp> h;
    h.inf = true;
    h.x = h.y = h.z = fp_zero();
    if (!h_rec[2 * NL]) h = jac_mul64(jac_from_affine(ld_fp(h_rec), ld_fp(h_rec + NL)), r);
    if (h.inf) {
        st_g1j(p_out, h);
        return;
    }
    st_fp(p_out, fp_mul(h.x, h.z));
    st_fp(p_out + NL, h.y);
    st_fp(p_out + 2 * NL, fp_mul(fp_sqr(h.z), h.z));
    p_out[3 * NL] = 0u;
}
NWV_HD void wb_point_s(const uint32_t* sig_rec, uint64_t r, uint32_t* s_out) {
    jac<fp> s;
    s.inf = true;
    s.x = s.y = s.z = fp_zero();
    if (!sig_rec[2 * NL]) s = jac_mul64(jac_from_affine(ld_fp(sig_rec), ld_fp(sig_rec + NL)), r);
    st_g1j(s_out, s);
}
NWV_HD void wb_points(const uint32_t* sig_rec, const uint32_t* h_rec, uint64_t r, uint32_t* p_out, uint32_t* s_out) {
    wb_point_h(h_rec, r, p_out);
    wb_point_s(sig_rec, r, s_out);
}
// an item outside the batch: identity on both sides (g_rlc_neutral's records; G1J_REC_WORDS =
// G1H_REC_WORDS, the flag in the last word)
NWV_HD void wb_neutral_rec(uint32_t* out) {
    jac<fp> s;
    s.inf = true;
    s.x = s.y = s.z = fp_zero();
    st_g1j(out, s);
}
NWV_HD void wb_neutral(uint32_t* p_out, uint32_t* s_out) {
    wb_neutral_rec(s_out);
    wb_neutral_rec(p_out);
}
static_assert(G1J_REC_WORDS == 3 * NL + 1, "a neutral Jacobian record is a neutral homogeneous one");
// an identity signature's item stays out of the batch: its equation is e(H, apk) == 1 with apk of
// order r, which holds only when H's G1 component is the identity -- H itself, or [h_eff] H0 for
// a key-side item (kmode: h_rec holds H0)
NWV_HD bool wb_identity_sig_holds(const uint32_t* h_rec, bool kmode) {
    if (h_rec[2 * NL]) return true;
    if (!kmode) return false;
    return jac_mul64(jac_from_affine(ld_fp(h_rec), ld_fp(h_rec + NL)), BLS_H_EFF).inf;
}
// group g's signature item: S_g (the group's first Jacobian record after the tree) as an affine
// signature record (the Miller kernel pairs -S_g with g2 as it pairs -sig), identity on its hash
// side, g2 as the Q of its unused pair
NWV_HD void wb_sig_item(const uint32_t* s_rec, uint32_t* sg_out, uint32_t* p_out, uint32_t* q_out) {
    const jac<fp> S = ld_g1j(s_rec);
    fp x = fp_zero(), y = fp_zero();
    if (!S.inf) g1_to_affine(x, y, S);
    st_g1(sg_out, x, y, S.inf);
    jac<fp> o;
    o.inf = true;
    o.x = o.y = o.z = fp_zero();
    st_g1j(p_out, o);
    const fp2 gx = k_g2x(), gy = k_g2y();
    st_fp(q_out, gx.c0);
    st_fp(q_out + NL, gx.c1);
    st_fp(q_out + 2 * NL, gy.c0);
    st_fp(q_out + 3 * NL, gy.c1);
    st_fp(q_out + 4 * NL, k_one());
    st_fp(q_out + 5 * NL, fp_zero());
    q_out[6 * NL] = 0u;
}
// level h of a group's signature tree over its live entries [0, min(m, gsize)): entry j takes entry
// j + h, h = ceil(m / 2) (k_bls_sfold's shape, per group)
NWV_HD void wb_sfold(uint32_t* grp, uint32_t j, uint32_t m, uint32_t gsize) {
    const uint32_t h = (m + 1) / 2, live = m < gsize ? m : gsize;
    if (j < h && j + h < live) rlc_sfold(grp + (size_t)G1J_REC_WORDS * j, grp + (size_t)G1J_REC_WORDS * (j + h));
}
// one step of a group's product tree on a wave (a bank of NSLOTS_PC slots): F <- the product of
// the records at positions p0, p0 + s, ... below m, at most fan of them (the kernels: WB_FAN);
// at(p) = position p's record.  Returns the Miller outputs the product holds.
template <class W, class At>
NWV_HD uint32_t w_ffold_step(const W& w, At at, uint32_t p0, uint32_t s, uint32_t m, uint32_t fan) {
    using namespace wave;
    init_slots_pc(w);
    const uint32_t* r0 = at(p0);
    w.put_words(REG_F, r0, 12);
    uint32_t cnt = r0[12 * NL];
    w.sync();
    for (uint32_t q = 1; q < fan && p0 + q * s < m; q++) {
        const uint32_t* r = at(p0 + q * s);
        w.put_words(REG_B, r, 12);
        w.sync();
        w.run(P_MUL_F_B);
        cnt += r[12 * NL];
    }
    return cnt;
}
// a group's verdict from its whole product in F: conjugation, final exponentiation, == 1
template <class W>
NWV_HD bool w_group_final(const W& w) {
    using namespace wave;
    w.run(P_CONJ_F);
    final_exp(w);
    return w.f_is_one();
}

// ---- the key-transposed batch check (bls_key_batch.h): the same product regrouped
// by key.  Every item of a group over registered keys contributes [r_i] H_i (Jacobian, so it can be
// added: wb_point_s's form, on the hash record) once per occurrence of a key in its list to that
// key's T_k; group g accepts iff (prod_k f(T_k, [h_eff] pk_k)) f(-S_g, g2) raised to the final
// exponent is 1.  The Miller entries are those of the wave batch check: T_k as a homogeneous
// record against key k's line table, S_g's entry as wb_sig_item writes it.
//
// lane `lane` of `lanes`' share of a key's sum: the records of hj (G1J_REC_WORDS each) at
// cidx[lane], cidx[lane + lanes], ... below cnt, added in that order (jac_add: exact when two
// occurrences name one point, as an item that lists a key twice does)
NWV_HD jac<fp> kb_lane_sum(const uint32_t* hj, const uint32_t* cidx, uint32_t cnt, uint32_t lane, uint32_t lanes) {
    jac<fp> acc;
    acc.inf = true;
    acc.x = acc.y = acc.z = fp_zero();
    for (uint32_t c = lane; c < cnt; c += lanes) acc = jac_add(acc, ld_g1j(hj + (size_t)G1J_REC_WORDS * cidx[c]));
    return acc;
}
// a key entry's Q record (the form the key sums' records take): the key's affine [h_eff] pk with Z = 1
NWV_HD uint32_t kb_key_q_word(const uint32_t* key_rec, int wd) {
    const fp one = k_one();
    return wd < 4 * NL ? key_rec[wd] : wd < 5 * NL ? one.l[wd - 4 * NL] : 0u;
}

// ---- dense key sums of large calls (nwv_bls_set_apk_dense_min): `lanes` lanes per
// item (4, 8 or 16), each adding its stride of the item's keys' affine [h_eff] pk records into a
// Jacobian accumulator; the partial sums meet in a tree of log2 lanes levels (lane s < h takes lane
// s + h's, h = lanes / 2 .. 1).  An item over more than half of a wholly registered key table whose
// list is strictly ascending sums the ABSENT keys instead, found from the list's gaps, and takes
// total - that sum.
//
// mixed addition (madd-2007-bl: the second point affine, Z2 = 1) with jac_add's exceptional cases:
// exact for equal points (doubling) and opposite ones (the identity)
template <class F> BLS_NOINLINE jac<F> jac_add_affine(const jac<F>& a, const F& x2, const F& y2) {
    using O = ops<F>;
    if (a.inf) return jac_from_affine(x2, y2);
    const F z1z1 = O::sqr(a.z);
    const F u2 = O::mul(x2, z1z1), s2 = O::mul(O::mul(y2, a.z), z1z1);
    if (O::eq(a.x, u2)) {
        if (O::eq(a.y, s2)) return jac_dbl(a);
        jac<F> o = a;
        o.inf = true;
        return o;
    }
    const F h = O::sub(u2, a.x), hh = O::sqr(h);
    F i = O::add(hh, hh);
    i = O::add(i, i);
    const F j = O::mul(h, i);
    F rr = O::sub(s2, a.y);
    rr = O::add(rr, rr);
    const F v = O::mul(a.x, i);
    jac<F> o;
    o.inf = false;
    o.x = O::sub(O::sub(O::sub(O::sqr(rr), j), v), v);
    const F yj = O::mul(a.y, j);
    o.y = O::sub(O::mul(rr, O::sub(v, o.x)), O::add(yj, yj));
    o.z = O::sub(O::sub(O::sqr(O::add(a.z, h)), z1z1), hh);
    return o;
}
// the records a dense item's key numbers name: key number k of the call's table sits in cache slot
// ktab[k] (a slot below `cap`; anything else is a key the cache does not hold)
struct DenseKeys {
    const uint32_t* hrc;   // the cache's [h_eff] pk records (G2_REC_WORDS per slot)
    const int32_t* sc;     // the slots' statuses
    const uint32_t* ktab;  // the call's key table, n_keys entries
    uint32_t n_keys, cap;
};
NWV_HD jac<fp2> blsd_identity() {
    jac<fp2> a;
    a.inf = true;
    a.x = a.y = a.z = f2_zero();
    return a;
}
NWV_HD jac<fp2> blsd_add_key(const DenseKeys& t, const jac<fp2>& acc, uint32_t k) {
    fp2 x, y;
    ld_g2(t.hrc + (size_t)G2_REC_WORDS * t.ktab[k], x, y);
    return jac_add_affine(acc, x, y);
}
// the key table's total (k_blsd_total): lane `lane` of `lanes`' share, keys lane, lane + lanes, ...;
// ok turns false at a key that is not cached with status OK (the total is then not used)
NWV_HD jac<fp2> blsd_total_lane(const DenseKeys& t, uint32_t lane, uint32_t lanes, bool& ok) {
    jac<fp2> acc = blsd_identity();
    ok = true;
    for (uint32_t k = lane; k < t.n_keys; k += lanes) {
        const uint32_t s = t.ktab[k];
        if (s >= t.cap || t.sc[s] != ST_OK) {
            ok = false;
            break;
        }
        acc = blsd_add_key(t, acc, k);
    }
    return acc;
}
// this lane's positions of the list (key numbers idx[0 .. cnt)) each follow a smaller number: true
// in every lane of the item <=> the list is strictly ascending
NWV_HD bool blsd_lane_ascending(const uint32_t* idx, uint32_t cnt, uint32_t lane, uint32_t lanes) {
    for (uint32_t j = lane; j < cnt; j += lanes)
        if (j && idx[j - 1] >= idx[j]) return false;
    return true;
}
// the lane's share of the list summed directly, in list order (multiplicity kept); first_bad = the
// first of its positions whose key's status is not OK (the lane stops there), else 0xffffffff
NWV_HD jac<fp2> blsd_lane_direct(const DenseKeys& t, const uint32_t* idx, uint32_t cnt, uint32_t lane, uint32_t lanes,
                                 uint32_t& first_bad) {
    jac<fp2> acc = blsd_identity();
    first_bad = 0xffffffffu;
    for (uint32_t j = lane; j < cnt; j += lanes) {
        if (t.sc[t.ktab[idx[j]]] != ST_OK) {
            first_bad = j;
            break;
        }
        acc = blsd_add_key(t, acc, idx[j]);
    }
    return acc;
}
// the lane's share of the keys a strictly ascending list leaves out: the absent keys in ascending
// order, found from the list's gaps, are dealt to the lanes in turn (the r-th absent key to lane
// r % lanes).  One addition per trip of the outer loop: the walk to the lane's next key is index
// arithmetic only, so the lanes of a wave -- which hold different items -- run their additions
// together however their gaps differ.
NWV_HD jac<fp2> blsd_lane_absent(const DenseKeys& t, const uint32_t* idx, uint32_t cnt, uint32_t lane, uint32_t lanes) {
    jac<fp2> acc = blsd_identity();
    uint32_t k = 0, j = 0, rank = 0;  // the next key number, the next list position, absent keys passed
    for (;;) {
        uint32_t mine = 0xffffffffu;
        while (k < t.n_keys && mine == 0xffffffffu) {
            if (j < cnt && idx[j] == k) j++;
            else if (rank++ % lanes == lane) mine = k;
            k++;
        }
        if (mine == 0xffffffffu) break;
        acc = blsd_add_key(t, acc, mine);
    }
    return acc;
}
// lane 0's end of an item: the tree's sum (of the absent keys when comp: the item's sum is then
// total - it), the item's first bad position -> its status, with the record zeroed unless OK
NWV_HD int32_t blsd_finish(const DenseKeys& t, const uint32_t* idx, jac<fp2>& acc, bool comp, const jac<fp2>& total,
                           uint32_t first_bad) {
    if (comp) {
        acc.y = f2_neg(acc.y);
        acc = jac_add(total, acc);
    }
    int32_t status = ST_OK;
    if (first_bad != 0xffffffffu) status = t.sc[t.ktab[idx[first_bad]]];
    else if (acc.inf) status = ST_PK_INFINITY;
    if (status != ST_OK) acc = blsd_identity();
    return status;
}

// ---- AggregateAuthenticator::aggregate (types/src/primary.rs:476-477) on a wave: g1_sum16 adds
// G1SUM_N points with complete formulas (the identity and equal points need no branches); point k
// sits in slots g1sum_slot(k) + 0..2 as (X : Y : Z) and the sum lands in U
constexpr int G1P_WORDS = 3 * NL;  // a homogeneous partial sum (X, Y, Z)
// the smallest sum program over cnt points (1 <= cnt <= G1SUM_N) and its input count
NWV_HD uint32_t g1_sum_width(uint32_t cnt) { return cnt <= 2 ? 2u : cnt <= 4 ? 4u : cnt <= 8 ? 8u : 16u; }
NWV_HD wave::Prog g1_sum_prog(uint32_t cnt) {
    const uint32_t k = g1_sum_width(cnt);
    return k == 2 ? wave::P_G1_SUM2 : k == 4 ? wave::P_G1_SUM4 : k == 8 ? wave::P_G1_SUM8 : wave::P_G1_SUM16;
}
// points a wave takes at a level of m > G1SUM_N inputs
NWV_HD uint32_t g1_sum_per(uint32_t) { return (uint32_t)wave::G1SUM_N; }

// the program's inputs: affine records (hom = 0: G1_REC_WORDS each, identity flagged; record j at
// idx[j] when idx, else at j) or partial sums (hom = 1: G1P_WORDS each); inputs past m are the
// identity.  The caller has run init_slots (the one comes from its constant slot).
template <class W>
NWV_HD void w_g1_sum_put(const W& w, const uint32_t* in, const uint32_t* idx, int hom, uint32_t first, uint32_t m,
                         uint32_t width = wave::G1SUM_N) {
    using namespace wave;
    const uint32_t* one = w.wm + SW * SLOT_ONE;
    for (int k = 0; k < (int)width; k++) {
        const uint32_t j = first + (uint32_t)k;
        const int s = g1sum_slot(k);
        if (j < m && hom) {
            w.put_words(s, in + (size_t)G1P_WORDS * j, 3);
            continue;
        }
        const uint32_t* r = j < m ? in + (size_t)G1_REC_WORDS * (idx ? idx[j] : j) : nullptr;
        if (r && !r[2 * NL]) {
            w.put_words(s, r, 2);
            w.put_words(s + 2, one, 1);
        } else {
            w.zero(s, 3);
            w.sync();
            w.put_words(s + 1, one, 1);
        }
    }
    w.sync();
}

// U (the program's sum) -> the 48-byte compressed point, x = X / Z, y = Y / Z (every lane calls
// it: the inversion runs on the wave; lane 0 writes)
template <class W>
NWV_HD void w_g1_sum_compress(const W& w, uint8_t* out48) {
    using namespace wave;
    const fp X = w.get(REG_U), Y = w.get(REG_U + 1), Z = w.get(REG_U + 2);
    if (fp_is_zero(Z)) {
        if (w.lane == 0) g1_compress(out48, fp_zero(), fp_zero(), true);
        return;
    }
    const fp zi = w.inv(Z);
    if (w.lane == 0) g1_compress(out48, fp_mul(X, zi), fp_mul(Y, zi), false);
}

}  // namespace bls

