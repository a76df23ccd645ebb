// nwv_bls.hip -- BLS12-381 min_sig verification engine on gfx950: the
// kernels over bls_verify.h and the C ABI of include/nwv_bls.h.
//
// A call stages its inputs in one pinned arena and one H2D copy, then runs on three streams
//   k_bls_keys_fill  one lane per key the device's key cache has not seen: decode + G2 membership
//                    (psi(Q) = [x] Q), into the cache (fastcrypto validates a key once, at
//                    deserialization); then k_bls_apk_g, one 8-lane group per item: the sum of the
//                    item's keys (eight partial sums and a tree), its first bad key's status
//   k_bls_sigs       one lane per item: decode + G1 membership (phi(P) = [-x^2] P)
//   k_bls_h2c_g      one 8-lane group per item: H(msg) (RFC 9380 hash_to_curve G1), the two
//                    field elements mapped side by side
// joined by k_bls_status (the statuses in the oracle's order), then
//   the pairing check, by default as ONE batch check over the call (bls_verify.h, kernels below:
//     [r_i] H_i and [r_i] sig_i per item, S = sum [r_i] sig_i, every item's Miller loop and that
//     of (-S, g2) in one grid, a product tree, one final exponentiation)
//   and only when that rejects (or under NWV_FLAG_BLS_PER_ITEM)
//     k_bls_pair   one lane per item: e(-sig, g2) e(H, apk) == 1 (two-pair Miller loop + final exp)
// and copies the per-item statuses back.  The Miller loops are the hot part: Fp products on VALU
// v_mad_u64_u32 (bls381.h), no MFMA (no dense contraction).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/nwv.h"
#include "../../include/nwv_bls.h"
#include "bls_verify.h"
#include "bls_shard.h"
#include "bls_msg_ring.h"
#include "bls_apk_ring.h"
#include "bls_key_batch.h"
#include "bls_apk_dense.h"
#include "lane_pool.h"
#include "lane_stream.h"
#include "place.h"
#include "stage_args.h"

using namespace bls;
using nwv::bls_for_ranges;
using nwv::bls_shard_ranges;

__attribute__((visibility("hidden"))) int nwv_internal_set_err(int code, const char* msg);
extern "C" {  // defined in nwv_host.hip's extern "C" section
__attribute__((visibility("hidden"))) uint32_t nwv_internal_ctx_flags(const nwv_ctx* ctx);
__attribute__((visibility("hidden"))) nwv::PlaceTable* nwv_internal_place(nwv_ctx* ctx);
__attribute__((visibility("hidden"))) int nwv_internal_hip_device(const nwv_ctx* ctx, int i);
__attribute__((visibility("hidden"))) void nwv_internal_fill_seed(const uint8_t* seed32, uint8_t out[32]);
}

// ------------------------------------------------------------------------------ kernels
#define BLS_LANES 64
#define BLS_IDX() const uint32_t i = blockIdx.x * BLS_LANES + threadIdx.x; \
    if (i >= n) return

// decode + check keys: key j of the list goes to record slot slot[j] (the committee key cache at
// registration, or a call's scratch table for keys the cache does not hold)
__global__ __launch_bounds__(BLS_LANES) void k_bls_keys_fill(uint32_t n, const uint8_t* pk, const uint32_t* slot,
                                                             uint32_t* rec, int32_t* st) {
    BLS_IDX();
    const uint32_t k = slot[i];
    st[k] = key_decode(pk + 96 * (size_t)i, rec + (size_t)G2_REC_WORDS * k);
}
// copy validated records into the key cache: record src[j] of `from` -> slot dst[j] of `to`
__global__ __launch_bounds__(BLS_LANES) void k_bls_rec_copy(uint32_t n, const uint32_t* src, const uint32_t* dst,
                                                            const uint32_t* from, uint32_t* to, int32_t* to_st) {
    const uint32_t t = blockIdx.x * BLS_LANES + threadIdx.x;
    const uint32_t i = t / G2_REC_WORDS, w = t % G2_REC_WORDS;
    if (i >= n) return;
    to[(size_t)G2_REC_WORDS * dst[i] + w] = from[(size_t)G2_REC_WORDS * src[i] + w];
    if (w == 0) to_st[dst[i]] = ST_OK;
}
// A call's key table: index k < KC_CAP names slot k of the device's key cache, KC_CAP <= k < AR_BASE
// entry k - KC_CAP of the call's scratch table (keys the cache does not hold, decoded by this
// call: up to MAX_CALL_KEYS of them, far more than the cache has slots), k >= AR_BASE slot
// k - AR_BASE of the device's aggregate-key ring (a recurring signer set's key sum standing in as
// the one key of its item: always valid, an [h_eff]-side record with a line table of its own)
constexpr uint32_t KC_CAP = 65536;
constexpr uint32_t MAX_CALL_KEYS = 1u << 26;  // nwv_bls_verify_many's limit on n_keys (and on n)
constexpr uint32_t AR_BASE = 0x80000000u;
static_assert(KC_CAP + MAX_CALL_KEYS <= AR_BASE, "no scratch index reaches the ring's range");
constexpr uint32_t SC_CAP = 65536;  // the verified-signature ring (BlsSigCache)
struct KeyTab {
    const uint32_t* rc;
    const int32_t* sc;
    const uint32_t* rs;
    const int32_t* ss;
    const uint32_t* lines;  // cached keys' Miller-loop line tables (KL_WORDS per slot), or null
    const uint32_t* hrc;    // cached keys' [h_eff] pk records (G2_REC_WORDS per slot), or null
    const uint32_t* arr;    // the aggregate-key ring's records (G2_REC_WORDS per slot), or null
    const uint32_t* arl;    // the ring's line tables (KL_WORDS per slot), or null
};
// words of a registered key's line table: (l0, l1, l4) of every Miller-loop step (w_key_lines)
constexpr size_t KL_WORDS = (size_t)wave::NSTEPS * 6 * wave::SW;
__device__ inline const uint32_t* key_rec(const KeyTab& t, uint32_t k) {
    return k < KC_CAP    ? t.rc + (size_t)G2_REC_WORDS * k
           : k < AR_BASE ? t.rs + (size_t)G2_REC_WORDS * (k - KC_CAP)
                         : t.arr + (size_t)G2_REC_WORDS * (k - AR_BASE);
}
__device__ inline int32_t key_st(const KeyTab& t, uint32_t k) {
    return k < KC_CAP ? t.sc[k] : k < AR_BASE ? t.ss[k - KC_CAP] : ST_OK;
}
// the line table of a one-key, key-side item's key: a cache slot's or a ring slot's
__device__ inline const uint32_t* key_lines(const KeyTab& t, uint32_t k) {
    return k < AR_BASE ? t.lines + KL_WORDS * k : t.arl + KL_WORDS * (k - AR_BASE);
}
__global__ __launch_bounds__(BLS_LANES) void k_bls_sigs(uint32_t n, const uint8_t* sig, uint32_t* rec, int32_t* st) {
    BLS_IDX();
    st[i] = sig_decode(sig + 48 * (size_t)i, rec + (size_t)G1_REC_WORDS * i);
}
// the pairing kernels run one item per GROUP of 8 lanes (bls_group.h): 8 items per 64-lane block
#define BLS_GIDX()                                                                  \
    __shared__ uint32_t g_lds[(BLS_LANES / GRP) * GX_WORDS];                       \
    const GCtx g = g_ctx(g_lds);                                                    \
    const uint32_t i = blockIdx.x * (BLS_LANES / GRP) + threadIdx.x / GRP;          \
    if (i >= n) return

// the key sum of item i over a group: lane s adds the item's keys s, s + 8, ... (apk_record's
// formulas), the eight partial sums meet in a three-level tree through the group's LDS area, and
// the status is that of the item's FIRST bad key in list order (apk_record's), else identity ->
// PK_INFINITY.  st_apk[i] = the item's key status (the signature's status is combined later).
constexpr int G2J_WORDS = 6 * NL + 1;  // Jacobian X, Y, Z (Fp2 each), identity flag
__device__ void st_g2j(uint32_t* o, const jac<fp2>& p) {
    st_f2(o, p.x);
    st_f2(o + F2W, p.y);
    st_f2(o + 2 * F2W, p.z);
    o[3 * F2W] = p.inf ? 1u : 0u;
}
__device__ jac<fp2> ld_g2j(const uint32_t* o) {
    jac<fp2> p;
    p.x = ld_f2(o);
    p.y = ld_f2(o + F2W);
    p.z = ld_f2(o + 2 * F2W);
    p.inf = o[3 * F2W] != 0;
    return p;
}
static_assert(4 * G2J_WORDS + 8 <= GX_WORDS, "the tree's first level fits a group's LDS area");
__global__ __launch_bounds__(BLS_LANES) void k_bls_apk_g(uint32_t n, KeyTab kt, const uint32_t* pk_off,
                                                         const uint32_t* pk_cnt, const uint32_t* pk_idx, uint32_t* rec,
                                                         int32_t* st_apk) {
    BLS_GIDX();
    const uint32_t cnt = pk_cnt[i];
    const uint32_t* idx = pk_idx + pk_off[i];
    uint32_t* out = rec + (size_t)G2_REC_WORDS * i;
    if (cnt == 1) {  // one key (Verifier::verify): its validated record is the sum, no inversion
        if (g.slot < G2_REC_WORDS) {
            const uint32_t k = idx[0];
            const int32_t ks = key_st(kt, k);
            const uint32_t* kr = key_rec(kt, k);
            for (int w = g.slot; w < G2_REC_WORDS; w += GRP) out[w] = ks == ST_OK ? kr[w] : (w == 4 * NL ? 1u : 0u);
            if (g.slot == 0) st_apk[i] = ks;
        }
        return;
    }
    jac<fp2> acc;
    acc.inf = true;
    acc.x = acc.y = acc.z = f2_zero();
    uint32_t first_bad = 0xffffffffu;
    for (uint32_t j = (uint32_t)g.slot; j < cnt; j += GRP) {
        const uint32_t k = idx[j];
        if (key_st(kt, k) != ST_OK) {
            first_bad = j;
            break;
        }
        fp2 x, y;
        ld_g2(key_rec(kt, k), x, y);
        acc = jac_add(acc, jac_from_affine(x, y));
    }
    // the group's first bad position, and the tree over the partial sums
    uint32_t* xa = g.xa;
    g_sync();
    xa[4 * G2J_WORDS + g.slot] = first_bad;
#pragma unroll 1
    for (int h = GRP / 2; h >= 1; h /= 2) {
        g_sync();
        if (g.slot >= h && g.slot < 2 * h) st_g2j(xa + (g.slot - h) * G2J_WORDS, acc);
        g_sync();
        if (g.slot < h) acc = jac_add(acc, ld_g2j(xa + g.slot * G2J_WORDS));
    }
    g_sync();
    uint32_t fb = 0xffffffffu;
    for (int s2 = 0; s2 < GRP; s2++) fb = min(fb, xa[4 * G2J_WORDS + s2]);
    if (g.slot != 0) return;
    int32_t status;
    fp2 x = f2_zero(), y = f2_zero();
    bool inf = true;
    if (cnt == 0) {
        status = ST_AGGR_MISMATCH;
    } else if (fb != 0xffffffffu) {
        status = key_st(kt, idx[fb]);
    } else {
        if (!acc.inf) g2_to_affine(x, y, acc);
        inf = acc.inf;
        status = acc.inf ? ST_PK_INFINITY : ST_OK;
    }
    if (status != ST_OK) {
        x = y = f2_zero();
        inf = true;
    }
    st_g2(out, x, y, inf);
    st_apk[i] = status;
}
// H(msg_i) on a group: lanes 0-3 map hash_to_field's u_0, lanes 4-7 u_1 (side by side), lane 4
// hands its point to lane 0 through the group's LDS area, lane 0 adds and clears the cofactor
// (kmode[i] = 1: item i's cofactor clearing is on its key side -- H0 = the maps' sum, see
// k_bls_key_heff; kmode may be null)
__global__ __launch_bounds__(BLS_LANES) void k_bls_h2c_g(uint32_t n, const uint8_t* msg, const uint64_t* off,
                                                         const uint32_t* len, const uint8_t* dst, uint32_t dl,
                                                         uint32_t* rec, const uint32_t* kmode) {
    BLS_GIDX();
    const jac<fp> q = h2c_map(msg + off[i], len[i], dst, dl, (g.slot & 4) ? 1 : 0);
    g_sync();
    if (g.slot == 4) st_g1j(g.xa, q);
    g_sync();
    const jac<fp> q1 = ld_g1j(g.xa);
    if (g.slot != 0) return;
    const jac<fp> h0 = jac_add(q, q1);
    const jac<fp> h = kmode && kmode[i] ? h0 : jac_mul64(h0, BLS_H_EFF);
    fp x = fp_zero(), y = fp_zero();
    if (!h.inf) g1_to_affine_vt(x, y, h);
    st_g1(rec + (size_t)G1_REC_WORDS * i, x, y, h.inf);
}
// The same on a lane pair: lane 2 j maps u_0 and lane 2 j + 1 u_1 of item 32 b + j; the odd lane
// hands its point over through LDS.  32 items a wave instead of 8: a 16,384-item call is 512 waves
// (one per SIMD at most) instead of 2,048 (two per SIMD, six of every group's eight lanes
// repeating the pair's work), so each lane's dependent chain runs with its SIMD to itself.
constexpr int G1J_WORDS = 3 * NL + 1;
__global__ __launch_bounds__(BLS_LANES) void k_bls_h2c_2(uint32_t n, const uint8_t* msg, const uint64_t* off,
                                                         const uint32_t* len, const uint8_t* dst, uint32_t dl,
                                                         uint32_t* rec, const uint32_t* kmode) {
    __shared__ uint32_t xa[(BLS_LANES / 2) * G1J_WORDS];
    const int pr = (int)threadIdx.x >> 1, u = (int)threadIdx.x & 1;
    const uint32_t i = blockIdx.x * (BLS_LANES / 2) + (uint32_t)pr;
    jac<fp> q;
    if (i < n) {
        q = h2c_map(msg + off[i], len[i], dst, dl, u);
        if (u) st_g1j(xa + G1J_WORDS * pr, q);
    }
    __syncthreads();
    if (i >= n || u) return;
    const jac<fp> q1 = ld_g1j(xa + G1J_WORDS * pr);
    const jac<fp> h0 = jac_add(q, q1);
    const jac<fp> h = kmode && kmode[i] ? h0 : jac_mul64(h0, BLS_H_EFF);
    fp x = fp_zero(), y = fp_zero();
    if (!h.inf) g1_to_affine_vt(x, y, h);
    st_g1(rec + (size_t)G1_REC_WORDS * i, x, y, h.inf);
}
// the item's status in the oracle's order: the signature's, then the keys'
__global__ __launch_bounds__(BLS_LANES) void k_bls_status(uint32_t n, const int32_t* st_sig, const int32_t* st_apk,
                                                          int32_t* st) {
    BLS_IDX();
    st[i] = st_sig[i] != ST_OK ? st_sig[i] : st_apk[i];
}
__global__ __launch_bounds__(BLS_LANES) void k_bls_pair(uint32_t n, const uint32_t* sig_rec, const uint32_t* h_rec,
                                                        const uint32_t* apk_rec, int32_t* st) {
    BLS_GIDX();
    if (st[i] != ST_OK) return;  // uniform over the group
    const bool ok = g_pairing_check(g, sig_rec + (size_t)G1_REC_WORDS * i, h_rec + (size_t)G1_REC_WORDS * i,
                                    apk_rec + (size_t)G2_REC_WORDS * i);
    g_sync();
    if (g.slot == 0) st[i] = ok ? ST_OK : ST_VERIFY_FAIL;
}
// the batch check (bls_verify.h), in stages:
//   k_bls_rlc_pts   one group per item: P_i = [r_i] H_i, s_i = [r_i] sig_i (Jacobian)
//   k_bls_sfold     ceil(log2 n) levels of G1 sums: S = sum s_i
//   k_bls_sig_item  one lane: (-S, g2) as item n
//   k_bls_rlc_ml    one group per item and one more: the Miller loops of (P_i, apk_i) and (-S, g2)
//   k_bls_ffold     ceil(log2 (n + 1)) levels of group Fp12 products
//   k_bls_final     one group: the final exponentiation, == 1
__global__ __launch_bounds__(BLS_LANES) void k_bls_rlc_pts(uint32_t n, const uint32_t* sig_rec, const uint32_t* h_rec,
                                                           const int32_t* st, const uint8_t* seed, uint32_t* prec,
                                                           uint32_t* srec) {
    BLS_GIDX();
    uint32_t* p = prec + (size_t)G1J_REC_WORDS * i;
    uint32_t* s = srec + (size_t)G1J_REC_WORDS * i;
    if (st[i] != ST_OK) {
        g_rlc_neutral(g, p, s);
        return;
    }
    g_rlc_points(g, sig_rec + (size_t)G1_REC_WORDS * i, h_rec + (size_t)G1_REC_WORDS * i, rlc_scalar(seed, i), p, s);
}
// one level of a tree over m entries: entry j <- entry j (+) entry j + h, h = ceil(m / 2), j < m - h
__global__ __launch_bounds__(BLS_LANES) void k_bls_sfold(uint32_t m, uint32_t* srec) {
    const uint32_t h = (m + 1) / 2;
    const uint32_t n = m - h;
    BLS_IDX();
    rlc_sfold(srec + (size_t)G1J_REC_WORDS * i, srec + (size_t)G1J_REC_WORDS * (i + h));
}
// -S (affine) and g2 as item n of the Miller-loop grid (srec[0] = S after the G1 tree)
__global__ void k_bls_sig_item(uint32_t n, const uint32_t* srec, uint32_t* prec, uint32_t* apk_rec) {
    if (blockIdx.x || threadIdx.x) return;
    rlc_sig_item(srec, prec + (size_t)G1J_REC_WORDS * n, apk_rec + (size_t)G2_REC_WORDS * n);
}
__global__ __launch_bounds__(BLS_LANES) void k_bls_rlc_ml(uint32_t n, const uint32_t* prec, const uint32_t* apk_rec,
                                                          uint32_t* frec) {
    BLS_GIDX();
    g_rlc_ml(g, prec + (size_t)G1J_REC_WORDS * i, apk_rec + (size_t)G2_REC_WORDS * i, frec + (size_t)F12_REC_WORDS * i);
}
__global__ __launch_bounds__(BLS_LANES) void k_bls_ffold(uint32_t m, uint32_t* frec) {
    const uint32_t h = (m + 1) / 2;
    const uint32_t n = m - h;
    BLS_GIDX();
    g_rlc_ffold(g, frec + (size_t)F12_REC_WORDS * i, frec + (size_t)F12_REC_WORDS * (i + h));
}
__global__ __launch_bounds__(BLS_LANES) void k_bls_final(const uint32_t* frec, int32_t* ok) {
    const uint32_t n = 1;
    BLS_GIDX();
    const bool r = g_rlc_final(g, frec);
    g_sync();
    if (g.slot == 0) *ok = r ? 1 : 0;
}
// st[i] <- the decode status when it is a failure, else the G1 check's
__global__ __launch_bounds__(BLS_LANES) void k_bls_st_join(uint32_t n, const int32_t* dec, int32_t* st) {
    BLS_IDX();
    if (dec[i] != ST_OK) st[i] = dec[i];
}
__global__ __launch_bounds__(BLS_LANES) void k_bls_keygen(uint32_t n, const uint8_t* sk, uint8_t* pk) {
    BLS_IDX();
    const jac<fp2> q = jac_mul_be(jac_from_affine(k_g2x(), k_g2y()), sk + 32 * (size_t)i, 32);
    fp2 x = f2_zero(), y = f2_zero();
    if (!q.inf) g2_to_affine(x, y, q);
    g2_compress(pk + 96 * (size_t)i, x, y, q.inf);
}
__global__ __launch_bounds__(BLS_LANES) void k_bls_sign(uint32_t n, const uint8_t* sk, const uint8_t* msg,
                                                        const uint64_t* off, const uint32_t* len, const uint8_t* dst,
                                                        uint32_t dl, uint8_t* sig) {
    BLS_IDX();
    const jac<fp> s = jac_mul_be(hash_to_g1(msg + off[i], len[i], dst, dl), sk + 32 * (size_t)i, 32);
    fp x = fp_zero(), y = fp_zero();
    if (!s.inf) g1_to_affine(x, y, s);
    g1_compress(sig + 48 * (size_t)i, x, y, s.inf);
}
__device__ void be_to_mont(fp& r, const uint8_t* b) {
    fp t;
    plain_from_be(t, b);
    r = fp_to_mont(t);
}
__global__ __launch_bounds__(BLS_LANES) void k_bls_h2c_out(uint32_t n, const uint8_t* msg, const uint64_t* off,
                                                           const uint32_t* len, const uint8_t* dst, uint32_t dl,
                                                           uint8_t* out) {
    BLS_IDX();
    uint32_t rec[G1_REC_WORDS];
    h2c_record(msg + off[i], len[i], dst, dl, rec);
    uint8_t* o = out + 96 * (size_t)i;
    if (rec[2 * NL]) {
        for (int k = 0; k < 96; k++) o[k] = 0;
        return;
    }
    plain_to_be(o, fp_from_mont(ld_fp(rec)));
    plain_to_be(o + 48, fp_from_mont(ld_fp(rec + NL)));
}
__global__ __launch_bounds__(BLS_LANES) void k_bls_pairing_raw(uint32_t n, const uint8_t* P, const uint8_t* Q,
                                                               uint8_t* out) {
    BLS_IDX();
    const uint8_t* p = P + 96 * (size_t)i;
    const uint8_t* q = Q + 192 * (size_t)i;
    uint32_t zp = 0, zq = 0;
    for (int k = 0; k < 96; k++) zp |= p[k];
    for (int k = 0; k < 192; k++) zq |= q[k];
    fp12 e = f12_one();
    if (zp && zq) {
        fp px, py;
        fp2 qx, qy;
        be_to_mont(px, p);
        be_to_mont(py, p + 48);
        be_to_mont(qx.c1, q);
        be_to_mont(qx.c0, q + 48);
        be_to_mont(qy.c1, q + 96);
        be_to_mont(qy.c0, q + 144);
        e = final_exp(miller_loop2(1, &px, &py, &qx, &qy));
    }
    const fp* c[12] = {&e.c0.c0.c0, &e.c0.c0.c1, &e.c0.c1.c0, &e.c0.c1.c1, &e.c0.c2.c0, &e.c0.c2.c1,
                       &e.c1.c0.c0, &e.c1.c0.c1, &e.c1.c1.c0, &e.c1.c1.c1, &e.c1.c2.c0, &e.c1.c2.c1};
    uint8_t* o = out + 576 * (size_t)i;
    for (int k = 0; k < 12; k++) plain_to_be(o + 48 * k, fp_from_mont(*c[k]));
}

// ---- the wave engine (bls_wave.h): one 64-lane wave per item ------------------------------------
// a wave's LDS for programs of up to NS slots: wm points at slot 0 (P << k sits below it)
#define BLSW_LDS(NS)                                            \
    __shared__ uint32_t wm_lds[wave::KP_WORDS + wave::SW * (NS)]; \
    uint32_t* const wm = wm_lds + wave::KP_WORDS
#define BLSW_IDX()                    \
    BLSW_LDS(wave::NSLOTS_PAIR);      \
    const uint32_t i = blockIdx.x;    \
    if (i >= n) return
// H(msg_i), homogeneous
__device__ __forceinline__ void blsw_h2c_item(uint32_t* wm, uint32_t i, const uint8_t* msg, const uint64_t* off,
                                              const uint32_t* len, const uint8_t* dst, uint32_t dl, uint32_t* hrec,
                                              const uint32_t* kmode) {
    const wave::Wave w{wm, (int)threadIdx.x};
    w_hash_to_g1(w, msg + off[i], len[i], dst, dl, hrec + (size_t)G1H_REC_WORDS * i, !(kmode && kmode[i]));
}
// signature decode only (one lane per item); the G1 check runs beside the pairing (k_blsw_pair_sub)
__global__ __launch_bounds__(BLS_LANES) void k_blsw_sigdec(uint32_t n, const uint8_t* sig, uint32_t* rec, int32_t* st) {
    BLS_IDX();
    fp x, y;
    bool inf;
    const int32_t s = g1_decompress(x, y, inf, sig + 48 * (size_t)i);
    if (s != ST_OK || inf) x = y = fp_zero();
    st_g1(rec + (size_t)G1_REC_WORDS * i, x, y, s == ST_OK && inf);
    st[i] = s;
}
__device__ __forceinline__ void blsw_sub_item(uint32_t* wm, uint32_t i, const uint32_t* rec, const int32_t* st_dec,
                                              int32_t* st_sub) {
    const wave::Wave w{wm, (int)threadIdx.x};
    const uint32_t* r = rec + (size_t)G1_REC_WORDS * i;
    int32_t s = ST_OK;
    if (st_dec[i] == ST_OK && !r[2 * NL]) s = w_g1_in_group(w, r) ? ST_OK : ST_NOT_IN_GROUP;
    if (threadIdx.x == 0) st_sub[i] = s;
}
__global__ __launch_bounds__(64) void k_blsw_sub(uint32_t n, const uint32_t* rec, const int32_t* st_dec, int32_t* st_sub) {
    BLSW_IDX();
    blsw_sub_item(wm, i, rec, st_dec, st_sub);
}
// e(-sig, g2) e(H, apk) == 1 for every item whose signature decoded and whose keys are valid
// (run beside the signature's G1 check: the status join puts that check first)
// H: homogeneous records (k_blsw_pre) or affine ones (k_bls_h2c_g, h_hom = 0); apk: Jacobian
// records (k_blsw_apk)
// (a one-key item whose key is in the cache takes the key's precomputed line table: the Miller
// loop then only evaluates lines, no G2 arithmetic)
__device__ __forceinline__ void blsw_pair_item(uint32_t* wm, uint32_t i, const uint32_t* srec, const int32_t* st_dec,
                                               const uint32_t* hrec, int h_hom, const uint32_t* arec,
                                               const int32_t* st_apk, const KeyTab& kt, const uint32_t* pk_off,
                                               const uint32_t* pk_cnt, const uint32_t* pk_idx, const uint32_t* kmode,
                                               int32_t* st_pair) {
    const wave::Wave w{wm, (int)threadIdx.x};
    int32_t s = ST_VERIFY_FAIL;
    if (st_dec[i] == ST_OK && st_apk[i] == ST_OK) {
        const uint32_t* ql = nullptr;
        if (kt.lines && kmode && kmode[i] && pk_cnt[i] == 1) ql = key_lines(kt, pk_idx[pk_off[i]]);
        s = w_pairing_check_g(w, srec + (size_t)G1_REC_WORDS * i,
                              hrec + (size_t)(h_hom ? G1H_REC_WORDS : G1_REC_WORDS) * i, h_hom != 0,
                              arec + (size_t)G2J_WORDS * i, true, ql)
                ? ST_OK
                : ST_VERIFY_FAIL;
    }
    if (threadIdx.x == 0) st_pair[i] = s;
}
// The throughput form: up to BLS_PACK_MAX items per wave (wave::WaveK: each item's slots in its
// own LDS bank, the narrow stages of every item in one pass).  e(-sig, g2) e(H, apk) == 1 for each
// item as blsw_pair_item; an item whose signature or keys failed gets VERIFY_FAIL whatever its bank
// computed.  Precomputed key lines are used only when every item of the wave has them (the Miller
// loop's program is one for the wave).
//
// The whole check is one loop over the flat script of wave::pairing_script (g_pair_script, one per
// line mode): the stage loop below is the kernel's only copy of the interpreter and the loop makes
// no calls, so no callee-saved registers go through scratch (round 5's out-of-line interpreter
// call wrote ~616 KB of scratch per item).  The banks share one P << k table at the front of the LDS
// (9.6 KB a bank instead of 10.5 KB).
constexpr int BLS_PACK_MAX = 4;
// items per group of the wave batch check (env NWV_BLS_BATCH_GROUP overrides)
#ifndef NWV_BLS_BATCH_GROUP_DEFAULT
#define NWV_BLS_BATCH_GROUP_DEFAULT 16
#endif
// eligible items per group of the key-transposed batch check (env NWV_BLS_KEY_GROUP overrides)
#ifndef NWV_BLS_KEY_GROUP_DEFAULT
#define NWV_BLS_KEY_GROUP_DEFAULT 2048
#endif
__device__ wave::SOp g_pair_script[2][wave::SCRIPT_MAX];  // [fixed key lines]
__device__ int g_pair_script_n[2];
// the Miller loop alone (wave::miller_script): the wave batch check's per-item pass
__device__ wave::SOp g_mill_script[2][wave::SCRIPT_MAX];
__device__ int g_mill_script_n[2];
// two waves per SIMD (<= 256 registers: at most 4 terms' LDS reads in flight, NWV_BLS_PAIR_TERMS
// of bls_wave.h)
// with three items a wave (NWV_BLS_PACK: 3 x 6.5 KB banks -- registers never live together share
// slots, tools/gen_bls_wave.py PC_ALIAS -- + the shared 0.9 KB table = 8 waves per CU): 16,384
// checks 23.5 -> 16.0 ms against one wave per SIMD with three 10.5 KB banks
// (profiles/round6_bls_pair_sweep.txt)
#ifndef NWV_BLS_PAIR_WAVES
#define NWV_BLS_PAIR_WAVES 2
#endif
// x / d and x % d for 0 <= x <= 64 and a wave-uniform 1 <= d <= 64 without a division sequence:
// x ceil(2^16 / d) >> 16 is exact there (the error x (ceil(2^16/d) - 2^16/d) / 2^16 < 1/1024 < 1/d)
__constant__ const uint32_t k_div_magic[65] = {0, 65536, 32768, 21846, 16384, 13108, 10923, 9363, 8192, 7282, 6554, 5958, 5462, 5042, 4682, 4370, 4096, 3856, 3641, 3450, 3277, 3121, 2979, 2850, 2731, 2622, 2521, 2428, 2341, 2260, 2185, 2115, 2048, 1986, 1928, 1873, 1821, 1772, 1725, 1681, 1639, 1599, 1561, 1525, 1490, 1457, 1425, 1395, 1366, 1338, 1311, 1286, 1261, 1237, 1214, 1192, 1171, 1150, 1130, 1111, 1093, 1075, 1058, 1041, 1024};  // ceil(2^16 / d)
__device__ __forceinline__ int lane_div(int x, int d) {
    const uint32_t m = k_div_magic[__builtin_amdgcn_readfirstlane(d)];
    return (int)(((uint32_t)x * m) >> 16);
}
__device__ __forceinline__ int lane_mod(int x, int d) { return x - lane_div(x, d) * d; }
// the Miller-only form's extra arguments (MILLER): entries [0, n_items) of the grid are the call's
// items, each with the identity on its signature side (srec, st_dec, st_apk and st_pair are not
// read); entry n_items + g is group g's signature item: sgrec's record g against g2's own line
// table, the identity on its hash side.  Every entry's F goes to frec (FB_REC_WORDS each) in
// place of a verdict; an item with inb = 0 (outside the batch) writes 1.
struct MillArgs {
    uint32_t n_items;
    const uint32_t* sgrec;
    const uint32_t* inb;
    uint32_t* frec;
};
// items [i0, i0 + k) on this wave: lds_k = the P << k table, then k banks; G: term reads in flight
template <int G, bool MILLER = false>
__device__ __forceinline__ void pair_flat(uint32_t* lds_k, uint32_t i0, int k, const uint32_t* srec,
                                          const int32_t* st_dec, const uint32_t* hrec, int h_hom,
                                          const uint32_t* arec, const int32_t* st_apk, const KeyTab& kt,
                                          const uint32_t* pk_off, const uint32_t* pk_cnt, const uint32_t* pk_idx,
                                          const uint32_t* kmode, int32_t* st_pair, const MillArgs* ma = nullptr) {
    using namespace wave;
    const int lane = (int)threadIdx.x;
    constexpr uint32_t bankw = (uint32_t)(SW * NSLOTS_PC);
    const WaveK w{lds_k + KP_WORDS, bankw, k, lane};
    const wword* kpt = (const wword*)lds_k;  // the shared P << k table
    const uint32_t* sig[BLS_PACK_MAX];
    const uint32_t* hr[BLS_PACK_MAX];
    const uint32_t* ql[BLS_PACK_MAX];
    bool fixed = true;
    for (int j = 0; j < k; j++) {
        const uint32_t i = i0 + j;
        if (MILLER && i >= ma->n_items) {  // a group's signature item
            sig[j] = ma->sgrec + (size_t)G1_REC_WORDS * (i - ma->n_items);
            hr[j] = hrec + (size_t)G1H_REC_WORDS * i;
            ql[j] = &T_G2_LINES[0][0][0];
            continue;
        }
        sig[j] = MILLER ? nullptr : srec + (size_t)G1_REC_WORDS * i;
        hr[j] = hrec + (size_t)(h_hom ? G1H_REC_WORDS : G1_REC_WORDS) * i;
        ql[j] = (kt.lines && kmode && kmode[i] && pk_cnt[i] == 1) ? key_lines(kt, pk_idx[pk_off[i]]) : nullptr;
        fixed = fixed && ql[j] != nullptr;
    }
    // P << k once, then every bank: slot 0 = 0, the pairing check's constants at slots 1..
    for (int t = lane; t < KP_WORDS; t += 64) lds_k[t] = (&T_KP[0][0])[t];
    for (int j = 0; j < k; j++) {
        if (lane < SW) w.bk(j)[lane] = 0u;
        for (int t = lane; t < SW * NCONSTS_PC; t += 64) w.bk(j)[SW + t] = (&T_CONSTS[0][0])[t];
    }
    w.zero(REG_PA, 2);
    w.zero(REG_PB, 3);
    w.zero(REG_QB, 6);
    w.sync();
    for (int j = 0; j < k; j++) {
        const uint32_t i = i0 + j;
        if ((!MILLER || sig[j]) && !sig[j][2 * NL]) {
            w.put_words(j, REG_PA, sig[j], 1);
            w.put_fp(j, REG_PA + 1, fp_neg(ld_fp(sig[j] + NL)));
        }
        const bool h_inf = hr[j][(h_hom ? 3 : 2) * NL] != 0;
        if (!h_inf) w.put_words(j, REG_PB, hr[j], h_hom ? 3 : 2);
        if (h_inf || !h_hom) w.put_fp(j, REG_PB + 2, k_one());
        w.put_words(j, REG_QB, arec + (size_t)G2J_WORDS * i, 6);
    }
    w.sync();
    // wave::pairing_check's set-up over the k banks
    w.zero(REG_F, 12);
    w.sync();
    w.put_fp(-1, REG_F, k_one());
    w.copy_slots(REG_TB, REG_QB, 6);
    w.sync();
    constexpr int LW = 6 * SW;  // words of a step's line
    // the next step's lines load while this step runs: g2's (every bank) and each item's key lines
    uint32_t la0 = 0, la1 = 0, lb0[BLS_PACK_MAX], lb1[BLS_PACK_MAX];
    auto fetch = [&](int st) {
        const uint32_t* g = &T_G2_LINES[st][0][0];
        la0 = lane < LW ? g[lane] : 0u;
        la1 = lane + 64 < LW ? g[lane + 64] : 0u;
        for (int j = 0; j < BLS_PACK_MAX; j++) {
            lb0[j] = 0u;
            lb1[j] = 0u;
            if (j < k && fixed) {
                const uint32_t* q = ql[j] + (size_t)st * LW;
                lb0[j] = lane < LW ? q[lane] : 0u;
                lb1[j] = lane + 64 < LW ? q[lane + 64] : 0u;
            }
        }
    };
    fetch(0);
    const SOp* script = MILLER ? g_mill_script[fixed ? 1 : 0] : g_pair_script[fixed ? 1 : 0];
    const int nops = MILLER ? g_mill_script_n[fixed ? 1 : 0] : g_pair_script_n[fixed ? 1 : 0];
    auto first_rec = [&](const SOp& o) { return load_rec(T_DATA + o.a + (uint32_t)lane_mod(lane, (int)(o.b >> 16)) * REC); };
    Rec cur = first_rec(script[0].c >> 16 == SOP_RUN ? script[0] : script[script[0].next_run]);
    int step = 0;
#pragma unroll 1
    for (int oi = 0; oi < nops; oi++) {
        const SOp op = script[oi];
        const uint32_t kind = op.c >> 16;
        if (kind == SOP_LINES) {
            for (int j = 0; j < k; j++) {
                uint32_t* b = w.bk(j);
                if (lane < LW) b[SW * REG_LA + lane] = la0;
                if (lane + 64 < LW) b[SW * REG_LA + lane + 64] = la1;
                if (fixed) {
                    if (lane < LW) b[SW * REG_LB + lane] = lb0[j];
                    if (lane + 64 < LW) b[SW * REG_LB + lane + 64] = lb1[j];
                }
            }
            w.sync();
            if (step + 1 < NSTEPS) fetch(step + 1);
            step++;
            continue;
        }
        if (kind == SOP_INV) {
            w.invert_slot((int)op.a, (int)op.b);
            w.sync();
            continue;
        }
        // RUN: the program's stages, `reps` times over (wave_run's loop over the banks: the one copy)
        const uint16_t* base0 = T_DATA + op.a;
        const uint16_t* base = base0;
        const int np = (int)(op.b & 0xffffu), nl0 = (int)(op.b >> 16), total = np * (int)(op.c & 0xffffu);
        int nl = nl0;
#pragma unroll 1
        for (int t = 0, s = 0; t < total; t++) {
            Hdr h = rec_hdr(cur);
            h.nap = __builtin_amdgcn_readfirstlane(h.nap);
            h.nan = __builtin_amdgcn_readfirstlane(h.nan);
            h.nbp = __builtin_amdgcn_readfirstlane(h.nbp);
            h.nbn = __builtin_amdgcn_readfirstlane(h.nbn);
            const bool wrap = s + 1 == np;
            const int nl_next = wrap ? nl0 : __builtin_amdgcn_readfirstlane(h.nl_next);
            const uint16_t* nbase = wrap ? base0 : base + (uint32_t)nl * REC;
            // the next stage's record, or the next RUN op's first one (records are static data)
            Rec nxt = cur;
            if (t + 1 < total) nxt = load_rec(nbase + (uint32_t)lane_mod(lane, nl_next) * REC);
            else if (op.next_run >= 0) nxt = first_rec(script[op.next_run]);
            const int ipp = lane_div(64, nl), first = lane_div(lane, nl);
            if (first < ipp) {
                const uint32_t dst = rec_u16(cur, 0);
#pragma unroll 1
                for (int item = first; item < k; item += ipp) {
                    wword* wm = (wword*)w.bk(item);
                    const fp v = lane_value<G>(wm, kpt, h, cur);
#pragma unroll
                    for (int j = 0; j < NL; j++) wm[SW * dst + j] = v.l[j];
                }
            }
            wsync();
            base = nbase;
            nl = nl_next;
            cur = nxt;
            s = wrap ? 0 : s + 1;
        }
    }
    if (MILLER) {
        // fail closed: a pass that found no script (or not all of its steps) writes F = 0 and
        // counts no Miller output, so its group's last wave rejects
        const bool ran = nops > 0 && step == NSTEPS;
        const fp one = k_one();
        for (int j = 0; j < k; j++) {
            const uint32_t i = i0 + j;
            const bool live = i >= ma->n_items || ma->inb[i] != 0;
            uint32_t* o = ma->frec + (size_t)FB_REC_WORDS * i;
            for (int t = lane; t < 12 * SW; t += 64)
                o[t] = !ran ? 0u : live ? w.bk(j)[SW * REG_F + t] : t < NL ? one.l[t] : 0u;
            if (lane == 0) {
                o[12 * SW] = ran ? 1u : 0u;
                o[12 * SW + 1] = 0u;
            }
        }
        return;
    }
    const uint32_t ok = w.f_is_one_mask();
    if (lane == 0)
        for (int j = 0; j < k; j++) {
            const uint32_t i = i0 + j;
            st_pair[i] = (st_dec[i] == ST_OK && st_apk[i] == ST_OK && ((ok >> j) & 1u)) ? ST_OK : ST_VERIFY_FAIL;
        }
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NWV_BLS_PAIR_WAVES))) void k_blsw_pair_k(
    uint32_t n, uint32_t kper, const uint32_t* srec, const int32_t* st_dec, const uint32_t* hrec, int h_hom,
    const uint32_t* arec, const int32_t* st_apk, KeyTab kt, const uint32_t* pk_off, const uint32_t* pk_cnt,
    const uint32_t* pk_idx, const uint32_t* kmode, int32_t* st_pair) {
    extern __shared__ uint32_t lds_k[];
    const uint32_t i0 = blockIdx.x * kper;
    if (i0 >= n) return;
    pair_flat<NWV_BLS_PAIR_TERMS>(lds_k, i0, (int)(n - i0 < kper ? n - i0 : kper), srec, st_dec, hrec, h_hom, arec,
                                  st_apk, kt, pk_off, pk_cnt, pk_idx, kmode, st_pair);
}
// The wave batch check (bls_verify.h): one final exponentiation per group of `grp` consecutive
// items instead of one per item.
//   k_blsw_rlc_pts   two lanes per item: [r_i] H_i (homogeneous) and [r_i] sig_i (Jacobian); an item
//                    outside the batch (a failed status, an identity signature) writes neutral
//                    records, inb = 0 and its own pairing verdict
//   k_blsw_sfold     the levels of every group's G1 tree: S_g = sum [r_i] sig_i
//   k_blsw_sig_items one lane per group: S_g affine, entry n + g of the Miller grid
//   k_blsw_mill_k    the Miller loops of the n items and the groups' signature items, packed as
//                    k_blsw_pair_k packs (pair_flat over wave::miller_script), F records out
//   k_blsw_ffold     the levels of every group's product tree, WB_FAN records a wave; the last
//                    level's wave (one per group) runs the final exponentiation, verdict word out
//   k_blsw_mark      st_pair of the items inside the batch from their group's verdict
__global__ __launch_bounds__(BLS_LANES) void k_blsw_rlc_pts(uint32_t n, const uint32_t* srec, const uint32_t* hrec,
                                                            const int32_t* st_dec, const int32_t* st_apk,
                                                            const uint32_t* kmode, const uint8_t* seed, uint32_t* prec,
                                                            uint32_t* jrec, uint32_t* inb, int32_t* st_pair) {
    // two lanes an item: the even one takes [r] H (and the item's flags), the odd one [r] sig; both
    // walk the same scalar, so a pair never diverges
    const uint32_t t = blockIdx.x * BLS_LANES + threadIdx.x, i = t >> 1;
    if (i >= n) return;
    const bool sig_side = (t & 1u) != 0;
    uint32_t* p = prec + (size_t)G1H_REC_WORDS * i;
    uint32_t* s = jrec + (size_t)G1J_REC_WORDS * i;
    const uint32_t* sr = srec + (size_t)G1_REC_WORDS * i;
    const uint32_t* hr = hrec + (size_t)G1_REC_WORDS * i;
    const bool ok = st_dec[i] == ST_OK && st_apk[i] == ST_OK;
    if (!ok || sr[2 * NL]) {
        wb_neutral_rec(sig_side ? s : p);
        if (sig_side) return;
        inb[i] = 0u;
        st_pair[i] = ok && wb_identity_sig_holds(hr, kmode && kmode[i]) ? ST_OK : ST_VERIFY_FAIL;
        return;
    }
    const uint64_t r = rlc_scalar(seed, i);
    if (sig_side) {
        wb_point_s(sr, r, s);
    } else {
        wb_point_h(hr, r, p);
        inb[i] = 1u;
    }
}
// level m of the groups' G1 trees: lane (g, j), j < ceil(m / 2)
__global__ __launch_bounds__(BLS_LANES) void k_blsw_sfold(uint32_t n_items, uint32_t grp, uint32_t ng, uint32_t m,
                                                          uint32_t* jrec) {
    const uint32_t h = (m + 1) / 2, n = ng * h;
    BLS_IDX();
    const uint32_t g = i / h, j = i % h, lo = g * grp;
    wb_sfold(jrec + (size_t)G1J_REC_WORDS * lo, j, m, min(grp, n_items - lo));
}
__global__ __launch_bounds__(BLS_LANES) void k_blsw_sig_items(uint32_t n_items, uint32_t grp, uint32_t n,
                                                              const uint32_t* jrec, uint32_t* sgrec, uint32_t* prec,
                                                              uint32_t* arec) {
    BLS_IDX();
    wb_sig_item(jrec + (size_t)G1J_REC_WORDS * i * grp, sgrec + (size_t)G1_REC_WORDS * i,
                prec + (size_t)G1H_REC_WORDS * (n_items + i), arec + (size_t)G2J_WORDS * (n_items + i));
}
static_assert(G2J_WORDS == G2J_REC_WORDS, "wb_sig_item writes the key sums' record form");
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NWV_BLS_PAIR_WAVES))) void k_blsw_mill_k(
    uint32_t n, uint32_t kper, MillArgs ma, const uint32_t* prec, const uint32_t* arec, KeyTab kt,
    const uint32_t* pk_off, const uint32_t* pk_cnt, const uint32_t* pk_idx, const uint32_t* kmode) {
    extern __shared__ uint32_t lds_k[];
    const uint32_t i0 = blockIdx.x * kper;
    if (i0 >= n) return;
    pair_flat<NWV_BLS_PAIR_TERMS, true>(lds_k, i0, (int)(n - i0 < kper ? n - i0 : kper), nullptr, nullptr, prec, 1, arec,
                                        nullptr, kt, pk_off, pk_cnt, pk_idx, kmode, nullptr, &ma);
}
// stride s of the groups' product trees: wave wv of group g multiplies the group's records at
// positions (wv WB_FAN + q) s, q < WB_FAN, below the group's items + 1 (position p < items: item
// g grp + p; position items: the group's signature item n_items + g) into the first of them.  With
// one wave a group (last) the product is the group's whole: that wave accepts when it holds every
// Miller output of the group and its final exponentiation is 1.  gok[g] was zeroed before the tree.
__global__ __launch_bounds__(64) void k_blsw_ffold(uint32_t n_items, uint32_t grp, uint32_t wpg, uint32_t s, int last,
                                                   uint32_t* frec, int32_t* gok) {
    BLSW_LDS(wave::NSLOTS_PC);
    const uint32_t g = blockIdx.x / wpg, wv = blockIdx.x % wpg, lo = g * grp;
    if (lo >= n_items) return;
    const uint32_t gsize = min(grp, n_items - lo), m = gsize + 1, p0 = wv * WB_FAN * s;
    if (p0 >= m) return;
    const wave::Wave w{wm, (int)threadIdx.x};
    auto at = [&](uint32_t p) { return frec + (size_t)FB_REC_WORDS * (p < gsize ? lo + p : n_items + g); };
    const uint32_t cnt = w_ffold_step(w, at, p0, s, m, WB_FAN);
    if (last) {
        const bool ok = w_group_final(w);
        if (threadIdx.x == 0) gok[g] = (ok && cnt == m) ? 1 : 0;
        return;
    }
    uint32_t* o = at(p0);
    w.get_words(wave::REG_F, o, 12);
    if (threadIdx.x == 0) o[12 * NL] = cnt;
}
__global__ __launch_bounds__(BLS_LANES) void k_blsw_mark(uint32_t n, uint32_t grp, const int32_t* gok,
                                                         const uint32_t* inb, int32_t* st_pair) {
    BLS_IDX();
    if (inb[i]) st_pair[i] = gok[i / grp] == 1 ? ST_OK : ST_VERIFY_FAIL;
}
// The key-transposed batch check (bls_key_batch.h, bls_verify.h): the wave batch check's product
// regrouped by registered key, K + 1 Miller loops a group of K distinct keys whatever its items.
// The host's plan names the groups' items (`items`, group g at positions [g grp, (g + 1) grp)) and
// every (group, key) entry's occurrences (coff / cidx, positions in `items`).
//   k_blsk_rlc_pts   two lanes per position: [r_i] H_i and [r_i] sig_i, both Jacobian, r_i by the
//                    caller's item index
//   k_blsw_sfold     (the wave batch check's) S_g over the positions' [r_i] sig_i
//   k_blsk_key_sums  one wave per key entry: T_k, the entry's hash side; the key's record as its Q
//   k_blsk_sig_items one lane per group: S_g's entry behind the key entries
//   k_blsw_mill_k    (the wave batch check's) every entry a one-key key-side item on its key's
//                    registered line table
//   k_blsk_ffold     k_blsw_ffold's tree over groups of unequal entry counts
//   k_blsk_mark      st_pair of the groups' items from their group's verdict
// Fail closed beyond the F records' counts: an item the plan names whose statuses the device does
// not find OK (or whose signature is the identity), or an entry whose key's status is not OK,
// poisons its group, and a poisoned group's last wave rejects.
__global__ __launch_bounds__(BLS_LANES) void k_blsk_rlc_pts(uint32_t n, uint32_t grp, const uint32_t* items,
                                                            const uint32_t* srec, const uint32_t* hrec,
                                                            const int32_t* st_dec, const int32_t* st_apk,
                                                            const uint8_t* seed, uint32_t* hj, uint32_t* sj,
                                                            uint32_t* poison) {
    const uint32_t t = blockIdx.x * BLS_LANES + threadIdx.x, e = t >> 1;
    if (e >= n) return;
    const uint32_t i = items[e];
    const bool sig_side = (t & 1u) != 0;
    const uint32_t* sr = srec + (size_t)G1_REC_WORDS * i;
    uint32_t* out = (sig_side ? sj : hj) + (size_t)G1J_REC_WORDS * e;
    if (st_dec[i] != ST_OK || st_apk[i] != ST_OK || sr[2 * NL]) {
        wb_neutral_rec(out);
        if (!sig_side) poison[e / grp] = 1u;
        return;
    }
    wb_point_s(sig_side ? sr : hrec + (size_t)G1_REC_WORDS * i, rlc_scalar(seed, i), out);
}
__global__ __launch_bounds__(64) void k_blsk_key_sums(uint32_t n, const uint32_t* coff, const uint32_t* cidx,
                                                      const uint32_t* eslot, const uint32_t* egrp, const uint32_t* hj,
                                                      KeyTab kt, uint32_t* prec, uint32_t* arec, uint32_t* poison) {
    __shared__ uint32_t xa[32 * G1J_REC_WORDS];
    const uint32_t m = blockIdx.x;
    if (m >= n) return;
    const int lane = (int)threadIdx.x;
    const uint32_t c0 = coff[m], slot = eslot[m];
    jac<fp> acc = kb_lane_sum(hj, cidx + c0, coff[m + 1] - c0, (uint32_t)lane, 64u);
#pragma unroll 1
    for (int h = 32; h >= 1; h >>= 1) {
        __syncthreads();
        if (lane >= h && lane < 2 * h) st_g1j(xa + (lane - h) * G1J_REC_WORDS, acc);
        __syncthreads();
        if (lane < h) acc = jac_add(acc, ld_g1j(xa + lane * G1J_REC_WORDS));
    }
    const uint32_t* kr = kt.hrc + (size_t)G2_REC_WORDS * slot;
    uint32_t* q = arec + (size_t)G2J_WORDS * m;
    for (int wd = lane; wd < G2J_WORDS; wd += 64) q[wd] = kb_key_q_word(kr, wd);
    if (lane != 0) return;
    wb_store_hom(prec + (size_t)G1H_REC_WORDS * m, acc);
    if (kt.sc[slot] != ST_OK) poison[egrp[m]] = 1u;
}
__global__ __launch_bounds__(BLS_LANES) void k_blsk_sig_items(uint32_t n, uint32_t grp, uint32_t n_ent,
                                                              const uint32_t* sj, uint32_t* sgrec, uint32_t* prec,
                                                              uint32_t* arec) {
    BLS_IDX();
    wb_sig_item(sj + (size_t)G1J_REC_WORDS * i * grp, sgrec + (size_t)G1_REC_WORDS * i,
                prec + (size_t)G1H_REC_WORDS * (n_ent + i), arec + (size_t)G2J_WORDS * (n_ent + i));
}
// k_blsw_ffold with group g's records at positions p < keys: key entry goff[g] + p; p = keys: the
// group's signature entry n_ent + g
__global__ __launch_bounds__(64) void k_blsk_ffold(uint32_t ng, const uint32_t* goff, uint32_t n_ent, uint32_t wpg,
                                                   uint32_t s, int last, uint32_t* frec, const uint32_t* poison,
                                                   int32_t* gok) {
    BLSW_LDS(wave::NSLOTS_PC);
    const uint32_t g = blockIdx.x / wpg, wv = blockIdx.x % wpg;
    if (g >= ng) return;
    const uint32_t e0 = goff[g], keys = goff[g + 1] - e0, m = keys + 1, p0 = wv * WB_FAN * s;
    if (p0 >= m) return;
    const wave::Wave w{wm, (int)threadIdx.x};
    auto at = [&](uint32_t p) { return frec + (size_t)FB_REC_WORDS * (p < keys ? e0 + p : n_ent + g); };
    const uint32_t cnt = w_ffold_step(w, at, p0, s, m, WB_FAN);
    if (last) {
        const bool ok = w_group_final(w);
        if (threadIdx.x == 0) gok[g] = (ok && cnt == m && poison[g] == 0u) ? 1 : 0;
        return;
    }
    uint32_t* o = at(p0);
    w.get_words(wave::REG_F, o, 12);
    if (threadIdx.x == 0) o[12 * NL] = cnt;
}
__global__ __launch_bounds__(BLS_LANES) void k_blsk_mark(uint32_t n, uint32_t grp, const uint32_t* items,
                                                         const int32_t* gok, int32_t* st_pair) {
    BLS_IDX();
    st_pair[items[i]] = gok[i / grp] == 1 ? ST_OK : ST_VERIFY_FAIL;
}
// the flat scripts into g_pair_script on the calling thread's device, once per device
static int ensure_pair_script() {
    static std::mutex mu;
    static bool done[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
        return nwv_internal_set_err(NWV_ERR_HIP, "pair script: no device");
    std::lock_guard<std::mutex> g(mu);
    if (done[dev]) return NWV_OK;
    static wave::SOp ops[2][wave::SCRIPT_MAX];
    int cnt[2];
    for (int f = 0; f < 2; f++) cnt[f] = wave::pairing_script(f != 0, ops[f]);
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_pair_script), ops, sizeof(ops)) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(g_pair_script_n), cnt, sizeof(cnt)) != hipSuccess)
        return nwv_internal_set_err(NWV_ERR_HIP, "pair script copy");
    for (int f = 0; f < 2; f++) cnt[f] = wave::miller_script(f != 0, ops[f]);
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_mill_script), ops, sizeof(ops)) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(g_mill_script_n), cnt, sizeof(cnt)) != hipSuccess)
        return nwv_internal_set_err(NWV_ERR_HIP, "miller script copy");
    done[dev] = true;
    return NWV_OK;
}
__global__ __launch_bounds__(64) void k_blsw_pair(uint32_t n, const uint32_t* srec, const int32_t* st_dec,
                                                  const uint32_t* hrec, int h_hom, const uint32_t* arec,
                                                  const int32_t* st_apk, KeyTab kt, const uint32_t* pk_off,
                                                  const uint32_t* pk_cnt, const uint32_t* pk_idx, const uint32_t* kmode,
                                                  int32_t* st_pair) {
    BLSW_LDS(wave::NSLOTS_PAIR2);  // the two-step Miller-loop programs (a key's line table)
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    blsw_pair_item(wm, i, srec, st_dec, hrec, h_hom, arec, st_apk, kt, pk_off, pk_cnt, pk_idx, kmode, st_pair);
}
// the pairing checks (blocks [0, n)) and the signatures' G1 checks (blocks [n, 2n)) as one launch:
// independent waves, so the launch takes as long as the slower of the two per item
__global__ __launch_bounds__(64) void k_blsw_pair_sub(uint32_t n, const uint32_t* srec, const int32_t* st_dec,
                                                      const uint32_t* hrec, int h_hom, const uint32_t* arec,
                                                      const int32_t* st_apk, KeyTab kt, const uint32_t* pk_off,
                                                      const uint32_t* pk_cnt, const uint32_t* pk_idx,
                                                      const uint32_t* kmode, int32_t* st_pair, int32_t* st_sub) {
    BLSW_LDS(wave::NSLOTS_PAIR2);
    const uint32_t b = blockIdx.x;
    if (b < n)
        blsw_pair_item(wm, b, srec, st_dec, hrec, h_hom, arec, st_apk, kt, pk_off, pk_cnt, pk_idx, kmode, st_pair);
    else if (b < 2 * n)
        blsw_sub_item(wm, b - n, srec, st_dec, st_sub);
}
// the same with the pairing on the flat script (pair_flat, one item on the wave); NWV_BLS_SUB_FLAT=1
__global__ __launch_bounds__(64) void k_blsw_pair_sub_f(uint32_t n, const uint32_t* srec, const int32_t* st_dec,
                                                        const uint32_t* hrec, int h_hom, const uint32_t* arec,
                                                        const int32_t* st_apk, KeyTab kt, const uint32_t* pk_off,
                                                        const uint32_t* pk_cnt, const uint32_t* pk_idx,
                                                        const uint32_t* kmode, int32_t* st_pair, int32_t* st_sub) {
    BLSW_LDS(wave::NSLOTS_PAIR2);
    const uint32_t b = blockIdx.x;
    if (b < n)
        pair_flat<8>(wm_lds, b, 1, srec, st_dec, hrec, h_hom, arec, st_apk, kt, pk_off, pk_cnt, pk_idx, kmode, st_pair);
    else if (b < 2 * n)
        blsw_sub_item(wm, b - n, srec, st_dec, st_sub);
}
// [h_eff] pk of newly registered keys (lane per key, affine records): the hash's cofactor clearing
// moves onto the key side -- e(H0, [h_eff] pk) = e([h_eff] H0, pk) for H0 in E(Fp), as the
// reduced pairing sees only H0's G1 component (tests/test_bls_hostemu.py
// test_wave_cofactor_on_key_side) -- so a cached key's item skips the 64-bit G1 chain on H
__global__ __launch_bounds__(BLS_LANES) void k_bls_key_heff(uint32_t n, const uint32_t* slots, const uint32_t* rc,
                                                            uint32_t* hrc) {
    BLS_IDX();
    const uint32_t k = slots[i];
    fp2 x, y;
    ld_g2(rc + (size_t)G2_REC_WORDS * k, x, y);
    g2_to_affine_vt(x, y, jac_mul64(jac_from_affine(x, y), BLS_H_EFF));
    st_g2(hrc + (size_t)G2_REC_WORDS * k, x, y, false);
}
// the line tables of newly registered keys (of their [h_eff] pk): one wave per key (slots[i] = its
// cache slot)
__global__ __launch_bounds__(64) void k_blsw_key_lines(uint32_t n, const uint32_t* slots, const uint32_t* rc,
                                                       uint32_t* lines) {
    BLSW_IDX();
    const uint32_t k = slots[i];
    const wave::Wave w{wm, (int)threadIdx.x};
    w_key_lines(w, rc + (size_t)G2_REC_WORDS * k, lines + KL_WORDS * k);
}
// the fills of a call's aggregate-key ring slots (bls_apk_ring.h), one wave per set: item item[j]'s
// Jacobian key sum (k_blsw_pre's arec) made affine into record slot[j] of the ring, and that
// point's line table (w_apk_fill).  A sum whose status is not OK writes nothing (the host never
// publishes its slot).  The host keeps the slots away from every other call until this one has
// synchronised (busy flags).
__global__ __launch_bounds__(64) void k_blsw_apk_fill(uint32_t n, const uint32_t* item, const uint32_t* slot,
                                                      const uint32_t* arec, const int32_t* st_apk, uint32_t* ring_rec,
                                                      uint32_t* ring_lines) {
    BLSW_IDX();
    const wave::Wave w{wm, (int)threadIdx.x};
    const uint32_t it = item[i], k = slot[i];
    w_apk_fill(w, arec + (size_t)G2J_WORDS * it, st_apk[it], ring_rec + (size_t)G2_REC_WORDS * k,
               ring_lines + KL_WORDS * k);
}
// the key sum of item i on a wave: lane j adds the item's keys j, j + 64, ... (Jacobian, jac_add:
// exact in every case), then a six-level tree through LDS.  The status is that of the item's first
// bad key in list order (else AGGR_MISMATCH for an empty list, PK_INFINITY for an identity sum).
// The sum stays Jacobian (G2J_WORDS record: the Miller-loop programs take a Jacobian Q), so there
// is no inversion; a one-key item copies its validated record with Z = 1.
__device__ __forceinline__ void blsw_apk_item(uint32_t* xa, uint32_t i, const KeyTab& kt, const uint32_t* pk_off,
                                              const uint32_t* pk_cnt, const uint32_t* pk_idx, const uint32_t* kmode,
                                              uint32_t* rec, int32_t* st_apk) {
    const int lane = (int)threadIdx.x;
    const uint32_t cnt = pk_cnt[i];
    const uint32_t* idx = pk_idx + pk_off[i];
    uint32_t* out = rec + (size_t)G2J_WORDS * i;
    // key-side items (every key cached) sum the keys' [h_eff] pk records
    KeyTab kq = kt;
    if (kmode && kmode[i]) kq.rc = kt.hrc;
    if (cnt == 1) {
        const uint32_t k = idx[0];
        const int32_t ks = key_st(kq, k);
        const uint32_t* kr = key_rec(kq, k);
        const fp one = k_one();
        for (int wd = lane; wd < G2J_WORDS; wd += 64) {
            uint32_t v = 0;
            if (wd < 4 * NL) v = ks == ST_OK ? kr[wd] : 0u;
            else if (wd < 5 * NL) v = one.l[wd - 4 * NL];
            else if (wd == 6 * NL) v = ks == ST_OK ? 0u : 1u;
            out[wd] = v;
        }
        if (lane == 0) st_apk[i] = ks;
        return;
    }
    jac<fp2> acc;
    acc.inf = true;
    acc.x = acc.y = acc.z = f2_zero();
    uint32_t first_bad = 0xffffffffu;
    for (uint32_t j = (uint32_t)lane; j < cnt; j += 64) {
        const uint32_t k = idx[j];
        if (key_st(kq, k) != ST_OK) {
            first_bad = j;
            break;
        }
        fp2 x, y;
        ld_g2(key_rec(kq, k), x, y);
        acc = jac_add(acc, jac_from_affine(x, y));
    }
    for (int m = 32; m >= 1; m >>= 1) first_bad = min(first_bad, (uint32_t)__shfl_xor((int)first_bad, m));
#pragma unroll 1
    for (int h = 32; h >= 1; h >>= 1) {
        __syncthreads();
        if (lane >= h && lane < 2 * h) st_g2j(xa + (lane - h) * G2J_WORDS, acc);
        __syncthreads();
        if (lane < h) acc = jac_add(acc, ld_g2j(xa + lane * G2J_WORDS));
    }
    if (lane != 0) return;
    int32_t status = ST_OK;
    if (cnt == 0) status = ST_AGGR_MISMATCH;
    else if (first_bad != 0xffffffffu) status = key_st(kq, idx[first_bad]);
    else if (acc.inf) status = ST_PK_INFINITY;
    if (status != ST_OK) {
        acc.inf = true;
        acc.x = acc.y = acc.z = f2_zero();
    }
    st_g2j(out, acc);
    st_apk[i] = status;
}
__global__ __launch_bounds__(64) void k_blsw_apk(uint32_t n, KeyTab kt, const uint32_t* pk_off, const uint32_t* pk_cnt,
                                                 const uint32_t* pk_idx, const uint32_t* kmode, uint32_t* rec,
                                                 int32_t* st_apk) {
    __shared__ uint32_t xa[32 * G2J_WORDS];
    if (blockIdx.x >= n) return;
    blsw_apk_item(xa, blockIdx.x, kt, pk_off, pk_cnt, pk_idx, kmode, rec, st_apk);
}
// the same over an item list (the items the dense key-sum stage leaves to the per-item code)
__global__ __launch_bounds__(64) void k_blsw_apk_list(uint32_t n, const uint32_t* item, KeyTab kt,
                                                      const uint32_t* pk_off, const uint32_t* pk_cnt,
                                                      const uint32_t* pk_idx, const uint32_t* kmode, uint32_t* rec,
                                                      int32_t* st_apk) {
    __shared__ uint32_t xa[32 * G2J_WORDS];
    if (blockIdx.x >= n) return;
    blsw_apk_item(xa, item[blockIdx.x], kt, pk_off, pk_cnt, pk_idx, kmode, rec, st_apk);
}
// ---- the dense key-sum stage of large wave calls (nwv_bls_set_apk_dense_min, DESIGN §3.6.5;
// bls_verify.h's blsd_* steps, bls_apk_dense.h's routing)
//
// the key table's total, one workgroup: tot = the sum of every key's [h_eff] pk record as a
// G2J_WORDS record, tot[G2J_WORDS] = 1 when every key of the table is cached with status OK (else
// 0: no item then takes its sum from the total)
constexpr int DT_WORDS = G2J_WORDS + 1;
__global__ __launch_bounds__(64) void k_blsd_total(DenseKeys t, uint32_t* tot) {
    __shared__ uint32_t xa[32 * G2J_WORDS];
    const int lane = (int)threadIdx.x;
    bool ok;
    jac<fp2> acc = blsd_total_lane(t, (uint32_t)lane, 64u, ok);
    const bool all_ok = __all(ok);
#pragma unroll 1
    for (int h = 32; h >= 1; h >>= 1) {
        __syncthreads();
        if (lane >= h && lane < 2 * h) st_g2j(xa + (lane - h) * G2J_WORDS, acc);
        __syncthreads();
        if (lane < h) acc = jac_add(acc, ld_g2j(xa + lane * G2J_WORDS));
    }
    if (lane != 0) return;
    if (!all_ok) acc = blsd_identity();
    st_g2j(tot, acc);
    tot[G2J_WORDS] = all_ok ? 1u : 0u;
}
// L lanes an item, 64 / L items a wave: item item[q]'s key sum over its list of key NUMBERS
// (idx0: the caller's indices into the call's key table, not cache slots), written where
// blsw_apk_item writes it.  mode[q] = 1 when the sum came from the total (a strictly ascending
// list over more than half of a wholly registered table), else 0 (summed directly).
template <int L>
__global__ __launch_bounds__(64) void k_blsd_apk(uint32_t n, const uint32_t* item, DenseKeys t, const uint32_t* pk_off,
                                                 const uint32_t* pk_cnt, const uint32_t* idx0, const uint32_t* tot,
                                                 uint32_t* rec, int32_t* st_apk, uint32_t* mode) {
    static_assert(L == 4 || L == 8 || L == 16, "lanes per item");
    constexpr int PER = 64 / L;
    __shared__ uint32_t lds[32 * G2J_WORDS];
    const uint32_t s = threadIdx.x % L, q = blockIdx.x * PER + threadIdx.x / L;
    uint32_t* xa = lds + (threadIdx.x / L) * (L / 2) * G2J_WORDS;  // the group's L / 2 records
    const bool live = q < n;  // (a lane past the list walks nothing: every lane reaches the barriers)
    const uint32_t i = live ? item[q] : 0u;
    const uint32_t cnt = live ? pk_cnt[i] : 0u;
    const uint32_t* idx = idx0 + (live ? pk_off[i] : 0u);
    bool asc = blsd_lane_ascending(idx, cnt, s, L);
    for (int m = L / 2; m >= 1; m >>= 1) asc = __shfl_xor((int)asc, m) && asc;
    const bool comp = asc && tot[G2J_WORDS] != 0 && cnt > t.n_keys / 2;
    uint32_t first_bad = 0xffffffffu;
    jac<fp2> acc = comp ? blsd_lane_absent(t, idx, cnt, s, L) : blsd_lane_direct(t, idx, cnt, s, L, first_bad);
    for (int m = L / 2; m >= 1; m >>= 1) first_bad = min(first_bad, (uint32_t)__shfl_xor((int)first_bad, m));
#pragma unroll 1
    for (int h = L / 2; h >= 1; h >>= 1) {
        __syncthreads();
        if (s >= (uint32_t)h && s < 2u * h) st_g2j(xa + (s - h) * G2J_WORDS, acc);
        __syncthreads();
        if (s < (uint32_t)h) acc = jac_add(acc, ld_g2j(xa + s * G2J_WORDS));
    }
    if (s != 0 || !live) return;
    const int32_t status = blsd_finish(t, idx, acc, comp, comp ? ld_g2j(tot) : acc, first_bad);
    st_g2j(rec + (size_t)G2J_WORDS * i, acc);
    st_apk[i] = status;
    mode[q] = comp ? 1u : 0u;
}
// hash to G1 (blocks [0, n)) and the key sums (blocks [n, 2n)) as one launch (one stream per
// call side): independent waves, the LDS of the larger of the two
__global__ __launch_bounds__(64) void k_blsw_pre(uint32_t n, const uint8_t* msg, const uint64_t* off,
                                                 const uint32_t* len, const uint8_t* dst, uint32_t dl, uint32_t* hrec,
                                                 KeyTab kt, const uint32_t* pk_off, const uint32_t* pk_cnt,
                                                 const uint32_t* pk_idx, const uint32_t* kmode, uint32_t* arec,
                                                 int32_t* st_apk) {
    constexpr int LW = wave::WM_WORDS > 32 * G2J_WORDS ? wave::WM_WORDS : 32 * G2J_WORDS;
    __shared__ uint32_t lds[LW];
    const uint32_t b = blockIdx.x;
    if (b < n)
        blsw_h2c_item(lds + wave::KP_WORDS, b, msg, off, len, dst, dl, hrec, kmode);
    else if (b < 2 * n)
        blsw_apk_item(lds, b - n, kt, pk_off, pk_cnt, pk_idx, kmode, arec, st_apk);
}
// k_blsw_pre of a call that uses the device's message ring (bls_msg_ring.h; `ring`: G1H_REC_WORDS
// u32 a slot, raw hashed points).  hsrc[i]: the slot that holds item i's message (a hit: no
// hashing, the record copied for a key-side item, run through the h_eff chain otherwise) or
// MR_NONE; hpub[i]: the slot a miss also writes its raw point to, or MR_NONE.  Items of one call
// that share a missing message each compute on their own (no cross-block wait); the host gives
// only the first of them a slot.  The host keeps every slot named here away from other calls'
// writes until this call's stream has completed (pins, busy flags).
constexpr uint32_t MR_NONE = 0xffffffffu;
__global__ __launch_bounds__(64) void k_blsw_pre_r(uint32_t n, const uint8_t* msg, const uint64_t* off,
                                                   const uint32_t* len, const uint8_t* dst, uint32_t dl, uint32_t* hrec,
                                                   KeyTab kt, const uint32_t* pk_off, const uint32_t* pk_cnt,
                                                   const uint32_t* pk_idx, const uint32_t* kmode, uint32_t* arec,
                                                   int32_t* st_apk, uint32_t* ring, const uint32_t* hsrc,
                                                   const uint32_t* hpub) {
    constexpr int LW = wave::WM_WORDS > 32 * G2J_WORDS ? wave::WM_WORDS : 32 * G2J_WORDS;
    __shared__ uint32_t lds[LW];
    const uint32_t b = blockIdx.x;
    if (b < n) {
        const wave::Wave w{lds + wave::KP_WORDS, (int)threadIdx.x};
        const uint32_t src = hsrc[b], pub = hpub[b];
        w_hash_ring_item(w, msg + off[b], len[b], dst, dl,
                         src != MR_NONE ? ring + (size_t)G1H_REC_WORDS * src : nullptr,
                         pub != MR_NONE ? ring + (size_t)G1H_REC_WORDS * pub : nullptr, kmode && kmode[b],
                         hrec + (size_t)G1H_REC_WORDS * b);
    } else if (b < 2 * n) {
        blsw_apk_item(lds, b - n, kt, pk_off, pk_cnt, pk_idx, kmode, arec, st_apk);
    }
}
// hashing ahead of need: one wave per message, the raw point alone, into the message's reserved
// ring slot
__global__ __launch_bounds__(64) void k_blsw_h2c_ahead(uint32_t n, const uint8_t* msg, const uint64_t* off,
                                                       const uint32_t* len, const uint8_t* dst, uint32_t dl,
                                                       uint32_t* ring, const uint32_t* slot) {
    BLSW_LDS(wave::NSLOTS);
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const wave::Wave w{wm, (int)threadIdx.x};
    w_hash_to_g1(w, msg + off[i], len[i], dst, dl, ring + (size_t)G1H_REC_WORDS * slot[i], false);
}

// AggregateAuthenticator::aggregate (types/src/primary.rs:476-477) on the wave engine: a wave adds
// up to 16 points with the smallest g1_sum program that holds them (2, 4, 8, 16 inputs: one level
// of complete additions, about three stages, per doubling).  The inputs (w_g1_sum_put's forms:
// affine records, optionally through a list of positions, or partial sums) are fetched in one
// batch -- every lane issues all its loads before any is stored -- rather than point by point.
// points [first, first + k) of the input (k <= G1SUM_N; those at or past m are the identity)
__device__ __forceinline__ void blsw_sum_load(uint32_t* wm, const uint32_t* in, const uint32_t* idx, int hom,
                                              uint32_t first, uint32_t m, uint32_t k) {
    using namespace wave;
    const int lane = (int)threadIdx.x;
    constexpr int PW = 3 * NL, T = (G1SUM_N * PW + 63) / 64;
    static_assert(T <= 32, "one mask bit per word");
    const int tot = (int)k * PW;
    init_slots(Wave{wm, lane});
    uint32_t v[T], one_at = 0;
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int wd = lane + 64 * t, q = wd / PW, c = (wd % PW) / NL, l = wd % NL;
        const uint32_t j = first + (uint32_t)q;
        uint32_t x = 0;
        bool one = false;
        if (wd < tot) {
            if (j >= m) {
                one = c == 1;  // the identity (0 : 1 : 0)
            } else if (hom) {
                x = in[(size_t)PW * j + (wd % PW)];
            } else {
                const uint32_t* r = in + (size_t)G1_REC_WORDS * (idx ? idx[j] : j);
                if (r[2 * NL]) one = c == 1;
                else if (c < 2) x = r[c * NL + l];
                else one = true;
            }
        }
        v[t] = x;
        one_at |= (one ? 1u : 0u) << t;
    }
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int wd = lane + 64 * t;
        if (wd < tot)
            wm[SW * g1sum_slot(wd / PW) + (wd % PW)] = (one_at >> t) & 1u ? wm[SW * SLOT_ONE + wd % NL] : v[t];
    }
    wsync();
}
// block b: points [b per, b per + per) (per <= G1SUM_N) -> partial sum b
__global__ __launch_bounds__(64) void k_blsw_g1_sum(uint32_t m, const uint32_t* in, const uint32_t* idx, int hom,
                                                    uint32_t* part, uint32_t per) {
    BLSW_LDS(wave::NSLOTS);
    const uint32_t first = blockIdx.x * per;
    if (first >= m) return;
    const uint32_t cnt = min(per, m - first);
    blsw_sum_load(wm, in, idx, hom, first, m, g1_sum_width(cnt));
    const wave::Wave w{wm, (int)threadIdx.x};
    w.run(g1_sum_prog(cnt));
    w.get_words(wave::REG_U, part + (size_t)G1P_WORDS * blockIdx.x, 3);
}
// the last level (m <= G1SUM_N inputs, one block): the first bad status of the n_st items in list
// order (st: null when every item is known good), else the compressed sum
__global__ __launch_bounds__(64) void k_blsw_g1_sum_fin(uint32_t m, const uint32_t* in, const uint32_t* idx, int hom,
                                                        uint32_t n_st, const int32_t* st, uint8_t* out48,
                                                        int32_t* out_st) {
    BLSW_LDS(wave::NSLOTS);
    const int lane = (int)threadIdx.x;
    if (blockIdx.x) return;
    if (st) {
        uint32_t bad = 0xffffffffu;
        for (uint32_t k = (uint32_t)lane; k < n_st; k += 64)
            if (st[k] != ST_OK) {
                bad = k;
                break;
            }
        for (int o = 32; o >= 1; o >>= 1) bad = min(bad, (uint32_t)__shfl_xor((int)bad, o));
        if (bad != 0xffffffffu) {
            if (lane == 0) *out_st = st[bad];
            return;
        }
    }
    blsw_sum_load(wm, in, idx, hom, 0, m, g1_sum_width(m));
    const wave::Wave w{wm, lane};
    w.run(g1_sum_prog(m));
    w_g1_sum_compress(w, out48);
    if (lane == 0) *out_st = ST_OK;
}

// the oracle's order: signature decode, its G1 check, the keys, the pairing equation
// (sc_rec: a verified signature's record is also kept in the signature ring, at slot sc_slot[i])
__global__ __launch_bounds__(BLS_LANES) void k_blsw_status(uint32_t n, const int32_t* dec, const int32_t* sub,
                                                           const int32_t* apk, const int32_t* pair, int32_t* st,
                                                           const uint32_t* srec, uint32_t* sc_rec, const uint32_t* sc_slot) {
    BLS_IDX();
    const int32_t s = dec[i] != ST_OK ? dec[i] : sub[i] != ST_OK ? sub[i] : apk[i] != ST_OK ? apk[i] : pair[i];
    st[i] = s;
    if (sc_rec && s == ST_OK) {
        uint32_t* d = sc_rec + (size_t)G1_REC_WORDS * sc_slot[i];
        const uint32_t* r = srec + (size_t)G1_REC_WORDS * i;
        for (int k = 0; k < G1_REC_WORDS; k++) d[k] = r[k];
    }
}

// ------------------------------------------------------------------------------- host side
namespace {

#define BLS_HIP(x)                                                                  \
    do {                                                                            \
        const hipError_t e_ = (x);                                                  \
        if (e_ != hipSuccess) return nwv_internal_set_err(NWV_ERR_HIP, hipGetErrorString(e_)); \
    } while (0)

struct DBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t n) {
        if (n <= cap) return NWV_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        if (hipMalloc(&p, n) != hipSuccess) return nwv_internal_set_err(NWV_ERR_OOM, "hipMalloc (bls)");
        cap = n;
        return NWV_OK;
    }
    ~DBuf() {
        if (p) (void)hipFree(p);
    }
};
struct HBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t n) {
        if (n <= cap) return NWV_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        if (hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess)
            return nwv_internal_set_err(NWV_ERR_OOM, "hipHostMalloc (bls)");
        cap = n;
        return NWV_OK;
    }
    ~HBuf() {
        if (p) (void)hipHostFree(p);
    }
};

// The committee key cache of a device.  fastcrypto validates a BLS public key once, when it is
// deserialized; here nwv_bls_keycache_register (epoch start: the committee's keys) decodes and
// subgroup-checks keys once and keeps the records of the VALID ones.  Verification calls only look
// keys up: a key the cache does not hold (a stray key, a single verify by an outsider, an invalid
// key) is decoded into the call's own scratch table and never takes a slot.  Slots are published
// only after the fill kernel has completed; reset (epoch change) waits for calls in flight, which
// hold the lock shared while their kernels read the records.
struct BlsKeyCache {
    std::shared_mutex mu;
    DBuf rec, st;  // KC_CAP x G2_REC_WORDS u32 records, KC_CAP int32 statuses
    DBuf hrec;     // KC_CAP x G2_REC_WORDS: [h_eff] pk of each slot
    DBuf lines;    // line tables of slots [0, used): KL_WORDS u32 each (grown as keys register)
    uint32_t lines_slots = 0;
    std::unordered_map<std::string, uint32_t> slot;
    uint32_t used = 0;
};

// One call in flight: its streams, staging arena and scratch.  A device keeps a pool of these, so
// concurrent callers run their pipelines side by side instead of queueing on one device lock.
struct BlsLane {
    hipStream_t stream = nullptr;              // H2D, signatures, pairing check, D2H
    hipStream_t side[2] = {nullptr, nullptr};  // keys + key sums (+ hash to G1 on small wave calls); hash to G1
    bool high = false;  // a reserved lane (lane_pool.h): its streams, side[1] included, at the greatest priority
    HBuf stage;
    DBuf in, work;
    // the key-transposed batch check's own buffers (sized by the plan, made after the pre-pairing
    // kernels: the call's arena and scratch never move under it): the statuses and verdicts on
    // the host, the plan's lists on both sides, the check's records
    HBuf kb_st, kb_up;
    DBuf kb_in, kb_work;
    // [0,1] keys, [1,2] key sums (side 0); [3,4] signatures (main); [5,6] hash to G1 (side 1; side
    // 0 on small wave calls); [7,8] pairing check (main); [9] inputs resident, [10] side 0 done,
    // [11] side 1 done.  side[1] is created by the first call that needs it: a lane of small wave
    // calls holds two streams, so the eight ordinary lanes map one to one onto 16 hardware queues
    hipEvent_t ev[12] = {};
    // ordering only (no timestamps): [0] inputs resident, [1] signatures decoded (small wave calls),
    // [2] key sums done (small wave calls that fill aggregate-key ring slots)
    hipEvent_t sev[3] = {};
    ~BlsLane() {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
        for (auto& e : sev)
            if (e) (void)hipEventDestroy(e);
        for (auto& t : side)
            if (t) (void)hipStreamDestroy(t);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// Signatures that passed a wave-path verify call of up to wave_max items, kept decoded (affine G1
// records) by their 48 bytes: AggregateAuthenticator::aggregate over votes the Core has already
// verified (primary/src/aggregators.rs VotesAggregator::append -> types/src/primary.rs:476) then
// sums kept records instead of decoding and G1-checking each signature again.  A ring of SC_CAP
// records: a verify call reserves n slots (unmapping what they held) under the unique lock before
// its kernels run, k_blsw_status writes the verified records into them, and the call maps them
// after its stream synchronises.  A reserved slot stays `busy` until its call maps or releases
// it, and the cursor steps over busy slots, so no two calls in flight ever write one slot.  An
// aggregate holds the shared lock from its lookups until its stream synchronises, so no slot it
// reads is reserved while its kernels run.
struct Sig48 {
    uint8_t b[48];
    bool operator==(const Sig48& o) const { return std::memcmp(b, o.b, 48) == 0; }
};
struct Sig48Hash {
    size_t operator()(const Sig48& s) const {  // the x coordinate's low 64 bits (big-endian bytes 40..47)
        uint64_t h;
        std::memcpy(&h, s.b + 40, 8);
        return (size_t)(h * 0x9e3779b97f4a7c15ull);
    }
};
struct BlsSigCache {
    std::shared_mutex mu;
    DBuf rec;  // SC_CAP x G1_REC_WORDS
    std::unordered_map<Sig48, uint32_t, Sig48Hash> slot;
    std::vector<Sig48> key;     // the signature slot s holds (when held[s])
    std::vector<uint8_t> held;  // slot s is mapped
    std::vector<uint8_t> busy;  // reserved by a call still in flight
    uint32_t next = 0;
    // n free slots from the ring's cursor (busy ones skipped: at most kMaxBusySlots are, one
    // keeping call of up to 1,024 items on each of a device's lanes, reserved ones included),
    // unmapped and marked busy -> out
    int reserve(size_t n, std::vector<uint32_t>& out) {
        std::unique_lock<std::shared_mutex> lk(mu);
        if (!rec.p) {
            int rc = rec.ensure((size_t)4 * G1_REC_WORDS * SC_CAP);
            if (rc) return rc;
            key.resize(SC_CAP);
            held.assign(SC_CAP, 0);
            busy.assign(SC_CAP, 0);
            slot.reserve(SC_CAP);
        }
        out.clear();
        for (size_t i = 0; i < n; i++) {
            uint32_t t = next, seen = 0;
            while (busy[t] && ++seen < SC_CAP) t = (t + 1) % SC_CAP;
            if (busy[t]) {  // only after failed calls abandoned their slots (SigSlots)
                for (uint32_t u : out) busy[u] = 0;
                out.clear();
                return nwv_internal_set_err(NWV_ERR_HIP, "bls signature ring: no free slot");
            }
            if (held[t]) {
                auto it = slot.find(key[t]);
                if (it != slot.end() && it->second == t) slot.erase(it);
                held[t] = 0;
            }
            busy[t] = 1;
            out.push_back(t);
            next = (t + 1) % SC_CAP;
        }
        return NWV_OK;
    }
    // the call's verified signatures (status OK) mapped to their slots (status null: the call
    // failed, its slots are only released)
    void publish(size_t n, const uint8_t* sigs, const int32_t* status, const std::vector<uint32_t>& slots) {
        std::unique_lock<std::shared_mutex> lk(mu);
        for (size_t i = 0; i < slots.size() && i < n; i++) {
            const uint32_t t = slots[i];
            busy[t] = 0;
            if (!status || status[i] != ST_OK) continue;
            std::memcpy(key[t].b, sigs + 48 * i, 48);
            held[t] = 1;
            slot[key[t]] = t;
        }
    }
};
// a call's reserved ring slots, released unless the call publishes them.  A call that fails
// after its kernels were queued may still have k_blsw_status writing into them: the release
// first waits for the call's stream, and if that wait fails too the slots stay busy (abandoned)
// so no other call can ever map a slot a late write may still land in.
struct SigSlots {
    BlsSigCache* sc = nullptr;
    std::vector<uint32_t> slots;
    size_t n = 0;
    hipStream_t stream = nullptr;  // the stream k_blsw_status writes the slots on
    ~SigSlots() {
        if (!sc) return;
        if (stream && hipStreamSynchronize(stream) != hipSuccess) return;  // abandoned, see above
        sc->publish(n, nullptr, nullptr, slots);
    }
};

constexpr size_t kMaxLanes = 8;  // ordinary lanes of a device; up to LATENCY_LANES_MAX reserved ones beside them
// the verified-signature ring's busy slots at any moment: every lane, ordinary or reserved, runs at
// most one call, and a call that keeps its signatures has at most 1,024 items (verify_on)
constexpr size_t kMaxBusySlots = (kMaxLanes + nwv::LATENCY_LANES_MAX) * 1024;
static_assert(kMaxBusySlots + 1024 <= SC_CAP, "a keeping call always finds 1,024 free ring slots");

// The hashed message points of a device (nwv_bls_set_msg_ring; bls_msg_ring.h keeps the books).
// Small wave calls look their messages up, pin the hits and reserve a slot per distinct miss
// before their kernels run; k_blsw_pre_r reads the pinned records and fills the reserved ones; the
// call publishes and unpins after its streams have synchronised.  No lock is held meanwhile.
struct BlsMsgCache {
    nwv::BlsMsgRing ring;
    DBuf rec;                     // ring.cap() x G1H_REC_WORDS u32: raw points
    std::atomic<bool> on{false};  // lookups and publishes (the buffer, once there, stays)
};
// a call's ring slots: the hits it pinned and the slots it reserved (for its own misses and for its
// ahead messages).  finish() publishes and unpins after the call's streams have synchronised; a
// call that fails before that synchronises them here and gives everything back, and if that wait
// fails too the slots stay pinned / busy (abandoned, as SigSlots does).
struct MsgSlots {
    struct Fresh {
        uint32_t slot;
        nwv::MsgKey key;
        uint32_t gate;  // ahead messages: the item whose OK status lets it publish, or UINT32_MAX
        bool ahead;
    };
    nwv::BlsMsgRing* ring = nullptr;
    std::vector<uint32_t> pinned;
    std::vector<Fresh> fresh;
    hipStream_t streams[2] = {nullptr, nullptr};
    // status: the call's per-item statuses (null: no gates to read).  out[3] += published item
    // slots, out[4] += published ahead slots
    void finish(const int32_t* status, uint64_t* out) {
        if (!ring) return;
        for (const Fresh& f : fresh) {
            if (f.ahead && f.gate != UINT32_MAX && (!status || status[f.gate] != ST_OK)) {
                ring->release(f.slot);
                continue;
            }
            if (ring->publish(f.slot, f.key) == f.slot && out) out[f.ahead ? 4 : 3]++;
        }
        for (uint32_t s : pinned) ring->unpin(s);
        ring = nullptr;
    }
    ~MsgSlots() {
        if (!ring) return;
        for (hipStream_t s : streams)
            if (s && hipStreamSynchronize(s) != hipSuccess) return;  // abandoned, see above
        for (const Fresh& f : fresh) ring->release(f.slot);
        for (uint32_t s : pinned) ring->unpin(s);
    }
};
// The aggregate keys of a device (nwv_bls_set_apk_ring; bls_apk_ring.h keeps the books): per slot
// the affine sum of a signer set's [h_eff] pk records and that point's line table.  A small wave
// call looks the sets of its key-side items up and pins the hits, whose items then run as one-key
// items on the slot; a set missed for the second time reserves a slot, k_blsw_apk_fill writes it
// beside the pairing kernel, and the call publishes it after its streams have synchronised if the
// item verified.  The sets are lists of key-cache slots: nwv_bls_keycache_reset empties the ring.
struct BlsApkCache {
    nwv::BlsApkRing ring;
    DBuf rec;                     // ring.cap() x G2_REC_WORDS u32
    DBuf lines;                   // ring.cap() x KL_WORDS u32
    std::atomic<bool> on{false};  // lookups and publishes (the buffers, once there, stay)
};
// a call's aggregate-key slots: the hits it pinned and the slots it reserved.  finish() publishes
// (behind each item's status) and unpins after the call's streams have synchronised; a call that
// fails before that synchronises them here and gives everything back, and if that wait fails too
// the slots stay pinned / busy (abandoned, as MsgSlots does).
struct ApkSlots {
    struct Fresh {
        uint32_t slot, item;
        nwv::ApkKey key;
    };
    nwv::BlsApkRing* ring = nullptr;
    std::vector<uint32_t> pinned;
    std::vector<Fresh> fresh;
    hipStream_t streams[2] = {nullptr, nullptr};
    // a set is kept only if the item that reserved its slot verified: out[3] += published slots
    void finish(const int32_t* status, uint64_t* out) {
        if (!ring) return;
        for (const Fresh& f : fresh) {
            if (status[f.item] != ST_OK)
                ring->release(f.slot);
            else if (ring->publish(f.slot, f.key) == f.slot)
                out[3]++;
        }
        for (uint32_t s : pinned) ring->unpin(s);
        ring = nullptr;
    }
    ~ApkSlots() {
        if (!ring) return;
        for (hipStream_t s : streams)
            if (s && hipStreamSynchronize(s) != hipSuccess) return;  // abandoned, see above
        for (const Fresh& f : fresh) ring->release(f.slot);
        for (uint32_t s : pinned) ring->unpin(s);
    }
};
// a call's ahead messages (nwv_bls_verify_many_ahead)
struct Ahead {
    size_t n = 0;
    const uint8_t* base = nullptr;
    const uint64_t* off = nullptr;
    const uint32_t* len = nullptr;
    const uint32_t* gate = nullptr;
};

struct BlsDev {
    int ordinal = -1;
    uint32_t flags = 0;  // the context's nwv_init flags
    BlsKeyCache kc;
    BlsSigCache sc;
    BlsMsgCache mr;
    BlsApkCache ar;
    // the lanes: kMaxLanes ordinary ones, and NWV_LATENCY_LANES reserved ones for calls of at most
    // latency_max items (nwv_set_latency_max; 0: no call is latency class), lane_pool.h
    nwv::LanePool<BlsLane> pool;
    std::atomic<size_t> latency_max{0};
    bool latency_priority = true;  // (env NWV_LATENCY_PRIORITY=0: reserved lanes at default priority)
    BlsDev() { pool.set_caps(kMaxLanes, nwv::latency_lanes_from_env()); }
    ~BlsDev() {
        for (BlsLane* l : pool.all()) delete l;
    }
    std::mutex stat_mu;  // the last completed verify_many call's stage times and path
    double last_ms[5] = {0, 0, 0, 0, 0};
    int last_path = 0;
    uint64_t last_keys[2] = {0, 0};  // key-list entries found in the cache, distinct keys decoded
    uint64_t last_batch[3] = {0, 0, 0};  // wave batch check: groups formed, rejected, items re-checked
    // nwv_bls_set_wave_batch_min: large wave calls of at least this many items take the wave batch
    // check (0: never)
    std::atomic<size_t> wave_batch_min{0};
    // nwv_bls_set_key_batch_min: large wave calls of at least this many items take the
    // key-transposed batch check (0: never); it goes before the wave batch check
    std::atomic<size_t> key_batch_min{0};
    // its last call: groups formed, rejected, items re-checked, Miller loops, items in the groups
    uint64_t last_kbatch[5] = {0, 0, 0, 0, 0};
    // nwv_bls_set_apk_dense_min: large wave calls of at least this many items sum their keys in the
    // dense stage (k_blsd_total, k_blsd_apk, k_blsw_apk_list) in place of k_blsw_apk (0: never)
    std::atomic<size_t> apk_dense_min{0};
    // its last call: items summed directly, by complement, left to the per-item kernel, lanes an item
    uint64_t last_apkd[4] = {0, 0, 0, 0};
};
// the BLS engine's state of one context: one BlsDev per device of the context (nwv_init with
// several devices shards nwv_bls_verify_many by item index, bls_shard.h).  Diagnostic / test hook:
// env NWV_BLS_DEVICE_REPLICAS=r gives every device r independent BlsDev shards (own key cache,
// ring and lanes), so the split, the per-shard key registration and the status merge run on a
// one-GPU box too.
struct BlsCtx {
    std::vector<BlsDev*> devs;
    // the devices' load (place.h): the Ed25519 engine's table when both engines have the same number
    // of device objects (device object j of either then counts on entry j, one load per device),
    // else a table of this engine's own
    nwv::PlaceTable* place = nullptr;
    std::unique_ptr<nwv::PlaceTable> own_place;
};
std::mutex g_mu;
std::unordered_map<nwv_ctx*, BlsCtx*> g_devs;

int ctx_of(nwv_ctx* ctx, BlsCtx** out) {
    if (!ctx) return nwv_internal_set_err(NWV_ERR_ARG, "null context");
    std::lock_guard<std::mutex> g(g_mu);
    auto it = g_devs.find(ctx);
    if (it != g_devs.end()) {
        *out = it->second;
        return NWV_OK;
    }
    // one BlsDev per HIP device of the context times this engine's own replicas (the Ed25519
    // engine's replicas, NWV_DEVICE_REPLICAS, are that engine's device objects, not devices)
    const int nd = nwv_internal_hip_device(ctx, -1);
    if (nd <= 0 || nwv_internal_hip_device(ctx, 0) < 0) return nwv_internal_set_err(NWV_ERR_NODEV, "context has no device");
    static const int replicas = [] {
        const char* e = std::getenv("NWV_BLS_DEVICE_REPLICAS");
        const int r = e ? std::atoi(e) : 1;
        return r < 1 ? 1 : (r > 8 ? 8 : r);
    }();
    auto* c = new BlsCtx;
    for (int k = 0; k < nd; k++)
        for (int r = 0; r < replicas; r++) {
            auto* d = new BlsDev;
            d->ordinal = nwv_internal_hip_device(ctx, k);
            d->flags = nwv_internal_ctx_flags(ctx);
            d->latency_priority = nwv::latency_priority_from_env();
            c->devs.push_back(d);
        }
    nwv::PlaceTable* shared = nwv_internal_place(ctx);
    if (shared && shared->size() == c->devs.size()) {
        c->place = shared;
    } else {
        c->own_place.reset(new nwv::PlaceTable(c->devs.size(), nwv::place_mode_from_env()));
        c->place = c->own_place.get();
    }
    g_devs[ctx] = c;
    *out = c;
    return NWV_OK;
}

// the context's first device (single-device entry points: keygen, sign, hash, pairing)
int dev_of(nwv_ctx* ctx, BlsDev** out) {
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    *out = c->devs[0];
    return NWV_OK;
}

// the device that served the calling thread's last nwv_bls_verify_many on a context (range 0's, when
// the call split): what nwv_bls_last_kernel_ms / _last_path / _last_keys read; device 0 if none
thread_local std::unordered_map<const nwv_ctx*, size_t> t_last_dev;
int last_dev_of(nwv_ctx* ctx, BlsDev** out) {
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    const auto it = t_last_dev.find(ctx);
    *out = c->devs[(it != t_last_dev.end() && it->second < c->devs.size()) ? it->second : 0];
    return NWV_OK;
}

// fn(dev) on every device of the context (one host thread each), first nonzero rc in device order
template <class Fn>
int on_all_devices(BlsCtx& c, Fn fn) {
    std::vector<std::pair<size_t, size_t>> r;
    for (size_t k = 0; k < c.devs.size(); k++) r.push_back({k, k + 1});
    std::vector<std::string> err(c.devs.size());
    const int rc = bls_for_ranges(r, [&](size_t k, size_t, size_t) {
        const int e = fn(*c.devs[k]);
        if (e) err[k] = nwv_last_error();
        return e;
    });
    if (rc)
        for (size_t k = 0; k < err.size(); k++)
            if (!err[k].empty()) return nwv_internal_set_err(rc, err[k].c_str());
    return rc;
}

// a lane of the device's pool for the duration of one call, by the rule of lane_pool.h (created on
// demand: at most kMaxLanes ordinary lanes, and the reserved ones that only latency-class calls take)
class LaneLease {
  public:
    explicit LaneLease(BlsDev& d, bool latency = false) : d_(d) {
        lane_ = d.pool.lease(latency, [&](bool reserved) -> BlsLane* {
            auto l = std::make_unique<BlsLane>();
            l->high = reserved && d.latency_priority;
            if (hipSetDevice(d.ordinal) != hipSuccess || nwv::lane_stream_create(&l->stream, l->high) != hipSuccess ||
                nwv::lane_stream_create(&l->side[0], l->high) != hipSuccess) {
                rc_ = nwv_internal_set_err(NWV_ERR_HIP, "bls stream");
                return nullptr;
            }
            for (auto& e : l->ev)
                if (hipEventCreate(&e) != hipSuccess) {
                    rc_ = nwv_internal_set_err(NWV_ERR_HIP, "bls event");
                    return nullptr;
                }
            for (auto& e : l->sev)
                if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
                    rc_ = nwv_internal_set_err(NWV_ERR_HIP, "bls event");
                    return nullptr;
                }
            return l.release();
        });
        if (lane_ && hipSetDevice(d.ordinal) != hipSuccess) rc_ = nwv_internal_set_err(NWV_ERR_HIP, "hipSetDevice (bls)");
    }
    ~LaneLease() {
        if (lane_) d_.pool.give_back(lane_);
    }
    int rc() const { return rc_; }
    BlsLane& operator*() { return *lane_; }
    BlsLane* operator->() { return lane_; }

  private:
    BlsDev& d_;
    BlsLane* lane_ = nullptr;
    int rc_ = NWV_OK;
};

// an arena of sections placed 256-byte aligned, filled on the host, copied with one H2D
struct Arena {
    std::vector<std::pair<const void*, size_t>> parts;
    std::vector<size_t> offs;
    size_t total = 0;
    size_t add(const void* p, size_t n) {
        const size_t o = total;
        parts.push_back({p, n});
        offs.push_back(o);
        total += (n + 255) & ~(size_t)255;
        return o;
    }
};

constexpr int kBlocks(size_t n) { return (int)((n + BLS_LANES - 1) / BLS_LANES); }
// blocks of the group kernels: 8 items per 64-lane block
constexpr int gBlocks(size_t n) { return (int)((n + BLS_LANES / GRP - 1) / (BLS_LANES / GRP)); }
size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// Key registration: the keys the cache does not hold are decoded and subgroup-checked into a
// scratch table, then (after the stream has completed) the valid ones are copied into fresh
// slots and published.  Invalid keys take no slot; a failure publishes nothing.
int keycache_register(BlsDev& d, size_t n_keys, const uint8_t* keys) {
    if (d.flags & NWV_FLAG_NO_KEYCACHE) return NWV_OK;
    {  // fast path: every key already held
        std::shared_lock<std::shared_mutex> g(d.kc.mu);
        bool all = d.kc.rec.p != nullptr;
        for (size_t j = 0; j < n_keys && all; j++)
            all = d.kc.slot.count(std::string(reinterpret_cast<const char*>(keys + 96 * j), 96)) != 0;
        if (all) return NWV_OK;
    }
    LaneLease lane(d);
    if (lane.rc()) return lane.rc();
    std::unique_lock<std::shared_mutex> g(d.kc.mu);
    int rc;
    if ((rc = d.kc.rec.ensure((size_t)4 * G2_REC_WORDS * KC_CAP)) || (rc = d.kc.st.ensure((size_t)4 * KC_CAP)) ||
        (rc = d.kc.hrec.ensure((size_t)4 * G2_REC_WORDS * KC_CAP)))
        return rc;
    std::vector<std::string> fresh;
    std::vector<uint8_t> fk;
    std::unordered_map<std::string, uint32_t> seen;
    for (size_t j = 0; j < n_keys; j++) {
        std::string kb(reinterpret_cast<const char*>(keys + 96 * j), 96);
        if (d.kc.slot.count(kb) || seen.count(kb)) continue;
        seen.emplace(kb, (uint32_t)fresh.size());
        fresh.push_back(kb);
        fk.insert(fk.end(), keys + 96 * j, keys + 96 * (j + 1));
    }
    const size_t m = fresh.size();
    if (m == 0) return NWV_OK;
    // scratch: keys, identity slot list, records, statuses; then the copy lists
    const size_t o_keys = 0, o_slot = al256(96 * m), o_rec = al256(o_slot + 4 * m),
                 o_st = al256(o_rec + 4 * G2_REC_WORDS * m), o_src = al256(o_st + 4 * m), o_dst = al256(o_src + 4 * m),
                 o_end = o_dst + 4 * m;
    if ((rc = lane->work.ensure(o_end)) || (rc = lane->stage.ensure(o_end))) return rc;
    uint8_t* w = static_cast<uint8_t*>(lane->work.p);
    uint8_t* h = static_cast<uint8_t*>(lane->stage.p);
    std::memcpy(h + o_keys, fk.data(), 96 * m);
    auto* hs = reinterpret_cast<uint32_t*>(h + o_slot);
    for (size_t j = 0; j < m; j++) hs[j] = (uint32_t)j;
    BLS_HIP(hipMemcpyAsync(w, h, o_rec, hipMemcpyHostToDevice, lane->stream));
    hipLaunchKernelGGL(k_bls_keys_fill, dim3(kBlocks(m)), dim3(BLS_LANES), 0, lane->stream, (uint32_t)m, w + o_keys,
                       reinterpret_cast<const uint32_t*>(w + o_slot), reinterpret_cast<uint32_t*>(w + o_rec),
                       reinterpret_cast<int32_t*>(w + o_st));
    BLS_HIP(hipGetLastError());
    BLS_HIP(hipMemcpyAsync(h + o_st, w + o_st, 4 * m, hipMemcpyDeviceToHost, lane->stream));
    BLS_HIP(hipStreamSynchronize(lane->stream));
    const auto* kst = reinterpret_cast<const int32_t*>(h + o_st);
    auto* src = reinterpret_cast<uint32_t*>(h + o_src);
    auto* dst = reinterpret_cast<uint32_t*>(h + o_dst);
    size_t nv = 0;
    for (size_t j = 0; j < m && d.kc.used + nv < KC_CAP; j++)
        if (kst[j] == ST_OK) {
            src[nv] = (uint32_t)j;
            dst[nv] = d.kc.used + (uint32_t)nv;
            nv++;
        }
    if (nv == 0) return NWV_OK;
    BLS_HIP(hipMemcpyAsync(w + o_src, h + o_src, o_end - o_src, hipMemcpyHostToDevice, lane->stream));
    hipLaunchKernelGGL(k_bls_rec_copy, dim3(kBlocks(nv * G2_REC_WORDS)), dim3(BLS_LANES), 0, lane->stream,
                       (uint32_t)nv, reinterpret_cast<const uint32_t*>(w + o_src),
                       reinterpret_cast<const uint32_t*>(w + o_dst), reinterpret_cast<const uint32_t*>(w + o_rec),
                       static_cast<uint32_t*>(d.kc.rec.p), static_cast<int32_t*>(d.kc.st.p));
    BLS_HIP(hipGetLastError());
    // the new slots' Miller-loop line tables (the table grows by whole copies: registration is rare)
    const uint32_t need = d.kc.used + (uint32_t)nv;
    if (need > d.kc.lines_slots) {
        uint32_t cap = std::max<uint32_t>(need, std::max<uint32_t>(2 * d.kc.lines_slots, 256u));
        cap = std::min<uint32_t>(cap, (uint32_t)KC_CAP);
        DBuf nb;
        if ((rc = nb.ensure(4 * KL_WORDS * cap))) return rc;
        if (d.kc.used)
            BLS_HIP(hipMemcpyAsync(nb.p, d.kc.lines.p, 4 * KL_WORDS * d.kc.used, hipMemcpyDeviceToDevice,
                                   lane->stream));
        BLS_HIP(hipStreamSynchronize(lane->stream));
        std::swap(d.kc.lines.p, nb.p);
        std::swap(d.kc.lines.cap, nb.cap);
        d.kc.lines_slots = cap;
    }
    hipLaunchKernelGGL(k_bls_key_heff, dim3(kBlocks(nv)), dim3(BLS_LANES), 0, lane->stream, (uint32_t)nv,
                       reinterpret_cast<const uint32_t*>(w + o_dst), static_cast<const uint32_t*>(d.kc.rec.p),
                       static_cast<uint32_t*>(d.kc.hrec.p));
    hipLaunchKernelGGL(k_blsw_key_lines, dim3((unsigned)nv), dim3(64), 0, lane->stream, (uint32_t)nv,
                       reinterpret_cast<const uint32_t*>(w + o_dst), static_cast<const uint32_t*>(d.kc.hrec.p),
                       static_cast<uint32_t*>(d.kc.lines.p));
    BLS_HIP(hipGetLastError());
    BLS_HIP(hipStreamSynchronize(lane->stream));
    for (size_t k = 0; k < nv; k++) d.kc.slot.emplace(fresh[src[k]], dst[k]);  // published after the copy
    d.kc.used += (uint32_t)nv;
    return NWV_OK;
}

// the whole verify_many pipeline on one lane of a device: after one H2D copy, three streams --
//   side 0: the call's keys the cache does not hold, decoded into the scratch table
//           (k_bls_keys_fill), then the key sums (k_bls_apk_g)
//   main  : signature decode + G1 checks (k_bls_sigs)
//   side 1: hash to G1 (k_bls_h2c_g)
// -- then, joined on the main stream, the statuses in the oracle's order and the pairing check
int verify_on(BlsDev& d, size_t n_keys, const uint8_t* keys, size_t n, const uint8_t* sigs, const uint32_t* pk_off,
              const uint32_t* pk_cnt, const uint32_t* pk_idx, size_t n_idx, const uint8_t* msg_base,
              const uint64_t* msg_off, const uint32_t* msg_len, size_t msg_bytes, const uint8_t* dst, size_t dl,
              int32_t* status, const Ahead* ahead = nullptr, uint64_t* mstat = nullptr, uint64_t* astat = nullptr,
              bool latency = false) {
    LaneLease lane(d, latency);
    if (lane.rc()) return lane.rc();
    BlsLane& L = *lane;
    static const uint8_t zero[8] = {0};
    // pairing-check mode: the wave engine per item (default), or the 8-lane group kernels -- one
    // random-linear-combination batch check (NWV_FLAG_BLS_BATCH) or per item (NWV_FLAG_BLS_PER_ITEM)
    const bool group_item = (d.flags & NWV_FLAG_BLS_PER_ITEM) != 0;
    const bool batch = !group_item && (d.flags & NWV_FLAG_BLS_BATCH) != 0;
    const bool wavem = !group_item && !batch;
    // wave-per-item hashing and G1 checks while the call has fewer items than the chip has SIMDs
    // (latency); above that, one item per lane keeps every lane busy (throughput)
    static const size_t wave_max = [] {
        const char* e = std::getenv("NWV_BLS_WAVE_MAX");
        return e ? (size_t)std::strtoul(e, nullptr, 10) : (size_t)1024;
    }();
    const bool wave_small = wavem && n <= wave_max;
    // the wave batch check (one final exponentiation per group of wb_grp items): large wave calls
    // of at least nwv_bls_set_wave_batch_min items
    static const size_t wb_grp = [] {
        const char* e = std::getenv("NWV_BLS_BATCH_GROUP");
        const size_t v = e ? (size_t)std::strtoul(e, nullptr, 10) : (size_t)NWV_BLS_BATCH_GROUP_DEFAULT;
        return v < 1 ? (size_t)1 : v > 4096 ? (size_t)4096 : v;
    }();
    const size_t wb_min = d.wave_batch_min.load(std::memory_order_relaxed);
    const bool wbatch = wavem && !wave_small && wb_min > 0 && n >= wb_min;
    const size_t wb_ng = wbatch ? (n + wb_grp - 1) / wb_grp : 0, wb_m = wbatch ? n + wb_ng : 0;
    // the key-transposed batch check (bls_key_batch.h): large wave calls of at least
    // nwv_bls_set_key_batch_min items; groups of kb_grp eligible items, a group dropped when its
    // distinct keys + 1 exceed 1 / kb_ratio of its items (0: never)
    static const uint32_t kb_grp = [] {
        const char* e = std::getenv("NWV_BLS_KEY_GROUP");
        const unsigned long v = e ? std::strtoul(e, nullptr, 10) : (unsigned long)NWV_BLS_KEY_GROUP_DEFAULT;
        return (uint32_t)(v < 1 ? 1 : v > 65536 ? 65536 : v);
    }();
    static const uint32_t kb_ratio = [] {
        const char* e = std::getenv("NWV_BLS_KEY_GROUP_RATIO");
        const unsigned long v = e ? std::strtoul(e, nullptr, 10) : 4ul;
        return (uint32_t)(v > 1024 ? 1024 : v);
    }();
    const size_t kb_min = d.key_batch_min.load(std::memory_order_relaxed);
    // the dense key-sum stage (bls_apk_dense.h): large wave calls of at least
    // nwv_bls_set_apk_dense_min items; NWV_BLS_APK_LANES forces the lanes an item gets (4, 8, 16)
    static const unsigned long ad_forced = [] {
        const char* e = std::getenv("NWV_BLS_APK_LANES");
        return e ? std::strtoul(e, nullptr, 10) : 0ul;
    }();
    const size_t ad_min = d.apk_dense_min.load(std::memory_order_relaxed);
    const bool ad_run = wavem && !wave_small && ad_min > 0 && n >= ad_min;
    int rc;
    // the call's key table: cache slots (lookups only) or scratch entries KC_CAP + j
    std::shared_lock<std::shared_mutex> kc_hold(d.kc.mu);  // records stay put while our kernels read them
    const bool cached = !(d.flags & NWV_FLAG_NO_KEYCACHE) && d.kc.rec.p != nullptr;
    std::vector<uint32_t> ktab(n_keys), fill_slot;
    std::vector<uint8_t> fill_keys;
    uint64_t hits = 0;
    {
        std::unordered_map<std::string, uint32_t> fresh;
        for (size_t j = 0; j < n_keys; j++) {
            std::string kb(reinterpret_cast<const char*>(keys + 96 * j), 96);
            if (cached) {
                auto it = d.kc.slot.find(kb);
                if (it != d.kc.slot.end()) {
                    ktab[j] = it->second;
                    hits++;
                    continue;
                }
            }
            auto f = fresh.find(kb);
            if (f != fresh.end()) {
                ktab[j] = KC_CAP + f->second;
                continue;
            }
            const uint32_t e = (uint32_t)fresh.size();
            fresh.emplace(std::move(kb), e);
            ktab[j] = KC_CAP + e;
            fill_slot.push_back(e);
            fill_keys.insert(fill_keys.end(), keys + 96 * j, keys + 96 * (j + 1));
        }
    }
    std::vector<uint32_t> remap(n_idx);
    for (size_t t = 0; t < n_idx; t++) remap[t] = ktab[pk_idx[t]];
    // key-side cofactor clearing (wave path): items whose keys are all in the cache use the keys'
    // [h_eff] pk records and line tables, and their hash skips the h_eff chain
    const bool kside = wavem && cached && d.kc.lines_slots;
    std::vector<uint32_t> kmode(kside ? n : 0);
    for (size_t i = 0; i < kmode.size(); i++) {
        bool all = pk_cnt[i] > 0;
        for (uint32_t j = 0; j < pk_cnt[i] && all; j++) all = remap[pk_off[i] + j] < KC_CAP;
        kmode[i] = all ? 1u : 0u;
    }
    // the dense key-sum stage's item lists and lanes (the stage reads the caller's key numbers and
    // the key table itself: an ascending list is ascending in those, not in cache slots)
    nwv::ApkDenseSplit ads;
    if (ad_run) nwv::apk_dense_split(n, kside ? kmode.data() : nullptr, pk_cnt, ads);
    const size_t n_dn = ads.dense.size(), n_rest = ads.rest.size();
    const uint32_t ad_lanes = ad_run ? nwv::apk_dense_lanes(n_dn, ad_forced) : 0;
    const size_t n_dec = fill_slot.size();  // keys decoded by this call
    // verified signatures stay decoded in the device's ring (BlsSigCache) for aggregates
    // (n <= 1,024 whatever NWV_BLS_WAVE_MAX says: the calls in flight on a device's lanes then hold
    // at most kMaxBusySlots busy slots)
    const bool keep = wave_small && n <= 1024 && !(d.flags & NWV_FLAG_NO_SIGCACHE);
    SigSlots kept;
    if (keep) {
        if ((rc = d.sc.reserve(n, kept.slots))) return rc;
        kept.sc = &d.sc;
        kept.n = n;
    }
    // the device's message ring (the same small wave calls): hits pinned, one slot reserved per
    // distinct missing message and per ahead message that is neither cached nor a duplicate
    const bool use_ring = wave_small && n <= 1024 && d.mr.on.load(std::memory_order_acquire) &&
                          dl <= nwv::MsgKey::MAX_DST;
    MsgSlots ms;
    std::vector<uint8_t> rsec;  // the ring's arena section: aoff | hsrc | hpub | aslot | alen | ahead messages
    size_t n_ah = 0, r_hsrc = 0, r_hpub = 0, r_aslot = 0, r_alen = 0, r_amsg = 0;
    uint64_t mcount[5] = {0, 0, 0, 0, 0};
    if (use_ring) {
        nwv::BlsMsgRing& R = d.mr.ring;
        ms.ring = &R;
        ms.streams[0] = L.stream;
        ms.streams[1] = L.side[0];
        std::vector<uint32_t> hsrc(n, MR_NONE), hpub(n, MR_NONE);
        std::unordered_multimap<uint64_t, size_t> mine;  // this call's reserved keys: hash -> ms.fresh index
        auto mine_has = [&](const nwv::MsgKey& k, uint64_t hk) {
            const auto r = mine.equal_range(hk);
            for (auto it = r.first; it != r.second; ++it)
                if (ms.fresh[it->second].key == k) return true;
            return false;
        };
        auto take = [&](const nwv::MsgKey& k, uint32_t gate, bool is_ahead) {
            const uint64_t hk = k.hash();
            if (mine_has(k, hk)) return MR_NONE;
            const uint32_t r = R.reserve();
            if (r == nwv::BlsMsgRing::NONE) return MR_NONE;  // every slot in use: computed, not kept
            mine.emplace(hk, ms.fresh.size());
            ms.fresh.push_back({r, k, gate, is_ahead});
            return r;
        };
        for (size_t i = 0; i < n; i++) {
            mcount[2]++;
            if (msg_len[i] > nwv::MsgKey::MAX_MSG) continue;
            const nwv::MsgKey k = nwv::MsgKey::make(dst, dl, msg_base + msg_off[i], msg_len[i]);
            const uint32_t s = R.lookup_pin(k);
            if (s != nwv::BlsMsgRing::NONE) {
                hsrc[i] = s;
                ms.pinned.push_back(s);
                mcount[2]--;
                mcount[kside && kmode[i] ? 0 : 1]++;
                continue;
            }
            hpub[i] = take(k, UINT32_MAX, false);
        }
        std::vector<uint32_t> aslot, alen;
        std::vector<uint64_t> aoff;
        std::vector<uint8_t> amsg;
        for (size_t j = 0; ahead && j < ahead->n; j++) {
            if (ahead->len[j] > nwv::MsgKey::MAX_MSG) continue;
            const nwv::MsgKey k = nwv::MsgKey::make(dst, dl, ahead->base + ahead->off[j], ahead->len[j]);
            if (R.contains(k)) continue;
            const uint32_t r = take(k, ahead->gate ? ahead->gate[j] : UINT32_MAX, true);
            if (r == MR_NONE) continue;
            aslot.push_back(r);
            alen.push_back(ahead->len[j]);
            aoff.push_back(amsg.size());
            amsg.insert(amsg.end(), ahead->base + ahead->off[j], ahead->base + ahead->off[j] + ahead->len[j]);
        }
        n_ah = aslot.size();
        r_hsrc = 8 * n_ah;
        r_hpub = r_hsrc + 4 * n;
        r_aslot = r_hpub + 4 * n;
        r_alen = r_aslot + 4 * n_ah;
        r_amsg = r_alen + 4 * n_ah;
        rsec.assign(r_amsg + amsg.size() + 1, 0);
        if (n_ah) {
            std::memcpy(rsec.data(), aoff.data(), 8 * n_ah);
            std::memcpy(rsec.data() + r_aslot, aslot.data(), 4 * n_ah);
            std::memcpy(rsec.data() + r_alen, alen.data(), 4 * n_ah);
            if (!amsg.empty()) std::memcpy(rsec.data() + r_amsg, amsg.data(), amsg.size());
        }
        std::memcpy(rsec.data() + r_hsrc, hsrc.data(), 4 * n);
        std::memcpy(rsec.data() + r_hpub, hpub.data(), 4 * n);
    }
    // the device's aggregate-key ring (the same small wave calls): the key-side items of 2 to 1,024
    // keys.  A hit is pinned and its item becomes a one-key item on the ring slot, in arrays of the
    // call's own (made only when some item hit); a set missed for the second time reserves a slot
    // for k_blsw_apk_fill (one item of the call per set)
    const bool use_apk = wave_small && n <= 1024 && kside && d.ar.on.load(std::memory_order_acquire);
    ApkSlots as;
    std::vector<uint32_t> a_off, a_cnt, a_idx, a_fill;  // a_fill: the fills' items, then their slots
    uint64_t acount[4] = {0, 0, 0, 0};
    if (use_apk) {
        nwv::BlsApkRing& R = d.ar.ring;
        as.ring = &R;
        as.streams[0] = L.stream;
        as.streams[1] = L.side[0];
        std::vector<uint32_t> hit(n, nwv::BlsApkRing::NONE);
        for (size_t i = 0; i < n; i++) {
            if (!kmode[i] || !nwv::ApkKey::eligible(pk_cnt[i])) continue;
            nwv::ApkKey k = nwv::ApkKey::make(remap.data() + pk_off[i], pk_cnt[i]);
            const uint32_t s = R.lookup_pin(k);
            if (s != nwv::BlsApkRing::NONE) {
                hit[i] = s;
                as.pinned.push_back(s);
                acount[0]++;
                continue;
            }
            acount[1]++;
            bool mine = false;  // an earlier item of this call fills the set already
            for (const ApkSlots::Fresh& f : as.fresh) mine = mine || f.key == k;
            if (mine) continue;
            bool noted = false;
            const uint32_t r = R.miss(k, &noted);
            if (noted) acount[2]++;
            if (r != nwv::BlsApkRing::NONE) as.fresh.push_back({r, (uint32_t)i, std::move(k)});
        }
        if (acount[0]) {
            a_off.assign(pk_off, pk_off + n);
            a_cnt.assign(pk_cnt, pk_cnt + n);
            a_idx = remap;
            for (size_t i = 0; i < n; i++) {
                if (hit[i] == nwv::BlsApkRing::NONE) continue;
                a_off[i] = (uint32_t)a_idx.size();
                a_cnt[i] = 1;
                a_idx.push_back(AR_BASE + hit[i]);
            }
        }
        for (const ApkSlots::Fresh& f : as.fresh) a_fill.push_back(f.item);
        for (const ApkSlots::Fresh& f : as.fresh) a_fill.push_back(f.slot);
    }
    const size_t n_fill = as.fresh.size();
    const bool a_hit = !a_idx.empty();
    const uint32_t* k_off = a_hit ? a_off.data() : pk_off;
    const uint32_t* k_cnt = a_hit ? a_cnt.data() : pk_cnt;
    const std::vector<uint32_t>& k_idx = a_hit ? a_idx : remap;
    const size_t nk_idx = k_idx.size();
    uint8_t seed[32];
    nwv_internal_fill_seed(nullptr, seed);  // the batch coefficients' key: OS entropy per call
    Arena a;
    const size_t o_keys = a.add(n_dec ? (const void*)fill_keys.data() : zero, 96 * n_dec + 8),
                 o_kslot = a.add(n_dec ? (const void*)fill_slot.data() : zero, 4 * n_dec + 4),
                 o_sigs = a.add(sigs, 48 * n), o_off = a.add(k_off, 4 * n), o_cnt = a.add(k_cnt, 4 * n),
                 o_idx = a.add(nk_idx ? (const void*)k_idx.data() : zero, 4 * nk_idx + 4),
                 o_msg = a.add(msg_bytes ? (const void*)msg_base : zero, msg_bytes + 1),
                 o_moff = a.add(msg_off, 8 * n), o_mlen = a.add(msg_len, 4 * n), o_dst = a.add(dst, dl),
                 o_seed = a.add(seed, 32), o_kmode = a.add(kside ? (const void*)kmode.data() : zero, 4 * kmode.size() + 4),
                 o_scs = a.add(keep ? (const void*)kept.slots.data() : zero, 4 * kept.slots.size() + 4);
    // (one section for everything the ring adds: a single verification still fits stage_h2d's arguments)
    const size_t o_ring = use_ring ? a.add(rsec.data(), rsec.size()) : 0;
    const size_t o_fill = n_fill ? a.add(a_fill.data(), 8 * n_fill) : 0;
    const size_t o_dlist = n_dn ? a.add(ads.dense.data(), 4 * n_dn) : 0,
                 o_rlist = n_dn && n_rest ? a.add(ads.rest.data(), 4 * n_rest) : 0,
                 o_idx0 = n_dn ? a.add(pk_idx, 4 * n_idx) : 0, o_ktab = n_dn ? a.add(ktab.data(), 4 * n_keys) : 0;
    // (pinned, behind the arena: the batch verdict word, the wave batch check's group verdicts, the
    // dense key sums' per-item modes)
    const size_t h_dmode = al256(al256(a.total) + 64 + 4 * wb_ng);
    if ((rc = L.stage.ensure(h_dmode + 4 * n_dn)) || (rc = L.in.ensure(a.total))) return rc;
    uint8_t* h = static_cast<uint8_t*>(L.stage.p);
    for (size_t k = 0; k < a.parts.size(); k++)
        if (a.parts[k].second) std::memcpy(h + a.offs[k], a.parts[k].first, a.parts[k].second);
    // scratch: the call's key records + statuses, item sig / H / apk records, three status arrays,
    // the batch check's shares (W-order Fp12 + Jacobian G1 per item) and its verdict word
    const size_t w_krec = 0, w_kst = w_krec + 4 * G2_REC_WORDS * n_dec, w_srec = al256(w_kst + 4 * n_dec + 4),
                 w_hrec = w_srec + 4 * G1_REC_WORDS * n, w_arec = w_hrec + 4 * G1_REC_WORDS * n,
                 w_st = w_arec + 4 * G2_REC_WORDS * (n + 1), w_ssig = al256(w_st + 4 * n), w_sapk = al256(w_ssig + 4 * n),
                 w_ok = al256(w_sapk + 4 * n), w_frec = al256(w_ok + 4),
                 w_jrec = al256(w_frec + 4 * F12_REC_WORDS * (batch ? n + 1 : 0)),
                 w_prec = al256(w_jrec + 4 * G1J_REC_WORDS * (batch ? n : 0)),
                 w_hh = al256(w_prec + 4 * G1J_REC_WORDS * (batch ? n + 1 : 0) + 4),
                 w_sdec = al256(w_hh + 4 * G1H_REC_WORDS * (wavem ? n : 0)), w_ssub = al256(w_sdec + 4 * n),
                 w_spair = al256(w_ssub + 4 * n), w_aj = al256(w_spair + 4 * n + 4),
                 w_wb = al256(w_aj + 4 * G2J_WORDS * (wavem ? n + wb_ng : 0) + 4),
                 // the wave batch check's scratch: F records, [r] H, [r] sig, the groups' S_g, in-batch
                 // flags, the groups' verdict words
                 w_wf = w_wb, w_wp = al256(w_wf + 4 * FB_REC_WORDS * wb_m), w_wj = al256(w_wp + 4 * G1H_REC_WORDS * wb_m),
                 w_wsg = al256(w_wj + 4 * G1J_REC_WORDS * (wbatch ? n : 0)),
                 w_winb = al256(w_wsg + 4 * G1_REC_WORDS * wb_ng), w_wgok = al256(w_winb + 4 * (wbatch ? n : 0)),
                 // the dense key sums' scratch: the key table's total and flag, the items' modes
                 w_dtot = al256(w_wgok + 4 * wb_ng + 4), w_dmode = al256(w_dtot + 4 * (n_dn ? DT_WORDS : 0)),
                 w_end = w_dmode + 4 * n_dn + 4;
    if ((rc = L.work.ensure(w_end))) return rc;
    uint8_t* in = static_cast<uint8_t*>(L.in.p);
    uint8_t* w = static_cast<uint8_t*>(L.work.p);
    KeyTab kt{cached ? static_cast<const uint32_t*>(d.kc.rec.p) : nullptr,
              cached ? static_cast<const int32_t*>(d.kc.st.p) : nullptr, reinterpret_cast<uint32_t*>(w + w_krec),
              reinterpret_cast<int32_t*>(w + w_kst),
              cached && d.kc.lines_slots ? static_cast<const uint32_t*>(d.kc.lines.p) : nullptr,
              cached ? static_cast<const uint32_t*>(d.kc.hrec.p) : nullptr,
              use_apk ? static_cast<const uint32_t*>(d.ar.rec.p) : nullptr,
              use_apk ? static_cast<const uint32_t*>(d.ar.lines.p) : nullptr};
    const uint32_t* km = kside ? reinterpret_cast<const uint32_t*>(in + o_kmode) : nullptr;
    auto* srec = reinterpret_cast<uint32_t*>(w + w_srec);
    auto* hrec = reinterpret_cast<uint32_t*>(w + w_hrec);
    auto* arec = reinterpret_cast<uint32_t*>(w + w_arec);
    auto* st = reinterpret_cast<int32_t*>(w + w_st);
    auto* ssig = reinterpret_cast<int32_t*>(w + w_ssig);
    auto* sapk = reinterpret_cast<int32_t*>(w + w_sapk);
    auto* okw = reinterpret_cast<int32_t*>(w + w_ok);
    auto* frec = reinterpret_cast<uint32_t*>(w + w_frec);
    auto* jrec = reinterpret_cast<uint32_t*>(w + w_jrec);
    auto* prec = reinterpret_cast<uint32_t*>(w + w_prec);
    auto* hh = reinterpret_cast<uint32_t*>(w + w_hh);
    auto* sdec = reinterpret_cast<int32_t*>(w + w_sdec);
    auto* ssub = reinterpret_cast<int32_t*>(w + w_ssub);
    auto* spair = reinterpret_cast<int32_t*>(w + w_spair);
    auto* ajrec = reinterpret_cast<uint32_t*>(w + w_aj);
    hipStream_t s0 = L.stream, s1 = L.side[0], s2 = L.side[1];
    kept.stream = s0;
    // the per-stage timing events of a small call only on a NWV_FLAG_BLS_STAGE_TIMES context: else
    // just the two that order the streams (the others cost a single verification ~0.1 ms:
    // 2.85 -> 2.72-2.81 ms, profiles/round6_bls_stage_timing_ab.json)
    const bool no_timing = !(d.flags & NWV_FLAG_BLS_STAGE_TIMES);
    bool untimed = false;  // a small call that recorded no stage events (set on that path only)
    auto trec = [&](int k, hipStream_t s) { return no_timing ? hipSuccess : hipEventRecord(L.ev[k], s); };
    // stage times of the completed call, its path and key counts -> the device's "last call"
    uint64_t wb_stat[3] = {0, 0, 0}, kb_stat[5] = {0, 0, 0, 0, 0}, ad_stat[4] = {0, 0, 0, 0};
    auto finish = [&](int path_done) -> int {
        const int pairs[5][2] = {{0, 1}, {3, 4}, {5, 6}, {1, 2}, {7, 8}};  // keys, sigs, h2c, apk, pairing
        double ms5[5] = {0, 0, 0, 0, 0};
        for (int k = 0; k < 5 && !untimed; k++) {
            float ms = 0;
            BLS_HIP(hipEventElapsedTime(&ms, L.ev[pairs[k][0]], L.ev[pairs[k][1]]));
            ms5[k] = ms;
        }
        std::lock_guard<std::mutex> g(d.stat_mu);
        std::memcpy(d.last_ms, ms5, sizeof ms5);
        d.last_path = path_done;
        d.last_keys[0] = hits;
        d.last_keys[1] = n_dec;
        std::memcpy(d.last_batch, wb_stat, sizeof wb_stat);
        std::memcpy(d.last_kbatch, kb_stat, sizeof kb_stat);
        std::memcpy(d.last_apkd, ad_stat, sizeof ad_stat);
        return NWV_OK;
    };
    BLS_HIP(nwv_stage::stage_h2d(in, h, a.total, s0));  // small calls: through kernel arguments
    BLS_HIP(hipEventRecord(L.sev[0], s0));
    BLS_HIP(hipStreamWaitEvent(s1, L.sev[0], 0));
    if (wave_small) {
        untimed = no_timing;
        // a call of up to wave_max items on two streams (8 concurrent calls then fit 16 hardware
        // queues one to one): side 0 decodes the keys the cache does not hold, then hashes to G1
        // and sums the keys in one launch (k_blsw_pre); main decodes the signatures, then runs
        // the pairing checks and the signatures' G1 checks in one launch (k_blsw_pair_sub)
        BLS_HIP(trec(0, s1));
        if (n_dec)
            hipLaunchKernelGGL(k_bls_keys_fill, dim3(kBlocks(n_dec)), dim3(BLS_LANES), 0, s1, (uint32_t)n_dec,
                               in + o_keys, reinterpret_cast<const uint32_t*>(in + o_kslot),
                               const_cast<uint32_t*>(kt.rs), const_cast<int32_t*>(kt.ss));
        BLS_HIP(trec(1, s1));
        BLS_HIP(trec(5, s1));
        if (use_ring)
            hipLaunchKernelGGL(k_blsw_pre_r, dim3((unsigned)(2 * n)), dim3(64), 0, s1, (uint32_t)n, in + o_msg,
                               reinterpret_cast<const uint64_t*>(in + o_moff),
                               reinterpret_cast<const uint32_t*>(in + o_mlen), in + o_dst, (uint32_t)dl, hh, kt,
                               reinterpret_cast<const uint32_t*>(in + o_off),
                               reinterpret_cast<const uint32_t*>(in + o_cnt),
                               reinterpret_cast<const uint32_t*>(in + o_idx), km, ajrec, sapk,
                               static_cast<uint32_t*>(d.mr.rec.p),
                               reinterpret_cast<const uint32_t*>(in + o_ring + r_hsrc),
                               reinterpret_cast<const uint32_t*>(in + o_ring + r_hpub));
        else
            hipLaunchKernelGGL(k_blsw_pre, dim3((unsigned)(2 * n)), dim3(64), 0, s1, (uint32_t)n, in + o_msg,
                               reinterpret_cast<const uint64_t*>(in + o_moff),
                               reinterpret_cast<const uint32_t*>(in + o_mlen), in + o_dst, (uint32_t)dl, hh, kt,
                               reinterpret_cast<const uint32_t*>(in + o_off),
                               reinterpret_cast<const uint32_t*>(in + o_cnt),
                               reinterpret_cast<const uint32_t*>(in + o_idx), km, ajrec, sapk);
        if (n_fill) BLS_HIP(hipEventRecord(L.sev[2], s1));
        BLS_HIP(trec(2, s1));
        BLS_HIP(trec(6, s1));
        BLS_HIP(trec(3, s0));
        hipLaunchKernelGGL(k_blsw_sigdec, dim3(kBlocks(n)), dim3(BLS_LANES), 0, s0, (uint32_t)n, in + o_sigs, srec,
                           sdec);
        BLS_HIP(trec(4, s0));
        BLS_HIP(hipEventRecord(L.sev[1], s0));
        // the ahead messages on the main stream, idle from here on: the pairing, on side 0, does
        // not wait for them
        if (n_ah)
            hipLaunchKernelGGL(k_blsw_h2c_ahead, dim3((unsigned)n_ah), dim3(64), 0, s0, (uint32_t)n_ah,
                               (const uint8_t*)(in + o_ring + r_amsg), reinterpret_cast<const uint64_t*>(in + o_ring),
                               reinterpret_cast<const uint32_t*>(in + o_ring + r_alen), (const uint8_t*)(in + o_dst),
                               (uint32_t)dl, static_cast<uint32_t*>(d.mr.rec.p),
                               reinterpret_cast<const uint32_t*>(in + o_ring + r_aslot));
        // the aggregate-key fills on the main stream too, behind the key sums: they run beside the
        // pairing kernel, which reads the sums and never the slots being filled
        if (n_fill) {
            BLS_HIP(hipStreamWaitEvent(s0, L.sev[2], 0));
            hipLaunchKernelGGL(k_blsw_apk_fill, dim3((unsigned)n_fill), dim3(64), 0, s0, (uint32_t)n_fill,
                               reinterpret_cast<const uint32_t*>(in + o_fill),
                               reinterpret_cast<const uint32_t*>(in + o_fill + 4 * n_fill), (const uint32_t*)ajrec,
                               (const int32_t*)sapk, static_cast<uint32_t*>(d.ar.rec.p),
                               static_cast<uint32_t*>(d.ar.lines.p));
        }
        kept.stream = s1;  // k_blsw_status writes the ring slots there
        // the rest runs on side 0 behind the hash, which ends after the signatures' decode (one
        // lane each, ~0.45 ms against ~0.57 ms): its wait on the decode is already met, so the
        // cross-queue hand-off (~25 us in the single-verify trace) is off the critical path
        BLS_HIP(hipStreamWaitEvent(s1, L.sev[1], 0));
        BLS_HIP(trec(7, s1));
        static const bool sub_flat = [] {
            const char* e = std::getenv("NWV_BLS_SUB_FLAT");
            return e && std::atoi(e) != 0;
        }();
        if (sub_flat && ensure_pair_script()) return NWV_ERR_HIP;
        hipLaunchKernelGGL(sub_flat ? k_blsw_pair_sub_f : k_blsw_pair_sub, dim3((unsigned)(2 * n)), dim3(64), 0, s1,
                           (uint32_t)n,
                           (const uint32_t*)srec, (const int32_t*)sdec, (const uint32_t*)hh, 1, (const uint32_t*)ajrec,
                           (const int32_t*)sapk, kt, reinterpret_cast<const uint32_t*>(in + o_off),
                           reinterpret_cast<const uint32_t*>(in + o_cnt), reinterpret_cast<const uint32_t*>(in + o_idx),
                           km, spair, ssub);
        BLS_HIP(trec(8, s1));
        // (the verified records into the ring slots this call reserved)
        hipLaunchKernelGGL(k_blsw_status, dim3(kBlocks(n)), dim3(BLS_LANES), 0, s1, (uint32_t)n,
                           (const int32_t*)sdec, (const int32_t*)ssub, (const int32_t*)sapk, (const int32_t*)spair, st,
                           (const uint32_t*)srec, keep ? static_cast<uint32_t*>(d.sc.rec.p) : nullptr,
                           reinterpret_cast<const uint32_t*>(in + o_scs));
        BLS_HIP(hipGetLastError());
        BLS_HIP(hipMemcpyAsync(status, st, 4 * n, hipMemcpyDeviceToHost, s1));
        BLS_HIP(hipStreamSynchronize(s1));
        if (n_ah || n_fill) BLS_HIP(hipStreamSynchronize(s0));
        if (keep) {
            d.sc.publish(n, sigs, status, kept.slots);
            kept.sc = nullptr;
        }
        // H(m) is a function of dst and message alone: a miss is published whatever its item's
        // status; an ahead message only behind its gate
        ms.finish(status, mcount);
        if (mstat)
            for (int k = 0; k < 5; k++) mstat[k] += mcount[k];
        // a set is a function of the key cache's slots alone, but it is kept only behind a verified
        // aggregate: peers cannot churn the ring without valid certificates
        as.finish(status, acount);
        if (astat)
            for (int k = 0; k < 4; k++) astat[k] += acount[k];
        return finish(3);
    }
    if (!L.side[1] && nwv::lane_stream_create(&L.side[1], L.high) != hipSuccess)
        return nwv_internal_set_err(NWV_ERR_HIP, "bls stream");
    s2 = L.side[1];
    BLS_HIP(hipStreamWaitEvent(s2, L.sev[0], 0));
    // side 0: keys, key sums
    BLS_HIP(hipEventRecord(L.ev[0], s1));
    if (n_dec)
        hipLaunchKernelGGL(k_bls_keys_fill, dim3(kBlocks(n_dec)), dim3(BLS_LANES), 0, s1, (uint32_t)n_dec, in + o_keys,
                           reinterpret_cast<const uint32_t*>(in + o_kslot), const_cast<uint32_t*>(kt.rs),
                           const_cast<int32_t*>(kt.ss));
    BLS_HIP(hipEventRecord(L.ev[1], s1));
    auto* dtot = reinterpret_cast<uint32_t*>(w + w_dtot);
    auto* dmode = reinterpret_cast<uint32_t*>(w + w_dmode);
    if (wavem && n_dn) {
        // the dense stage: the key table's total, the dense items L lanes each, then the items
        // left to the per-item code through their list (all three write disjoint records)
        const DenseKeys dk{kt.hrc, kt.sc, reinterpret_cast<const uint32_t*>(in + o_ktab), (uint32_t)n_keys, KC_CAP};
        const auto* d_list = reinterpret_cast<const uint32_t*>(in + o_dlist);
        const auto* p_off = reinterpret_cast<const uint32_t*>(in + o_off);
        const auto* p_cnt = reinterpret_cast<const uint32_t*>(in + o_cnt);
        const auto* p_idx0 = reinterpret_cast<const uint32_t*>(in + o_idx0);
        hipLaunchKernelGGL(k_blsd_total, dim3(1), dim3(64), 0, s1, dk, dtot);
        const unsigned per = 64 / ad_lanes, blocks = (unsigned)((n_dn + per - 1) / per);
        auto* kern = ad_lanes == 16 ? k_blsd_apk<16> : ad_lanes == 8 ? k_blsd_apk<8> : k_blsd_apk<4>;
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), 0, s1, (uint32_t)n_dn, d_list, dk, p_off, p_cnt, p_idx0,
                           (const uint32_t*)dtot, ajrec, sapk, dmode);
        if (n_rest)
            hipLaunchKernelGGL(k_blsw_apk_list, dim3((unsigned)n_rest), dim3(64), 0, s1, (uint32_t)n_rest,
                               reinterpret_cast<const uint32_t*>(in + o_rlist), kt, p_off, p_cnt,
                               reinterpret_cast<const uint32_t*>(in + o_idx), km, ajrec, sapk);
    } else if (wavem)
        hipLaunchKernelGGL(k_blsw_apk, dim3((unsigned)n), dim3(64), 0, s1, (uint32_t)n, kt,
                           reinterpret_cast<const uint32_t*>(in + o_off), reinterpret_cast<const uint32_t*>(in + o_cnt),
                           reinterpret_cast<const uint32_t*>(in + o_idx), km, ajrec, sapk);
    else
        hipLaunchKernelGGL(k_bls_apk_g, dim3(gBlocks(n)), dim3(BLS_LANES), 0, s1, (uint32_t)n, kt,
                           reinterpret_cast<const uint32_t*>(in + o_off), reinterpret_cast<const uint32_t*>(in + o_cnt),
                           reinterpret_cast<const uint32_t*>(in + o_idx), arec, sapk);
    BLS_HIP(hipEventRecord(L.ev[2], s1));
    BLS_HIP(hipEventRecord(L.ev[10], s1));
    // side 1: hash to G1 (every item: the statuses are not known yet)
    BLS_HIP(hipEventRecord(L.ev[5], s2));
    // hash to G1: lane pairs (NWV_BLS_H2C_GROUP=1: the 8-lane group form)
    static const bool h2c_group = [] {
        const char* e = std::getenv("NWV_BLS_H2C_GROUP");
        return e && std::atoi(e) != 0;
    }();
    if (!h2c_group)
        hipLaunchKernelGGL(k_bls_h2c_2, dim3((unsigned)((n + BLS_LANES / 2 - 1) / (BLS_LANES / 2))), dim3(BLS_LANES), 0,
                           s2, (uint32_t)n, in + o_msg, reinterpret_cast<const uint64_t*>(in + o_moff),
                           reinterpret_cast<const uint32_t*>(in + o_mlen), in + o_dst, (uint32_t)dl, hrec, km);
    else
    hipLaunchKernelGGL(k_bls_h2c_g, dim3(gBlocks(n)), dim3(BLS_LANES), 0, s2, (uint32_t)n, in + o_msg,
                       reinterpret_cast<const uint64_t*>(in + o_moff), reinterpret_cast<const uint32_t*>(in + o_mlen),
                       in + o_dst, (uint32_t)dl, hrec, km);
    BLS_HIP(hipEventRecord(L.ev[6], s2));
    BLS_HIP(hipEventRecord(L.ev[11], s2));
    if (wavem) {
        // large wave calls: the one-lane-per-item decode + G1 check of the group path, which keeps
        // every lane busy (an all-Ok subgroup column), then every item's pairing check on a wave
        BLS_HIP(hipEventRecord(L.ev[3], s0));
        hipLaunchKernelGGL(k_bls_sigs, dim3(kBlocks(n)), dim3(BLS_LANES), 0, s0, (uint32_t)n, in + o_sigs, srec, sdec);
        BLS_HIP(hipMemsetAsync(ssub, 0, 4 * n, s0));
        BLS_HIP(hipEventRecord(L.ev[4], s0));
        BLS_HIP(hipStreamWaitEvent(s0, L.ev[10], 0));
        BLS_HIP(hipStreamWaitEvent(s0, L.ev[11], 0));
        BLS_HIP(hipEventRecord(L.ev[7], s0));
        // items per pairing wave (env NWV_BLS_PACK, 1..4): one LDS bank of ~6.5 KB each
        static const uint32_t pack = [] {
            const char* e = std::getenv("NWV_BLS_PACK");
            const long v = e ? std::strtol(e, nullptr, 10) : 3;
            return (uint32_t)(v < 1 ? 1 : v > BLS_PACK_MAX ? BLS_PACK_MAX : v);
        }();
        // diagnostic (occupancy experiments): NWV_BLS_LDS_PAD bytes of extra LDS per pairing wave
        static const size_t lds_pad = [] {
            const char* e = std::getenv("NWV_BLS_LDS_PAD");
            return e ? (size_t)std::strtoull(e, nullptr, 10) : (size_t)0;
        }();
        // (every item's keys cached is what the key side already asks: kside)
        const bool kb_cand = !wave_small && kside && kb_min > 0 && n >= kb_min;
        if ((pack > 1 || wbatch || kb_cand) && ensure_pair_script()) return NWV_ERR_HIP;
        const auto* d_off = reinterpret_cast<const uint32_t*>(in + o_off);
        const auto* d_cnt = reinterpret_cast<const uint32_t*>(in + o_cnt);
        const auto* d_idx = reinterpret_cast<const uint32_t*>(in + o_idx);
        // the per-item pairing checks of items [lo, lo + m): every item's own final exponentiation
        auto per_item_range = [&](size_t lo, size_t m) {
            if (pack > 1)
                hipLaunchKernelGGL(k_blsw_pair_k, dim3((unsigned)((m + pack - 1) / pack)), dim3(64),
                                   (size_t)4 * (wave::KP_WORDS + pack * wave::SW * wave::NSLOTS_PC) + lds_pad, s0,
                                   (uint32_t)m, pack, (const uint32_t*)srec + G1_REC_WORDS * lo,
                                   (const int32_t*)sdec + lo, (const uint32_t*)hrec + G1_REC_WORDS * lo, 0,
                                   (const uint32_t*)ajrec + G2J_WORDS * lo, (const int32_t*)sapk + lo, kt, d_off + lo,
                                   d_cnt + lo, d_idx, km ? km + lo : nullptr, spair + lo);
            else
                hipLaunchKernelGGL(k_blsw_pair, dim3((unsigned)m), dim3(64), lds_pad, s0, (uint32_t)m,
                                   (const uint32_t*)srec + G1_REC_WORDS * lo, (const int32_t*)sdec + lo,
                                   (const uint32_t*)hrec + G1_REC_WORDS * lo, 0, (const uint32_t*)ajrec + G2J_WORDS * lo,
                                   (const int32_t*)sapk + lo, kt, d_off + lo, d_cnt + lo, d_idx,
                                   km ? km + lo : nullptr, spair + lo);
        };
        int path_done = 3;
        bool kb_done = false;
        if (kb_cand) {
            // the pre-pairing statuses come back first: the plan groups the items they leave
            if ((rc = L.kb_st.ensure(12 * n + 64))) return rc;
            int32_t* h_dec = static_cast<int32_t*>(L.kb_st.p);
            int32_t *h_apk = h_dec + n, *h_gok = h_apk + n;
            BLS_HIP(hipMemcpyAsync(h_dec, sdec, 4 * n, hipMemcpyDeviceToHost, s0));
            BLS_HIP(hipMemcpyAsync(h_apk, sapk, 4 * n, hipMemcpyDeviceToHost, s0));
            BLS_HIP(hipStreamSynchronize(s0));
            std::vector<uint8_t> ok(n), el(n);
            for (size_t i = 0; i < n; i++) {
                ok[i] = h_dec[i] == ST_OK && h_apk[i] == ST_OK;
                // (a compressed identity has bit 6 of its first byte set; the kernels check again)
                el[i] = ok[i] && kmode[i] && !(sigs[48 * i] & 0x40);
            }
            nwv::KeyBatchPlan P;
            nwv::key_batch_plan(n, ok.data(), el.data(), pk_off, pk_cnt, remap.data(), d.kc.used, kb_grp, kb_ratio, P);
            if (P.run) {
                const size_t ne = P.items.size(), ng = P.groups(), M = P.entries(), C = P.cidx.size(), KM = M + ng;
                // the plan's lists, one copy: items | goff | eslot | egrp | coff | cidx | 0..M-1 | ones
                const size_t u_goff = ne, u_eslot = u_goff + ng + 1, u_egrp = u_eslot + M, u_coff = u_egrp + M,
                             u_cidx = u_coff + M + 1, u_iota = u_cidx + C, u_ones = u_iota + M, u_end = u_ones + M;
                if ((rc = L.kb_up.ensure(4 * u_end)) || (rc = L.kb_in.ensure(4 * u_end))) return rc;
                uint32_t* up = static_cast<uint32_t*>(L.kb_up.p);
                std::memcpy(up, P.items.data(), 4 * ne);
                std::memcpy(up + u_goff, P.goff.data(), 4 * (ng + 1));
                std::memcpy(up + u_eslot, P.eslot.data(), 4 * M);
                std::memcpy(up + u_egrp, P.egrp.data(), 4 * M);
                std::memcpy(up + u_coff, P.coff.data(), 4 * (M + 1));
                std::memcpy(up + u_cidx, P.cidx.data(), 4 * C);
                for (size_t m = 0; m < M; m++) {
                    up[u_iota + m] = (uint32_t)m;
                    up[u_ones + m] = 1u;
                }
                const uint32_t* ki = static_cast<const uint32_t*>(L.kb_in.p);
                BLS_HIP(hipMemcpyAsync(L.kb_in.p, up, 4 * u_end, hipMemcpyHostToDevice, s0));
                // the check's records: [r] H and [r] sig per position, S_g per group, the Miller
                // entries' hash sides, Qs and F records, the groups' poison and verdict words
                const size_t k_sj = al256(4 * G1J_REC_WORDS * ne), k_sg = al256(k_sj + 4 * G1J_REC_WORDS * ne),
                             k_p = al256(k_sg + 4 * G1_REC_WORDS * ng), k_q = al256(k_p + 4 * G1H_REC_WORDS * KM),
                             k_f = al256(k_q + 4 * G2J_WORDS * KM), k_poi = al256(k_f + 4 * FB_REC_WORDS * KM),
                             k_gok = k_poi + 4 * ng, k_end = k_gok + 4 * ng + 4;
                if ((rc = L.kb_work.ensure(k_end))) return rc;
                uint8_t* kw = static_cast<uint8_t*>(L.kb_work.p);
                auto* khj = reinterpret_cast<uint32_t*>(kw);
                auto* ksj = reinterpret_cast<uint32_t*>(kw + k_sj);
                auto* ksg = reinterpret_cast<uint32_t*>(kw + k_sg);
                auto* kp = reinterpret_cast<uint32_t*>(kw + k_p);
                auto* kq = reinterpret_cast<uint32_t*>(kw + k_q);
                auto* kf = reinterpret_cast<uint32_t*>(kw + k_f);
                auto* kpoi = reinterpret_cast<uint32_t*>(kw + k_poi);
                auto* kgok = reinterpret_cast<int32_t*>(kw + k_gok);
                const uint32_t G = kb_grp, gmax = (uint32_t)std::min<size_t>(G, ne);
                uint32_t kmax = 0;
                for (size_t g = 0; g < ng; g++) kmax = std::max(kmax, P.goff[g + 1] - P.goff[g]);
                BLS_HIP(hipMemsetAsync(kpoi, 0, 8 * ng, s0));  // no poison; a group whose tree does not finish stays rejected
                hipLaunchKernelGGL(k_blsk_rlc_pts, dim3(kBlocks(2 * ne)), dim3(BLS_LANES), 0, s0, (uint32_t)ne, G, ki,
                                   (const uint32_t*)srec, (const uint32_t*)hrec, (const int32_t*)sdec,
                                   (const int32_t*)sapk, (const uint8_t*)(in + o_seed), khj, ksj, kpoi);
                for (uint32_t m = gmax; m > 1; m = (m + 1) / 2)
                    hipLaunchKernelGGL(k_blsw_sfold, dim3(kBlocks(ng * ((m + 1) / 2))), dim3(BLS_LANES), 0, s0,
                                       (uint32_t)ne, G, (uint32_t)ng, m, ksj);
                hipLaunchKernelGGL(k_blsk_key_sums, dim3((unsigned)M), dim3(64), 0, s0, (uint32_t)M, ki + u_coff,
                                   ki + u_cidx, ki + u_eslot, ki + u_egrp, (const uint32_t*)khj, kt, kp, kq, kpoi);
                hipLaunchKernelGGL(k_blsk_sig_items, dim3(kBlocks(ng)), dim3(BLS_LANES), 0, s0, (uint32_t)ng, G,
                                   (uint32_t)M, (const uint32_t*)ksj, ksg, kp, kq);
                // every key entry as a one-key key-side item of its own: key list entry m = slot eslot[m]
                const MillArgs ma{(uint32_t)M, ksg, ki + u_ones, kf};
                hipLaunchKernelGGL(k_blsw_mill_k, dim3((unsigned)((KM + pack - 1) / pack)), dim3(64),
                                   (size_t)4 * (wave::KP_WORDS + pack * wave::SW * wave::NSLOTS_PC) + lds_pad, s0,
                                   (uint32_t)KM, pack, ma, (const uint32_t*)kp, (const uint32_t*)kq, kt, ki + u_iota,
                                   ki + u_ones, ki + u_eslot, ki + u_ones);
                for (uint32_t s = 1;; s *= WB_FAN) {
                    const uint32_t ents = (kmax + 1 + s - 1) / s, wpg = (ents + WB_FAN - 1) / WB_FAN;
                    hipLaunchKernelGGL(k_blsk_ffold, dim3((unsigned)(ng * wpg)), dim3(64), 0, s0, (uint32_t)ng,
                                       ki + u_goff, (uint32_t)M, wpg, s, wpg == 1 ? 1 : 0, kf, (const uint32_t*)kpoi, kgok);
                    if (wpg == 1) break;
                }
                hipLaunchKernelGGL(k_blsk_mark, dim3(kBlocks(ne)), dim3(BLS_LANES), 0, s0, (uint32_t)ne, G, ki,
                                   (const int32_t*)kgok, spair);
                BLS_HIP(hipGetLastError());
                BLS_HIP(hipMemcpyAsync(h_gok, kgok, 4 * ng, hipMemcpyDeviceToHost, s0));
                BLS_HIP(hipStreamSynchronize(s0));
                // per item: the OK items outside the groups and every rejected group's items, in
                // shared launches as the wave batch check shares them
                std::vector<uint8_t> need(n, 0), ing(n, 0);
                for (uint32_t i : P.outside) need[i] = 1;
                for (uint32_t i : P.items) ing[i] = 1;
                for (size_t g = 0; g < ng; g++) {
                    if (h_gok[g] == 1) continue;
                    kb_stat[1]++;
                    for (uint32_t p = P.gfirst[g]; p < P.gfirst[g + 1]; p++) need[P.items[p]] = 1;
                }
                for (const auto& r : nwv::key_batch_ranges(n, need.data(), 1024)) {
                    per_item_range(r.first, r.second - r.first);
                    for (size_t i = r.first; i < r.second; i++) kb_stat[2] += ing[i];
                }
                kb_stat[0] = ng;
                kb_stat[3] = KM;
                kb_stat[4] = ne;
                path_done = kb_stat[1] ? 7 : 6;
                kb_done = true;
            }
        }
        if (!kb_done && wbatch) {
            auto* wf = reinterpret_cast<uint32_t*>(w + w_wf);
            auto* wp = reinterpret_cast<uint32_t*>(w + w_wp);
            auto* wj = reinterpret_cast<uint32_t*>(w + w_wj);
            auto* wsg = reinterpret_cast<uint32_t*>(w + w_wsg);
            auto* winb = reinterpret_cast<uint32_t*>(w + w_winb);
            auto* wgok = reinterpret_cast<int32_t*>(w + w_wgok);
            const uint32_t G = (uint32_t)wb_grp, ng = (uint32_t)wb_ng, gmax = (uint32_t)std::min<size_t>(wb_grp, n);
            BLS_HIP(hipMemsetAsync(wgok, 0, 4 * wb_ng, s0));  // a group whose tree does not finish stays rejected
            hipLaunchKernelGGL(k_blsw_rlc_pts, dim3(kBlocks(2 * n)), dim3(BLS_LANES), 0, s0, (uint32_t)n,
                               (const uint32_t*)srec, (const uint32_t*)hrec, (const int32_t*)sdec, (const int32_t*)sapk, km,
                               (const uint8_t*)(in + o_seed), wp, wj, winb, spair);
            for (uint32_t m = gmax; m > 1; m = (m + 1) / 2)
                hipLaunchKernelGGL(k_blsw_sfold, dim3(kBlocks((size_t)ng * ((m + 1) / 2))), dim3(BLS_LANES), 0, s0,
                                   (uint32_t)n, G, ng, m, wj);
            hipLaunchKernelGGL(k_blsw_sig_items, dim3(kBlocks(ng)), dim3(BLS_LANES), 0, s0, (uint32_t)n, G, ng,
                               (const uint32_t*)wj, wsg, wp, ajrec);
            const MillArgs ma{(uint32_t)n, wsg, winb, wf};
            hipLaunchKernelGGL(k_blsw_mill_k, dim3((unsigned)((wb_m + pack - 1) / pack)), dim3(64),
                               (size_t)4 * (wave::KP_WORDS + pack * wave::SW * wave::NSLOTS_PC) + lds_pad, s0,
                               (uint32_t)wb_m, pack, ma, (const uint32_t*)wp, (const uint32_t*)ajrec, kt, d_off, d_cnt,
                               d_idx, km);
            for (uint32_t s = 1;; s *= WB_FAN) {
                const uint32_t ents = (gmax + 1 + s - 1) / s, wpg = (ents + WB_FAN - 1) / WB_FAN;
                hipLaunchKernelGGL(k_blsw_ffold, dim3(ng * wpg), dim3(64), 0, s0, (uint32_t)n, G, wpg, s,
                                   wpg == 1 ? 1 : 0, wf, wgok);
                if (wpg == 1) break;
            }
            hipLaunchKernelGGL(k_blsw_mark, dim3(kBlocks(n)), dim3(BLS_LANES), 0, s0, (uint32_t)n, G,
                               (const int32_t*)wgok, (const uint32_t*)winb, spair);
            BLS_HIP(hipGetLastError());
            int32_t* hgok = reinterpret_cast<int32_t*>(h + al256(a.total) + 64);  // pinned: the groups' verdicts
            BLS_HIP(hipMemcpyAsync(hgok, wgok, 4 * wb_ng, hipMemcpyDeviceToHost, s0));
            BLS_HIP(hipStreamSynchronize(s0));
            // every rejected group's items per item.  A launch over a few items costs one item's
            // whole chain (~3 ms) however few they are, so rejected groups less than WB_GAP items
            // apart share a launch with the accepted groups between them (~1 us an item there)
            constexpr size_t WB_GAP = 1024;
            wb_stat[0] = wb_ng;
            for (size_t g = 0; g < wb_ng;) {
                if (hgok[g] == 1) {
                    g++;
                    continue;
                }
                size_t e = g + 1;  // the range's end: past its last rejected group
                wb_stat[1]++;
                for (size_t q = e; q < wb_ng && (q - e) * wb_grp < WB_GAP; q++)
                    if (hgok[q] != 1) {
                        e = q + 1;
                        wb_stat[1]++;
                    }
                const size_t lo = g * wb_grp, hi = std::min(n, e * wb_grp);
                per_item_range(lo, hi - lo);
                wb_stat[2] += hi - lo;
                g = e;
            }
            path_done = wb_stat[1] ? 5 : 4;
        } else if (!kb_done) {
            per_item_range(0, n);
        }
        BLS_HIP(hipEventRecord(L.ev[8], s0));
        hipLaunchKernelGGL(k_blsw_status, dim3(kBlocks(n)), dim3(BLS_LANES), 0, s0, (uint32_t)n,
                           (const int32_t*)sdec, (const int32_t*)ssub, (const int32_t*)sapk, (const int32_t*)spair, st,
                           (const uint32_t*)srec, nullptr, nullptr);
        BLS_HIP(hipGetLastError());
        BLS_HIP(hipMemcpyAsync(status, st, 4 * n, hipMemcpyDeviceToHost, s0));
        const uint32_t* h_dm = reinterpret_cast<const uint32_t*>(h + h_dmode);
        if (n_dn) BLS_HIP(hipMemcpyAsync(h + h_dmode, dmode, 4 * n_dn, hipMemcpyDeviceToHost, s0));
        BLS_HIP(hipStreamSynchronize(s0));
        if (ad_run) {
            for (size_t q = 0; q < n_dn; q++) ad_stat[h_dm[q] ? 1 : 0]++;
            ad_stat[2] = n_rest;
            ad_stat[3] = ad_lanes;
        }
        return finish(path_done);
    }
    // main: signatures, then the join
    BLS_HIP(hipEventRecord(L.ev[3], s0));
    hipLaunchKernelGGL(k_bls_sigs, dim3(kBlocks(n)), dim3(BLS_LANES), 0, s0, (uint32_t)n, in + o_sigs, srec, ssig);
    BLS_HIP(hipEventRecord(L.ev[4], s0));
    BLS_HIP(hipStreamWaitEvent(s0, L.ev[10], 0));
    BLS_HIP(hipStreamWaitEvent(s0, L.ev[11], 0));
    hipLaunchKernelGGL(k_bls_status, dim3(kBlocks(n)), dim3(BLS_LANES), 0, s0, (uint32_t)n, (const int32_t*)ssig,
                       (const int32_t*)sapk, st);
    BLS_HIP(hipEventRecord(L.ev[7], s0));
    auto per_item = [&]() {
        hipLaunchKernelGGL(k_bls_pair, dim3(gBlocks(n)), dim3(BLS_LANES), 0, s0, (uint32_t)n, (const uint32_t*)srec,
                           (const uint32_t*)hrec, (const uint32_t*)arec, st);
    };
    int32_t* hst = reinterpret_cast<int32_t*>(h + al256(a.total));  // pinned: the batch verdict word
    int path;
    if (batch) {
        hipLaunchKernelGGL(k_bls_rlc_pts, dim3(gBlocks(n)), dim3(BLS_LANES), 0, s0, (uint32_t)n, (const uint32_t*)srec,
                           (const uint32_t*)hrec, (const int32_t*)st, (const uint8_t*)(in + o_seed), prec, jrec);
        for (uint32_t m = (uint32_t)n; m > 1; m = (m + 1) / 2)
            hipLaunchKernelGGL(k_bls_sfold, dim3(kBlocks(m / 2)), dim3(BLS_LANES), 0, s0, m, jrec);
        hipLaunchKernelGGL(k_bls_sig_item, dim3(1), dim3(BLS_LANES), 0, s0, (uint32_t)n, (const uint32_t*)jrec, prec,
                           arec);
        hipLaunchKernelGGL(k_bls_rlc_ml, dim3(gBlocks(n + 1)), dim3(BLS_LANES), 0, s0, (uint32_t)(n + 1),
                           (const uint32_t*)prec, (const uint32_t*)arec, frec);
        for (uint32_t m = (uint32_t)n + 1; m > 1; m = (m + 1) / 2)
            hipLaunchKernelGGL(k_bls_ffold, dim3(gBlocks(m / 2)), dim3(BLS_LANES), 0, s0, m, frec);
        hipLaunchKernelGGL(k_bls_final, dim3(1), dim3(BLS_LANES), 0, s0, (const uint32_t*)frec, okw);
        BLS_HIP(hipMemcpyAsync(hst, okw, 4, hipMemcpyDeviceToHost, s0));
        BLS_HIP(hipStreamSynchronize(s0));
        BLS_HIP(hipGetLastError());
        path = *hst == 1 ? 1 : 2;
        if (*hst != 1) per_item();  // the batch check rejected: name the failing items exactly
    } else {
        per_item();
        path = 0;
    }
    BLS_HIP(hipEventRecord(L.ev[8], s0));
    BLS_HIP(hipGetLastError());
    BLS_HIP(hipMemcpyAsync(status, st, 4 * n, hipMemcpyDeviceToHost, s0));
    BLS_HIP(hipStreamSynchronize(s0));
    return finish(path);
}

// nwv_bls_hash_ahead on one device: the messages the ring does not hold, hashed (raw) into reserved
// slots, published once the launch has completed.  `sel` (optional): only messages j with sel[j]
// != 0.  Chunks of at most the ring's size (and 1,024): a chunk's slots are published before the
// next reserves, so a list longer than the ring leaves its LAST messages cached, as a FIFO should.
int msg_ring_fill(BlsDev& d, size_t n, const uint8_t* base, const uint64_t* off, const uint32_t* len,
                  const uint8_t* sel, const uint8_t* dst, size_t dl) {
    if (!d.mr.on.load(std::memory_order_acquire) || dl > nwv::MsgKey::MAX_DST) return NWV_OK;
    nwv::BlsMsgRing& R = d.mr.ring;
    const size_t chunk = std::min<size_t>(R.cap(), 1024);
    LaneLease lane(d);
    if (lane.rc()) return lane.rc();
    BlsLane& L = *lane;
    int rc;
    for (size_t j0 = 0; j0 < n;) {
        MsgSlots ms;
        ms.ring = &R;
        ms.streams[0] = L.stream;
        std::vector<uint32_t> aslot, alen;
        std::vector<uint64_t> aoff;
        std::vector<uint8_t> amsg;
        size_t j = j0;
        for (; j < n && aslot.size() < chunk; j++) {
            if ((sel && !sel[j]) || len[j] > nwv::MsgKey::MAX_MSG) continue;
            const nwv::MsgKey k = nwv::MsgKey::make(dst, dl, base + off[j], len[j]);
            if (R.contains(k)) continue;
            bool dup = false;
            for (const MsgSlots::Fresh& f : ms.fresh) dup = dup || f.key == k;
            if (dup) continue;
            const uint32_t r = R.reserve();
            if (r == nwv::BlsMsgRing::NONE) continue;  // every slot in use by calls in flight
            ms.fresh.push_back({r, k, UINT32_MAX, true});
            aslot.push_back(r);
            alen.push_back(len[j]);
            aoff.push_back(amsg.size());
            amsg.insert(amsg.end(), base + off[j], base + off[j] + len[j]);
        }
        j0 = j;
        const size_t m = aslot.size();
        if (!m) continue;
        const size_t o_slot = 8 * m, o_len = o_slot + 4 * m, o_dst = o_len + 4 * m, o_msg = o_dst + al256(dl + 1),
                     total = o_msg + amsg.size() + 1;
        if ((rc = L.stage.ensure(total)) || (rc = L.in.ensure(total))) return rc;
        uint8_t* h = static_cast<uint8_t*>(L.stage.p);
        uint8_t* in = static_cast<uint8_t*>(L.in.p);
        std::memcpy(h, aoff.data(), 8 * m);
        std::memcpy(h + o_slot, aslot.data(), 4 * m);
        std::memcpy(h + o_len, alen.data(), 4 * m);
        std::memcpy(h + o_dst, dst, dl);
        if (!amsg.empty()) std::memcpy(h + o_msg, amsg.data(), amsg.size());
        BLS_HIP(nwv_stage::stage_h2d(in, h, total, L.stream));
        hipLaunchKernelGGL(k_blsw_h2c_ahead, dim3((unsigned)m), dim3(64), 0, L.stream, (uint32_t)m,
                           (const uint8_t*)(in + o_msg), reinterpret_cast<const uint64_t*>(in),
                           reinterpret_cast<const uint32_t*>(in + o_len), (const uint8_t*)(in + o_dst), (uint32_t)dl,
                           static_cast<uint32_t*>(d.mr.rec.p), reinterpret_cast<const uint32_t*>(in + o_slot));
        BLS_HIP(hipGetLastError());
        BLS_HIP(hipStreamSynchronize(L.stream));
        ms.finish(nullptr, nullptr);
    }
    return NWV_OK;
}

// a call splits over the devices only into ranges of at least this many items (env
// NWV_BLS_SHARD_MIN, read once)
size_t bls_shard_min() {
    static const size_t v = [] {
        const char* e = std::getenv("NWV_BLS_SHARD_MIN");
        return e ? (size_t)std::strtoull(e, nullptr, 10) : (size_t)256;
    }();
    return v;
}

const uint8_t* dst_or_default(const uint8_t* dst, size_t* dl) {
    if (dst) return dst;
    *dl = sizeof(NWV_BLS_DST) - 1;
    return reinterpret_cast<const uint8_t*>(NWV_BLS_DST);
}

}  // namespace

__attribute__((visibility("hidden"))) void nwv_bls_ctx_release(nwv_ctx* ctx) {
    std::lock_guard<std::mutex> g(g_mu);
    auto it = g_devs.find(ctx);
    if (it == g_devs.end()) return;
    for (BlsDev* d : it->second->devs) {
        (void)hipSetDevice(d->ordinal);
        delete d;
    }
    delete it->second;
    g_devs.erase(it);
}

// nwv_diag_device_counters of the BLS12-381 engine (values [0, 6), include/nwv.h)
__attribute__((visibility("hidden"))) int nwv_bls_device_counters(nwv_ctx* ctx, int device_index, uint64_t* out,
                                                                  int cap) {
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    if (device_index < 0 || device_index >= (int)c->devs.size())
        return nwv_internal_set_err(NWV_ERR_ARG, "bad device index");
    const nwv::PlaceEntry e = c->place->get((size_t)device_index);
    const uint64_t v[6] = {e.ranges[NWV_ENGINE_BLS], e.items[NWV_ENGINE_BLS], e.out_ranges, e.peak,
                           (uint64_t)c->devs[device_index]->ordinal, c->devs.size()};
    for (int k = 0; k < cap && k < 6; k++) out[k] = v[k];
    return 6;
}

// the BLS12-381 engine's side of nwv_set_latency_max, nwv_latency_max, nwv_diag_qos and
// nwv_diag_qos_priority (include/nwv.h)
__attribute__((visibility("hidden"))) int nwv_bls_set_latency_max(nwv_ctx* ctx, size_t n) {
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    // below the shard minimum: a latency-class call is always one range
    const size_t v = nwv::latency_clamp(n, bls_shard_min());
    for (BlsDev* d : c->devs) d->latency_max.store(v);
    return NWV_OK;
}
__attribute__((visibility("hidden"))) size_t nwv_bls_latency_max(const nwv_ctx* ctx) {
    BlsCtx* c;
    if (ctx_of(const_cast<nwv_ctx*>(ctx), &c)) return 0;
    return c->devs[0]->latency_max.load();
}
__attribute__((visibility("hidden"))) int nwv_bls_diag_qos(nwv_ctx* ctx, int device_index, uint64_t out[8]) {
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    if (device_index < 0 || device_index >= (int)c->devs.size())
        return nwv_internal_set_err(NWV_ERR_ARG, "bad device index");
    c->devs[device_index]->pool.counters(out);
    return NWV_OK;
}
__attribute__((visibility("hidden"))) int nwv_bls_diag_qos_priority(nwv_ctx* ctx, int device_index, int out[3]) {
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    if (device_index < 0 || device_index >= (int)c->devs.size())
        return nwv_internal_set_err(NWV_ERR_ARG, "bad device index");
    BlsDev* d = c->devs[device_index];
    BLS_HIP(hipSetDevice(d->ordinal));
    (void)nwv::stream_priority_range(out + 1);
    if (const BlsLane* l = d->pool.first_reserved()) BLS_HIP(hipStreamGetPriority(l->stream, &out[0]));
    return NWV_OK;
}

// the message-ring counters of the calling thread's last verify call on a context
// (nwv_bls_last_msgs), and the aggregate-key ring's (nwv_bls_last_apk)
struct MsgStat {
    uint64_t v[5] = {0, 0, 0, 0, 0};
    uint64_t a[4] = {0, 0, 0, 0};
};
static thread_local std::unordered_map<const nwv_ctx*, MsgStat> t_last_msgs;

// nwv_bls_verify_many, with the ahead messages of nwv_bls_verify_many_ahead (ah.n = 0: none)
static int verify_many_impl(nwv_ctx* ctx, size_t n_keys, const uint8_t* keys, size_t n, const uint8_t* sigs,
                            const uint32_t* pk_off, const uint32_t* pk_cnt, const uint32_t* pk_idx,
                            const uint8_t* msg_base, const uint64_t* msg_off, const uint32_t* msg_len,
                            const uint8_t* dst, size_t dst_len, int32_t* status, const Ahead& ah) {
    MsgStat& mstat = t_last_msgs[ctx];
    mstat = MsgStat{};
    if (n == 0) return NWV_OK;
    if (!sigs || !pk_off || !pk_cnt || !msg_off || !msg_len || !status || (n_keys && !keys))
        return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    if (n > MAX_CALL_KEYS || n_keys > MAX_CALL_KEYS) return nwv_internal_set_err(NWV_ERR_ARG, "batch too large");
    dst = dst_or_default(dst, &dst_len);
    if (dst_len > 255) return nwv_internal_set_err(NWV_ERR_ARG, "DST longer than 255 bytes");
    // host-side shape checks: every key index and message range in bounds
    size_t n_idx = 0, msg_bytes = 0;
    for (size_t i = 0; i < n; i++) {
        n_idx = std::max<size_t>(n_idx, (size_t)pk_off[i] + pk_cnt[i]);
        if (msg_len[i] && !msg_base) return nwv_internal_set_err(NWV_ERR_ARG, "null msg_base");
        msg_bytes = std::max<size_t>(msg_bytes, msg_off[i] + msg_len[i]);
    }
    if (n_idx && !pk_idx) return nwv_internal_set_err(NWV_ERR_ARG, "null pk_idx");
    for (size_t k = 0; k < n_idx; k++)
        if (pk_idx[k] >= n_keys) return nwv_internal_set_err(NWV_ERR_ARG, "key index out of range");
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    // items split by index over the context's devices (bls_shard.h); a small call is one range on
    // the least-loaded device, the ranges of a larger one rotate (place.h)
    const auto ranges = bls_shard_ranges(n, c->devs.size(), bls_shard_min());
    const auto tickets = nwv::place_ranges(*c->place, ranges, NWV_ENGINE_BLS);
    t_last_dev[ctx] = tickets[0].dev();
    if (ranges.size() == 1) {
        BlsDev& d = *c->devs[tickets[0].dev()];
        // (a single range of at most nwv_latency_max items is latency class: lane_pool.h)
        return verify_on(d, n_keys, keys, n, sigs, pk_off, pk_cnt, pk_idx, n_idx, msg_base, msg_off, msg_len, msg_bytes,
                         dst, dst_len, status, ah.n ? &ah : nullptr, mstat.v, mstat.a, n <= d.latency_max.load());
    }
    std::vector<std::string> err(ranges.size());
    std::vector<MsgStat> rstat(ranges.size());  // (the ranges run on threads of their own)
    rc = bls_for_ranges(ranges, [&](size_t k, size_t lo, size_t hi) -> int {
        size_t ni = 0, mb = 0;  // the range's own key-index and message extents
        for (size_t i = lo; i < hi; i++) {
            ni = std::max<size_t>(ni, (size_t)pk_off[i] + pk_cnt[i]);
            mb = std::max<size_t>(mb, msg_off[i] + msg_len[i]);
        }
        const int e = verify_on(*c->devs[tickets[k].dev()], n_keys, keys, hi - lo, sigs + 48 * lo, pk_off + lo,
                                pk_cnt + lo, pk_idx, ni, msg_base, msg_off + lo, msg_len + lo, mb, dst, dst_len,
                                status + lo, nullptr, rstat[k].v, rstat[k].a);
        if (e) err[k] = nwv_last_error();
        return e;
    });
    if (rc)  // the failing range's message, on the caller's thread
        for (size_t k = 0; k < err.size(); k++)
            if (!err[k].empty()) return nwv_internal_set_err(rc, err[k].c_str());
    if (rc) return rc;
    for (const MsgStat& s : rstat) {
        for (int k = 0; k < 5; k++) mstat.v[k] += s.v[k];
        for (int k = 0; k < 4; k++) mstat.a[k] += s.a[k];
    }
    // a split call's ahead messages whose gates passed: hashed once the statuses are known, into
    // every device's ring (a range cannot read another range's statuses)
    if (ah.n) {
        std::vector<uint8_t> sel(ah.n);
        for (size_t j = 0; j < ah.n; j++)
            sel[j] = !ah.gate || ah.gate[j] == UINT32_MAX || status[ah.gate[j]] == NWV_BLS_OK;
        rc = on_all_devices(*c, [&](BlsDev& d) {
            return msg_ring_fill(d, ah.n, ah.base, ah.off, ah.len, sel.data(), dst, dst_len);
        });
    }
    return rc;
}

extern "C" {

int nwv_bls_verify_many(nwv_ctx* ctx, size_t n_keys, const uint8_t* keys, size_t n, const uint8_t* sigs,
                        const uint32_t* pk_off, const uint32_t* pk_cnt, const uint32_t* pk_idx,
                        const uint8_t* msg_base, const uint64_t* msg_off, const uint32_t* msg_len,
                        const uint8_t* dst, size_t dst_len, int32_t* status) {
    return verify_many_impl(ctx, n_keys, keys, n, sigs, pk_off, pk_cnt, pk_idx, msg_base, msg_off, msg_len, dst,
                            dst_len, status, Ahead{});
}

int nwv_bls_verify_many_ahead(nwv_ctx* ctx, size_t n_keys, const uint8_t* keys, size_t n, const uint8_t* sigs,
                              const uint32_t* pk_off, const uint32_t* pk_cnt, const uint32_t* pk_idx,
                              const uint8_t* msg_base, const uint64_t* msg_off, const uint32_t* msg_len,
                              const uint8_t* dst, size_t dst_len, int32_t* status, size_t n_ahead,
                              const uint8_t* ahead_base, const uint64_t* ahead_off, const uint32_t* ahead_len,
                              const uint32_t* ahead_gate) {
    Ahead ah;
    if (n_ahead) {
        if (!ahead_off || !ahead_len) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
        if (n_ahead > (1u << 20)) return nwv_internal_set_err(NWV_ERR_ARG, "too many ahead messages");
        for (size_t j = 0; j < n_ahead; j++) {
            if (ahead_len[j] && !ahead_base) return nwv_internal_set_err(NWV_ERR_ARG, "null ahead_base");
            if (ahead_gate && ahead_gate[j] != UINT32_MAX && ahead_gate[j] >= n)
                return nwv_internal_set_err(NWV_ERR_ARG, "ahead gate out of range");
        }
        ah = Ahead{n_ahead, ahead_base, ahead_off, ahead_len, ahead_gate};
    }
    return verify_many_impl(ctx, n_keys, keys, n, sigs, pk_off, pk_cnt, pk_idx, msg_base, msg_off, msg_len, dst,
                            dst_len, status, ah);
}

int nwv_bls_set_msg_ring(nwv_ctx* ctx, size_t slots) {
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    if (slots > nwv::BlsMsgRing::MAX_SLOTS) return nwv_internal_set_err(NWV_ERR_ARG, "message ring larger than 65,536 slots");
    static std::mutex mu;  // one setter at a time
    std::lock_guard<std::mutex> g(mu);
    if (slots) {
        for (BlsDev* d : c->devs)
            if (d->mr.ring.cap() && d->mr.ring.cap() != slots)
                return nwv_internal_set_err(NWV_ERR_ARG, "the message ring's size is fixed once set");
        for (BlsDev* d : c->devs) {
            if (d->mr.ring.cap()) continue;
            if (hipSetDevice(d->ordinal) != hipSuccess) return nwv_internal_set_err(NWV_ERR_HIP, "hipSetDevice (bls)");
            if ((rc = d->mr.rec.ensure((size_t)4 * G1H_REC_WORDS * slots))) return rc;
            d->mr.ring.init((uint32_t)slots);
        }
    }
    for (BlsDev* d : c->devs) d->mr.on.store(slots != 0, std::memory_order_release);
    return NWV_OK;
}

size_t nwv_bls_msg_ring(const nwv_ctx* ctx) {
    BlsCtx* c;
    if (ctx_of(const_cast<nwv_ctx*>(ctx), &c)) return 0;
    BlsDev* d = c->devs[0];
    return d->mr.on.load(std::memory_order_acquire) ? d->mr.ring.cap() : 0;
}

int nwv_bls_hash_ahead(nwv_ctx* ctx, size_t n, const uint8_t* msg_base, const uint64_t* msg_off,
                       const uint32_t* msg_len, const uint8_t* dst, size_t dst_len) {
    if (n == 0) return NWV_OK;
    if (!msg_off || !msg_len) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    for (size_t j = 0; j < n; j++)
        if (msg_len[j] && !msg_base) return nwv_internal_set_err(NWV_ERR_ARG, "null msg_base");
    dst = dst_or_default(dst, &dst_len);
    if (dst_len > 255) return nwv_internal_set_err(NWV_ERR_ARG, "DST longer than 255 bytes");
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    // every device: placement may send the later call to any of them
    return on_all_devices(*c, [&](BlsDev& d) { return msg_ring_fill(d, n, msg_base, msg_off, msg_len, nullptr, dst, dst_len); });
}

int nwv_bls_last_msgs(nwv_ctx* ctx, uint64_t out[5]) {
    if (!out) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    const auto it = t_last_msgs.find(ctx);
    for (int k = 0; k < 5; k++) out[k] = it != t_last_msgs.end() ? it->second.v[k] : 0;
    return NWV_OK;
}

int nwv_bls_msg_ring_stats(nwv_ctx* ctx, uint64_t out[3]) {
    if (!out) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    BlsDev* d;
    int rc = last_dev_of(ctx, &d);
    if (rc) return rc;
    d->mr.ring.counts(out);
    return NWV_OK;
}

int nwv_bls_set_apk_ring(nwv_ctx* ctx, size_t slots) {
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    if (slots > nwv::BlsApkRing::MAX_SLOTS)
        return nwv_internal_set_err(NWV_ERR_ARG, "aggregate-key ring larger than 4,096 slots");
    static std::mutex mu;  // one setter at a time
    std::lock_guard<std::mutex> g(mu);
    if (slots) {
        for (BlsDev* d : c->devs)
            if (d->ar.ring.cap() && d->ar.ring.cap() != slots)
                return nwv_internal_set_err(NWV_ERR_ARG, "the aggregate-key ring's size is fixed once set");
        for (BlsDev* d : c->devs) {
            if (d->ar.ring.cap()) continue;
            if (hipSetDevice(d->ordinal) != hipSuccess) return nwv_internal_set_err(NWV_ERR_HIP, "hipSetDevice (bls)");
            if ((rc = d->ar.rec.ensure((size_t)4 * G2_REC_WORDS * slots)) ||
                (rc = d->ar.lines.ensure((size_t)4 * KL_WORDS * slots)))
                return rc;
            d->ar.ring.init((uint32_t)slots);
        }
    }
    for (BlsDev* d : c->devs) d->ar.on.store(slots != 0, std::memory_order_release);
    return NWV_OK;
}

size_t nwv_bls_apk_ring(const nwv_ctx* ctx) {
    BlsCtx* c;
    if (ctx_of(const_cast<nwv_ctx*>(ctx), &c)) return 0;
    BlsDev* d = c->devs[0];
    return d->ar.on.load(std::memory_order_acquire) ? d->ar.ring.cap() : 0;
}

int nwv_bls_last_apk(nwv_ctx* ctx, uint64_t out[4]) {
    if (!out) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    const auto it = t_last_msgs.find(ctx);
    for (int k = 0; k < 4; k++) out[k] = it != t_last_msgs.end() ? it->second.a[k] : 0;
    return NWV_OK;
}

int nwv_bls_apk_ring_stats(nwv_ctx* ctx, uint64_t out[3]) {
    if (!out) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    BlsDev* d;
    int rc = last_dev_of(ctx, &d);
    if (rc) return rc;
    d->ar.ring.counts(out);
    return NWV_OK;
}

int nwv_bls_last_kernel_ms(nwv_ctx* ctx, double out_ms[5]) {
    if (!out_ms) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    BlsDev* d;
    int rc = last_dev_of(ctx, &d);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(d->stat_mu);
    for (int k = 0; k < 5; k++) out_ms[k] = d->last_ms[k];
    return NWV_OK;
}

int nwv_bls_last_path(nwv_ctx* ctx) {
    BlsDev* d;
    int rc = last_dev_of(ctx, &d);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(d->stat_mu);
    return d->last_path;
}

int nwv_bls_set_wave_batch_min(nwv_ctx* ctx, size_t n) {
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    for (BlsDev* d : c->devs) d->wave_batch_min.store(n, std::memory_order_relaxed);
    return NWV_OK;
}

size_t nwv_bls_wave_batch_min(const nwv_ctx* ctx) {
    BlsCtx* c;
    if (ctx_of(const_cast<nwv_ctx*>(ctx), &c)) return 0;
    return c->devs[0]->wave_batch_min.load(std::memory_order_relaxed);
}

int nwv_bls_last_batch(nwv_ctx* ctx, uint64_t out[3]) {
    if (!out) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    BlsDev* d;
    int rc = last_dev_of(ctx, &d);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(d->stat_mu);
    for (int k = 0; k < 3; k++) out[k] = d->last_batch[k];
    return NWV_OK;
}

int nwv_bls_set_key_batch_min(nwv_ctx* ctx, size_t n) {
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    for (BlsDev* d : c->devs) d->key_batch_min.store(n, std::memory_order_relaxed);
    return NWV_OK;
}

size_t nwv_bls_key_batch_min(const nwv_ctx* ctx) {
    BlsCtx* c;
    if (ctx_of(const_cast<nwv_ctx*>(ctx), &c)) return 0;
    return c->devs[0]->key_batch_min.load(std::memory_order_relaxed);
}

int nwv_bls_last_key_batch(nwv_ctx* ctx, uint64_t out[5]) {
    if (!out) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    BlsDev* d;
    int rc = last_dev_of(ctx, &d);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(d->stat_mu);
    for (int k = 0; k < 5; k++) out[k] = d->last_kbatch[k];
    return NWV_OK;
}

int nwv_bls_set_apk_dense_min(nwv_ctx* ctx, size_t n) {
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    for (BlsDev* d : c->devs) d->apk_dense_min.store(n, std::memory_order_relaxed);
    return NWV_OK;
}

size_t nwv_bls_apk_dense_min(const nwv_ctx* ctx) {
    BlsCtx* c;
    if (ctx_of(const_cast<nwv_ctx*>(ctx), &c)) return 0;
    return c->devs[0]->apk_dense_min.load(std::memory_order_relaxed);
}

int nwv_bls_last_apk_dense(nwv_ctx* ctx, uint64_t out[4]) {
    if (!out) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    BlsDev* d;
    int rc = last_dev_of(ctx, &d);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(d->stat_mu);
    for (int k = 0; k < 4; k++) out[k] = d->last_apkd[k];
    return NWV_OK;
}

int nwv_bls_last_keys(nwv_ctx* ctx, uint64_t out[2]) {
    if (!out) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    BlsDev* d;
    int rc = last_dev_of(ctx, &d);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(d->stat_mu);
    out[0] = d->last_keys[0];
    out[1] = d->last_keys[1];
    return NWV_OK;
}

int nwv_bls_keycache_register(nwv_ctx* ctx, size_t n_keys, const uint8_t* keys) {
    if (n_keys && !keys) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    if (n_keys > KC_CAP) return nwv_internal_set_err(NWV_ERR_ARG, "more keys than the cache holds");
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    // every device verifies its own item range against its own cache
    return n_keys ? on_all_devices(*c, [&](BlsDev& d) { return keycache_register(d, n_keys, keys); }) : NWV_OK;
}

int nwv_bls_keycache_reset(nwv_ctx* ctx) {
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    for (BlsDev* d : c->devs) {
        std::unique_lock<std::shared_mutex> g(d->kc.mu);  // waits for calls that read the records
        d->kc.slot.clear();
        d->kc.used = 0;
        // the aggregate-key ring's sets are lists of the slots just dropped: the same list will
        // name other keys, so every set and the filter go, under the same hold
        d->ar.ring.reset();
    }
    return NWV_OK;
}

int nwv_bls_keycache_size(nwv_ctx* ctx) {
    BlsDev* d;
    int rc = dev_of(ctx, &d);
    if (rc) return rc;
    std::shared_lock<std::shared_mutex> g(d->kc.mu);
    return (int)d->kc.used;
}

int nwv_bls_aggregate_verify(nwv_ctx* ctx, const uint8_t* sig48, const uint8_t* pks, size_t n_pks, const uint8_t* msg,
                             size_t msg_len) {
    if (!sig48) return NWV_ERR_SIGNATURE;  // sig: None
    if ((n_pks && !pks) || (msg_len && !msg)) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    std::vector<uint32_t> idx(n_pks);
    for (size_t k = 0; k < n_pks; k++) idx[k] = (uint32_t)k;
    const uint32_t off = 0, cnt = (uint32_t)n_pks, len = (uint32_t)msg_len;
    const uint64_t moff = 0;
    int32_t st = 0;
    static const uint8_t empty[1] = {0};
    const int rc = nwv_bls_verify_many(ctx, n_pks, pks, 1, sig48, &off, &cnt, idx.data(), msg_len ? msg : empty, &moff,
                                       &len, nullptr, 0, &st);
    if (rc) return rc;
    return st == NWV_BLS_OK ? NWV_OK : NWV_ERR_SIGNATURE;
}

int nwv_bls_verify(nwv_ctx* ctx, const uint8_t pk[96], const uint8_t* msg, size_t msg_len, const uint8_t sig[48]) {
    if (!pk || !sig) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    return nwv_bls_aggregate_verify(ctx, sig, pk, 1, msg, msg_len);
}

int nwv_bls_aggregate(nwv_ctx* ctx, size_t n, const uint8_t* sigs48, uint8_t out48[48], int32_t* status_or_null) {
    if (status_or_null) *status_or_null = NWV_BLS_AGGR_MISMATCH;
    if (n == 0) return NWV_ERR_SIGNATURE;
    if (!sigs48 || !out48) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    if (n > (1u << 26)) return nwv_internal_set_err(NWV_ERR_ARG, "batch too large");
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    // the first device, in index order, whose verified-signature ring holds every signature of the
    // call (a host-side lookup; the ring is read again below, under the lock the kernels run
    // under); none: the least-loaded device, which decodes them
    size_t holder = c->devs.size();
    if (c->devs.size() > 1 && n <= SC_CAP && !(c->devs[0]->flags & NWV_FLAG_NO_SIGCACHE))
        for (size_t j = 0; j < c->devs.size() && holder == c->devs.size(); j++) {
            BlsSigCache& sc = c->devs[j]->sc;
            std::shared_lock<std::shared_mutex> hold(sc.mu);
            if (!sc.rec.p) continue;
            bool all = true;
            Sig48 k;
            for (size_t i = 0; i < n && all; i++) {
                std::memcpy(k.b, sigs48 + 48 * i, 48);
                all = sc.slot.find(k) != sc.slot.end();
            }
            if (all) holder = j;
        }
    const nwv::Ticket ticket = holder < c->devs.size() ? nwv::Ticket(*c->place, holder, (uint64_t)n, NWV_ENGINE_BLS)
                                                       : nwv::Ticket(*c->place, (uint64_t)n, NWV_ENGINE_BLS);
    BlsDev* d = c->devs[ticket.dev()];
    LaneLease lane(*d, n <= d->latency_max.load());
    if ((rc = lane.rc())) return rc;
    BlsLane& L = *lane;
    // scratch: records, statuses, the sum tree's two partial-sum levels, the output, decode statuses
    const size_t n_part = (n + wave::G1SUM_N - 1) / wave::G1SUM_N + 1;  // g1_sum_per
    const size_t w_rec = 0, w_st = al256(4 * G1_REC_WORDS * n), w_pa = al256(w_st + 4 * n),
                 w_pb = al256(w_pa + 4 * G1P_WORDS * n_part), w_out = al256(w_pb + 4 * G1P_WORDS * n_part),
                 w_ost = w_out + 64, w_st2 = al256(w_ost + 8), w_end = w_st2 + 4 * n;
    if ((rc = L.in.ensure(48 * n)) || (rc = L.work.ensure(w_end)) || (rc = L.stage.ensure(128))) return rc;
    uint8_t* w = static_cast<uint8_t*>(L.work.p);
    // the sum of the records at `in` (through the positions idx_d when given) as a tree of
    // k_blsw_g1_sum levels; the last (one block) takes the first bad status of st_d when given
    auto sum_tree = [&](const uint32_t* in, const uint32_t* idx_d, const int32_t* st_d) {
        uint32_t m = (uint32_t)n;
        const uint32_t* src = in;
        int hom = 0, flip = 0;
        while (m > (uint32_t)wave::G1SUM_N) {
            const uint32_t per = g1_sum_per(m);
            const uint32_t nb = (m + per - 1) / per;
            auto* dst = reinterpret_cast<uint32_t*>(w + (flip ? w_pb : w_pa));
            hipLaunchKernelGGL(k_blsw_g1_sum, dim3(nb), dim3(64), 0, L.stream, m, src, idx_d, hom, dst, per);
            src = dst;
            idx_d = nullptr;
            hom = 1;
            m = nb;
            flip ^= 1;
        }
        hipLaunchKernelGGL(k_blsw_g1_sum_fin, dim3(1), dim3(64), 0, L.stream, m, src, idx_d, hom,
                           st_d ? (uint32_t)n : 0u, st_d, w + w_out, reinterpret_cast<int32_t*>(w + w_ost));
    };
    auto fetch = [&]() -> int {
        BLS_HIP(hipGetLastError());
        uint8_t* hs = static_cast<uint8_t*>(L.stage.p);
        BLS_HIP(hipMemcpyAsync(hs, w + w_out, 64 + 8, hipMemcpyDeviceToHost, L.stream));
        BLS_HIP(hipStreamSynchronize(L.stream));
        int32_t st;
        std::memcpy(&st, hs + 64, 4);
        if (status_or_null) *status_or_null = st;
        if (st != NWV_BLS_OK) return NWV_ERR_SIGNATURE;
        std::memcpy(out48, hs, 48);
        return NWV_OK;
    };
    // every signature verified by an earlier call: sum the ring's records (no decode, no G1 check)
    if (!(d->flags & NWV_FLAG_NO_SIGCACHE)) {
        std::shared_lock<std::shared_mutex> hold(d->sc.mu);
        if (d->sc.rec.p && n <= SC_CAP) {
            std::vector<uint32_t> pos(n);
            bool all = true;
            Sig48 k;
            for (size_t i = 0; i < n && all; i++) {
                std::memcpy(k.b, sigs48 + 48 * i, 48);
                auto it = d->sc.slot.find(k);
                if (it == d->sc.slot.end()) all = false;
                else pos[i] = it->second;
            }
            if (all) {
                BLS_HIP(nwv_stage::stage_h2d(L.in.p, pos.data(), 4 * n, L.stream));
                sum_tree(static_cast<const uint32_t*>(d->sc.rec.p), static_cast<const uint32_t*>(L.in.p), nullptr);
                return fetch();
            }
        }
    }
    BLS_HIP(nwv_stage::stage_h2d(L.in.p, sigs48, 48 * n, L.stream));
    if (n <= 1024) {  // decode on one lane each, the G1 checks on a wave each
        auto* sdec = reinterpret_cast<int32_t*>(w + w_st2);
        hipLaunchKernelGGL(k_blsw_sigdec, dim3(kBlocks(n)), dim3(BLS_LANES), 0, L.stream, (uint32_t)n,
                           (const uint8_t*)L.in.p, reinterpret_cast<uint32_t*>(w + w_rec), sdec);
        hipLaunchKernelGGL(k_blsw_sub, dim3((unsigned)n), dim3(64), 0, L.stream, (uint32_t)n,
                           reinterpret_cast<const uint32_t*>(w + w_rec), (const int32_t*)sdec,
                           reinterpret_cast<int32_t*>(w + w_st));
        hipLaunchKernelGGL(k_bls_st_join, dim3(kBlocks(n)), dim3(BLS_LANES), 0, L.stream, (uint32_t)n,
                           (const int32_t*)sdec, reinterpret_cast<int32_t*>(w + w_st));
    } else {
        hipLaunchKernelGGL(k_bls_sigs, dim3(kBlocks(n)), dim3(BLS_LANES), 0, L.stream, (uint32_t)n,
                           (const uint8_t*)L.in.p, reinterpret_cast<uint32_t*>(w + w_rec),
                           reinterpret_cast<int32_t*>(w + w_st));
    }
    sum_tree(reinterpret_cast<const uint32_t*>(w + w_rec), nullptr, reinterpret_cast<const int32_t*>(w + w_st));
    return fetch();
}

int nwv_bls_verify_batch_empty_fail(nwv_ctx* ctx, const uint8_t* msg, size_t msg_len, const uint8_t* pks,
                                    size_t n_pks, const uint8_t* sigs, size_t n_sigs) {
    if (n_sigs == 0)
        return nwv_internal_set_err(NWV_ERR_EMPTY,
                                    "Critical Error! This behavious can signal something dangerous, and that "
                                    "someone may be trying to bypass signature verification through providing "
                                    "empty batches.");
    if (n_pks != n_sigs)
        return nwv_internal_set_err(NWV_ERR_LENGTH, "Mismatch between number of signatures and public keys provided");
    uint8_t agg[48];
    int rc = nwv_bls_aggregate(ctx, n_sigs, sigs, agg, nullptr);
    if (rc) return rc;
    return nwv_bls_aggregate_verify(ctx, agg, pks, n_pks, msg, msg_len);
}

int nwv_bls_aggregate_batch_verify(nwv_ctx* ctx, size_t n_aggs, const uint8_t* const* sigs48,
                                   const uint8_t* const* pks, const size_t* n_pks, const uint8_t* const* msgs,
                                   const size_t* msg_lens, size_t n_msgs) {
    if (n_aggs != n_msgs) return nwv_internal_set_err(NWV_ERR_LENGTH, "signatures / messages count mismatch");
    if (n_aggs == 0) return NWV_OK;
    if (!sigs48 || !pks || !n_pks || !msgs || !msg_lens) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    std::vector<uint8_t> keys, sg(48 * n_aggs), mb;
    std::vector<uint32_t> off(n_aggs), cnt(n_aggs), idx, len(n_aggs);
    std::vector<uint64_t> moff(n_aggs);
    for (size_t i = 0; i < n_aggs; i++) {
        if (!sigs48[i]) return NWV_ERR_SIGNATURE;  // an aggregate holding no signature
        std::memcpy(sg.data() + 48 * i, sigs48[i], 48);
        off[i] = (uint32_t)idx.size();
        cnt[i] = (uint32_t)n_pks[i];
        for (size_t k = 0; k < n_pks[i]; k++) {
            idx.push_back((uint32_t)(keys.size() / 96));
            keys.insert(keys.end(), pks[i] + 96 * k, pks[i] + 96 * (k + 1));
        }
        moff[i] = mb.size();
        len[i] = (uint32_t)msg_lens[i];
        if (msg_lens[i]) mb.insert(mb.end(), msgs[i], msgs[i] + msg_lens[i]);
    }
    mb.push_back(0);
    std::vector<int32_t> st(n_aggs);
    const int rc = nwv_bls_verify_many(ctx, keys.size() / 96, keys.data(), n_aggs, sg.data(), off.data(), cnt.data(),
                                       idx.data(), mb.data(), moff.data(), len.data(), nullptr, 0, st.data());
    if (rc) return rc;
    for (int32_t s : st)
        if (s != NWV_BLS_OK) return NWV_ERR_SIGNATURE;
    return NWV_OK;
}

static int simple_launch(nwv_ctx* ctx, size_t in_bytes, const void* in_host, size_t in2_bytes, const void* in2_host,
                         size_t out_bytes, void* out_host,
                         const std::function<void(hipStream_t, uint8_t*, uint8_t*, uint8_t*)>& launch) {
    BlsDev* d;
    int rc = dev_of(ctx, &d);
    if (rc) return rc;
    LaneLease lane(*d);
    if ((rc = lane.rc())) return rc;
    BlsLane& L = *lane;
    const size_t o2 = (in_bytes + 255) & ~(size_t)255;
    if ((rc = L.in.ensure(o2 + in2_bytes + 16)) || (rc = L.work.ensure(out_bytes + 16))) return rc;
    uint8_t* in = static_cast<uint8_t*>(L.in.p);
    if (in_bytes) BLS_HIP(hipMemcpyAsync(in, in_host, in_bytes, hipMemcpyHostToDevice, L.stream));
    if (in2_bytes) BLS_HIP(hipMemcpyAsync(in + o2, in2_host, in2_bytes, hipMemcpyHostToDevice, L.stream));
    launch(L.stream, in, in + o2, static_cast<uint8_t*>(L.work.p));
    BLS_HIP(hipGetLastError());
    BLS_HIP(hipMemcpyAsync(out_host, L.work.p, out_bytes, hipMemcpyDeviceToHost, L.stream));
    BLS_HIP(hipStreamSynchronize(L.stream));
    return NWV_OK;
}

// messages + offsets + lengths + dst packed into one host block (the second input)
static std::vector<uint8_t> pack_msgs(size_t n, const uint8_t* msg_base, const uint64_t* msg_off,
                                      const uint32_t* msg_len, const uint8_t* dst, size_t dl, size_t* o_off,
                                      size_t* o_len, size_t* o_dst) {
    size_t bytes = 0;
    for (size_t i = 0; i < n; i++) bytes = std::max<size_t>(bytes, msg_off[i] + msg_len[i]);
    *o_off = (bytes + 1 + 7) & ~(size_t)7;
    *o_len = *o_off + 8 * n;
    *o_dst = *o_len + 4 * n;
    std::vector<uint8_t> v(*o_dst + dl + 1, 0);
    if (bytes) std::memcpy(v.data(), msg_base, bytes);
    std::memcpy(v.data() + *o_off, msg_off, 8 * n);
    std::memcpy(v.data() + *o_len, msg_len, 4 * n);
    std::memcpy(v.data() + *o_dst, dst, dl);
    return v;
}

int nwv_bls_keygen_many(nwv_ctx* ctx, size_t n, const uint8_t* sks, uint8_t* pks) {
    if (n == 0) return NWV_OK;
    if (!sks || !pks) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    return simple_launch(ctx, 32 * n, sks, 0, nullptr, 96 * n, pks, [&](hipStream_t s, uint8_t* in, uint8_t*, uint8_t* out) {
        hipLaunchKernelGGL(k_bls_keygen, dim3(kBlocks(n)), dim3(BLS_LANES), 0, s, (uint32_t)n, in, out);
    });
}

int nwv_bls_sign_many(nwv_ctx* ctx, size_t n, const uint8_t* sks, const uint8_t* msg_base, const uint64_t* msg_off,
                      const uint32_t* msg_len, const uint8_t* dst, size_t dst_len, uint8_t* sigs) {
    if (n == 0) return NWV_OK;
    if (!sks || !msg_off || !msg_len || !sigs) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    dst = dst_or_default(dst, &dst_len);
    size_t o_off, o_len, o_dst;
    const std::vector<uint8_t> m = pack_msgs(n, msg_base, msg_off, msg_len, dst, dst_len, &o_off, &o_len, &o_dst);
    return simple_launch(ctx, 32 * n, sks, m.size(), m.data(), 48 * n, sigs,
                         [&](hipStream_t s, uint8_t* in, uint8_t* mm, uint8_t* out) {
                             hipLaunchKernelGGL(k_bls_sign, dim3(kBlocks(n)), dim3(BLS_LANES), 0, s, (uint32_t)n, in, mm,
                                                reinterpret_cast<const uint64_t*>(mm + o_off),
                                                reinterpret_cast<const uint32_t*>(mm + o_len), mm + o_dst,
                                                (uint32_t)dst_len, out);
                         });
}

int nwv_bls_hash_to_g1_many(nwv_ctx* ctx, size_t n, const uint8_t* msg_base, const uint64_t* msg_off,
                            const uint32_t* msg_len, const uint8_t* dst, size_t dst_len, uint8_t* out96) {
    if (n == 0) return NWV_OK;
    if (!msg_off || !msg_len || !out96) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    dst = dst_or_default(dst, &dst_len);
    size_t o_off, o_len, o_dst;
    const std::vector<uint8_t> m = pack_msgs(n, msg_base, msg_off, msg_len, dst, dst_len, &o_off, &o_len, &o_dst);
    return simple_launch(ctx, 0, nullptr, m.size(), m.data(), 96 * n, out96,
                         [&](hipStream_t s, uint8_t*, uint8_t* mm, uint8_t* out) {
                             hipLaunchKernelGGL(k_bls_h2c_out, dim3(kBlocks(n)), dim3(BLS_LANES), 0, s, (uint32_t)n, mm,
                                                reinterpret_cast<const uint64_t*>(mm + o_off),
                                                reinterpret_cast<const uint32_t*>(mm + o_len), mm + o_dst,
                                                (uint32_t)dst_len, out);
                         });
}

int nwv_bls_pairing_many(nwv_ctx* ctx, size_t n, const uint8_t* P96, const uint8_t* Q192, uint8_t* out576) {
    if (n == 0) return NWV_OK;
    if (!P96 || !Q192 || !out576) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    return simple_launch(ctx, 96 * n, P96, 192 * n, Q192, 576 * n, out576,
                         [&](hipStream_t s, uint8_t* in, uint8_t* in2, uint8_t* out) {
                             hipLaunchKernelGGL(k_bls_pairing_raw, dim3(kBlocks(n)), dim3(BLS_LANES), 0, s, (uint32_t)n,
                                                in, in2, out);
                         });
}

}  // extern "C"
