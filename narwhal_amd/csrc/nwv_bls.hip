// nwv_bls.hip -- BLS12-381 min_sig verification engine on gfx950: the
// kernels over bls_verify.h and the C ABI of include/nwv_bls.h.
//
// nwv_bls_verify_many runs on one lane of a device (verify_on): a plan made on the host (CallPlan:
// the call's key table against the device's key cache, its ring slots, its path), the inputs staged
// in one pinned arena and one H2D copy, then the path's function.  nwv_bls_last_path reports the
// path's code:
//   the small wave call (run_small, at most NWV_BLS_WAVE_MAX = 1,024 items; code 3), two streams:
//     side 0  k_bls_keys_fill (keys the cache does not hold), then k_blsw_pre / k_blsw_pre_r: one
//             wave per item hashes to G1 (or takes the message ring's point), one sums the keys
//     main    k_blsw_sigdec, then the ahead hashes (k_blsw_h2c_ahead) and the aggregate-key fills
//             (k_blsw_apk_fill) beside the pairing
//     side 0  k_blsw_pair_sub: the pairing checks and the signatures' G1 checks in one launch,
//             k_blsw_status; then the signature, message and aggregate-key rings' publishes
//   the large wave call (run_large_wave), three streams:
//     side 0  k_bls_keys_fill, then the key sums: k_blsw_apk, or the dense stage (k_blsd_total,
//             k_blsd_apk, k_blsw_apk_list; nwv_bls_set_apk_dense_min)
//     side 1  k_bls_h2c_2: hash to G1 on lane pairs
//     main    k_bls_sigs (decode + G1 check, one lane per item), then one of three pairing stages
//       the key-transposed check (pair_key_batch, nwv_bls_set_key_batch_min): code 6, or 7 when a
//         group rejected and its items ran per item
//       the wave batch check (pair_wave_batch, nwv_bls_set_wave_batch_min): one final
//         exponentiation a group; code 4, or 5 when a group rejected
//       per item (pair_per_item: k_blsw_pair_k, NWV_BLS_PACK items a wave): code 3
//     and k_blsw_status
//   the group engines (run_group: 8 lanes an item, the large calls' side streams with k_bls_apk_g):
//     NWV_FLAG_BLS_PER_ITEM  k_bls_pair, one two-pair Miller loop + final exponentiation an item: code 0
//     NWV_FLAG_BLS_BATCH     one random-linear-combination check over the call (k_bls_rlc_pts ..
//                            k_bls_final): code 1; k_bls_pair only when it rejects: code 2
// The statuses are the oracle's, in its order: signature decode, its G1 check (phi(P) = [-x^2] P),
// the keys (fastcrypto validates a key once, at deserialization: psi(Q) = [x] Q), the pairing
// equation e(-sig, g2) e(H, apk) == 1.  The Miller loops are the hot part: Fp products on VALU
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
// H(msg_i) on a lane pair: lane 2 j maps u_0 and lane 2 j + 1 u_1 of item 32 b + j; the odd lane
// hands its point over through LDS, the even lane adds and clears the cofactor (kmode[i] = 1: item
// i's cofactor clearing is on its key side -- H0 = the maps' sum, see k_bls_key_heff; kmode may be
// null).  32 items a wave instead of an 8-lane group's 8: a 16,384-item call is 512 waves (one per
// SIMD at most) instead of 2,048 (two per SIMD, six of every group's eight lanes repeating the
// pair's work), so each lane's dependent chain runs with its SIMD to itself.
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
// H: homogeneous records (k_blsw_pre) or affine ones (k_bls_h2c_2, h_hom = 0); apk: Jacobian
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

// an environment variable as a number clamped to [lo, hi] (unset: dflt; a negative value: lo)
unsigned long env_ulong(const char* name, unsigned long dflt, unsigned long lo, unsigned long hi) {
    const char* e = std::getenv(name);
    if (!e) return dflt;
    const unsigned long v = std::strtoul(e, nullptr, 10);
    return std::strchr(e, '-') || v < lo ? lo : v > hi ? hi : v;
}
// the engine's environment, read once per process
struct BlsEnv {
    size_t wave_max = env_ulong("NWV_BLS_WAVE_MAX", 1024, 0, ~0ul);  // small wave calls: at most this many items
    // items per group of the wave batch check
    size_t wb_grp = env_ulong("NWV_BLS_BATCH_GROUP", NWV_BLS_BATCH_GROUP_DEFAULT, 1, 4096);
    // the key-transposed batch check: groups of kb_grp eligible items, a group dropped when its
    // distinct keys + 1 exceed 1 / kb_ratio of its items (0: never)
    uint32_t kb_grp = (uint32_t)env_ulong("NWV_BLS_KEY_GROUP", NWV_BLS_KEY_GROUP_DEFAULT, 1, 65536);
    uint32_t kb_ratio = (uint32_t)env_ulong("NWV_BLS_KEY_GROUP_RATIO", 4, 0, 1024);
    unsigned long ad_forced = env_ulong("NWV_BLS_APK_LANES", 0, 0, ~0ul);  // lanes a dense item gets (4, 8, 16)
    // items per pairing wave (1..4): one LDS bank of ~6.5 KB each
    uint32_t pack = (uint32_t)env_ulong("NWV_BLS_PACK", 3, 1, BLS_PACK_MAX);
    // diagnostic (occupancy experiments): bytes of extra LDS per pairing wave
    size_t lds_pad = env_ulong("NWV_BLS_LDS_PAD", 0, 0, ~0ul);
    // a call splits over the devices only into ranges of at least this many items
    size_t shard_min = env_ulong("NWV_BLS_SHARD_MIN", 256, 0, ~0ul);
    int replicas = (int)env_ulong("NWV_BLS_DEVICE_REPLICAS", 1, 1, 8);  // BlsDev shards per device (BlsCtx)
};
const BlsEnv& bls_env() {
    static const BlsEnv e;
    return e;
}

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
// A section of a staging arena or of a scratch buffer: declared once with its element type, it
// gives the typed pointer into the host or the device copy of its buffer.
template <class T>
struct Sec {
    size_t off = 0;
    T* at(void* base) const { return reinterpret_cast<T*>(static_cast<uint8_t*>(base) + off); }
};
// sections of one buffer in order, each 256-byte aligned or packed behind the one before it
struct Layout {
    size_t end = 0;
    template <class T>
    Sec<T> packed(size_t bytes) {
        const Sec<T> s{end};
        end += bytes;
        return s;
    }
    template <class T>
    Sec<T> aligned(size_t bytes) {
        end = al256(end);
        return packed<T>(bytes);
    }
};

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
    // every one of the n signatures is in the ring: their slots -> pos (when given); the caller holds
    // the lock, shared
    bool holds_all(size_t n, const uint8_t* sigs48, uint32_t* pos = nullptr) const {
        if (!rec.p || n > SC_CAP) return false;
        Sig48 k;
        for (size_t i = 0; i < n; i++) {
            std::memcpy(k.b, sigs48 + 48 * i, 48);
            const auto it = slot.find(k);
            if (it == slot.end()) return false;
            if (pos) pos[i] = it->second;
        }
        return true;
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
    const int replicas = bls_env().replicas;
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
// device object `device_index` of the context (the diagnostics' argument)
int dev_at(nwv_ctx* ctx, int device_index, BlsCtx** c, BlsDev** out) {
    int rc = ctx_of(ctx, c);
    if (rc) return rc;
    if (device_index < 0 || device_index >= (int)(*c)->devs.size())
        return nwv_internal_set_err(NWV_ERR_ARG, "bad device index");
    *out = (*c)->devs[device_index];
    return NWV_OK;
}
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
    template <class T>
    Sec<const T> add(const void* p, size_t n) {
        const Sec<const T> s{total};
        parts.push_back({p, n});
        offs.push_back(total);
        total += al256(n);
        return s;
    }
    void fill(uint8_t* h) const {
        for (size_t k = 0; k < parts.size(); k++)
            if (parts[k].second) std::memcpy(h + offs[k], parts[k].first, parts[k].second);
    }
};

constexpr int kBlocks(size_t n) { return (int)((n + BLS_LANES - 1) / BLS_LANES); }
// blocks of the group kernels: 8 items per 64-lane block
constexpr int gBlocks(size_t n) { return (int)((n + BLS_LANES / GRP - 1) / (BLS_LANES / GRP)); }

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
    Layout o;
    const auto o_keys = o.aligned<uint8_t>(96 * m);
    const auto o_slot = o.aligned<uint32_t>(4 * m), o_rec = o.aligned<uint32_t>(4 * G2_REC_WORDS * m);
    const auto o_st = o.aligned<int32_t>(4 * m);
    const auto o_src = o.aligned<uint32_t>(4 * m), o_dst = o.aligned<uint32_t>(4 * m);
    if ((rc = lane->work.ensure(o.end)) || (rc = lane->stage.ensure(o.end))) return rc;
    void* w = lane->work.p;
    void* h = lane->stage.p;
    std::memcpy(o_keys.at(h), fk.data(), 96 * m);
    for (size_t j = 0; j < m; j++) o_slot.at(h)[j] = (uint32_t)j;
    BLS_HIP(hipMemcpyAsync(w, h, o_rec.off, hipMemcpyHostToDevice, lane->stream));
    hipLaunchKernelGGL(k_bls_keys_fill, dim3(kBlocks(m)), dim3(BLS_LANES), 0, lane->stream, (uint32_t)m, o_keys.at(w),
                       o_slot.at(w), o_rec.at(w), o_st.at(w));
    BLS_HIP(hipGetLastError());
    BLS_HIP(hipMemcpyAsync(o_st.at(h), o_st.at(w), 4 * m, hipMemcpyDeviceToHost, lane->stream));
    BLS_HIP(hipStreamSynchronize(lane->stream));
    const int32_t* kst = o_st.at(h);
    uint32_t *src = o_src.at(h), *dst = o_dst.at(h);
    size_t nv = 0;
    for (size_t j = 0; j < m && d.kc.used + nv < KC_CAP; j++)
        if (kst[j] == ST_OK) {
            src[nv] = (uint32_t)j;
            dst[nv] = d.kc.used + (uint32_t)nv;
            nv++;
        }
    if (nv == 0) return NWV_OK;
    BLS_HIP(hipMemcpyAsync(o_src.at(w), src, o.end - o_src.off, hipMemcpyHostToDevice, lane->stream));
    hipLaunchKernelGGL(k_bls_rec_copy, dim3(kBlocks(nv * G2_REC_WORDS)), dim3(BLS_LANES), 0, lane->stream,
                       (uint32_t)nv, o_src.at(w), o_dst.at(w), o_rec.at(w), static_cast<uint32_t*>(d.kc.rec.p),
                       static_cast<int32_t*>(d.kc.st.p));
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
    hipLaunchKernelGGL(k_bls_key_heff, dim3(kBlocks(nv)), dim3(BLS_LANES), 0, lane->stream, (uint32_t)nv, o_dst.at(w),
                       static_cast<const uint32_t*>(d.kc.rec.p), static_cast<uint32_t*>(d.kc.hrec.p));
    hipLaunchKernelGGL(k_blsw_key_lines, dim3((unsigned)nv), dim3(64), 0, lane->stream, (uint32_t)nv, o_dst.at(w),
                       static_cast<const uint32_t*>(d.kc.hrec.p), static_cast<uint32_t*>(d.kc.lines.p));
    BLS_HIP(hipGetLastError());
    BLS_HIP(hipStreamSynchronize(lane->stream));
    for (size_t k = 0; k < nv; k++) d.kc.slot.emplace(fresh[src[k]], dst[k]);  // published after the copy
    d.kc.used += (uint32_t)nv;
    return NWV_OK;
}

// ---- nwv_bls_verify_many on one device lane: a plan made on the host, typed buffers, one
// function per path (the file's header names the paths)
//
// what a call brings (a range of a split call brings its own extents)
struct CallIn {
    size_t n_keys;
    const uint8_t* keys;
    size_t n;
    const uint8_t* sigs;
    const uint32_t *pk_off, *pk_cnt, *pk_idx;
    size_t n_idx;  // entries of pk_idx the call's items reach
    const uint8_t* msg_base;
    const uint64_t* msg_off;
    const uint32_t* msg_len;
    size_t msg_bytes;
    const uint8_t* dst;
    size_t dl;
};
// a call's ring slots.  The order is a condition: verify_on declares its LaneLease, then its shared
// lock on the key cache, then this, so the slots are given back (ApkSlots, MsgSlots, SigSlots, each
// after its streams' waits) before the key-cache lock drops and before the lane returns to the pool
struct CallSlots {
    SigSlots kept;
    MsgSlots ms;
    ApkSlots as;
};
// everything a call decides on the host, before any GPU work
struct CallPlan {
    // pairing-check mode: the wave engine per item (default), or the 8-lane group kernels -- one
    // random-linear-combination batch check (NWV_FLAG_BLS_BATCH) or per item (NWV_FLAG_BLS_PER_ITEM)
    bool group_item = false, batch = false, wavem = false;
    bool wave_small = false;  // at most NWV_BLS_WAVE_MAX items: the two-stream call
    bool wbatch = false;      // the wave batch check: wb_ng groups, wb_m Miller entries
    bool kb_cand = false;     // the key-transposed batch check, if its plan runs
    bool ad_run = false;      // the dense key-sum stage
    bool keep = false, use_ring = false, use_apk = false;  // the signature, message and aggregate-key rings
    bool cached = false, kside = false;
    bool no_timing = false;
    size_t wb_ng = 0, wb_m = 0;
    // the key table: cache slots (lookups only) or scratch entries KC_CAP + j
    std::vector<uint32_t> ktab, fill_slot, remap, kmode;
    std::vector<uint8_t> fill_keys;
    uint64_t hits = 0;
    size_t n_dec() const { return fill_slot.size(); }  // keys decoded by this call
    // the dense key-sum stage's item lists and lanes
    nwv::ApkDenseSplit ads;
    uint32_t ad_lanes = 0;
    // the message ring's arena section: aoff | hsrc | hpub | aslot | alen | ahead messages
    std::vector<uint8_t> rsec;
    size_t n_ah = 0, r_hsrc = 0, r_hpub = 0, r_aslot = 0, r_alen = 0, r_amsg = 0;
    uint64_t mcount[5] = {0, 0, 0, 0, 0};
    // the aggregate-key ring: the call's own key lists when some item hit (a_fill: the fills' items,
    // then their slots)
    std::vector<uint32_t> a_off, a_cnt, a_idx, a_fill;
    size_t n_fill = 0;
    uint64_t acount[4] = {0, 0, 0, 0};
    // the key lists the kernels read
    const uint32_t *k_off = nullptr, *k_cnt = nullptr;
    const std::vector<uint32_t>* k_idx = nullptr;
};
// stage times of the completed call, its path and counters -> the device's "last call"
struct CallStats {
    int path = 0;
    bool untimed = false;  // a small call that recorded no stage events
    uint64_t wb[3] = {0, 0, 0}, kb[5] = {0, 0, 0, 0, 0}, ad[4] = {0, 0, 0, 0};
};

// the call's key table, its remapped key lists and the key-side flags (under the caller's shared
// lock on the cache)
void plan_keys(const BlsKeyCache& kc, const CallIn& c, CallPlan& P) {
    P.ktab.resize(c.n_keys);
    std::unordered_map<std::string, uint32_t> fresh;
    for (size_t j = 0; j < c.n_keys; j++) {
        std::string kb(reinterpret_cast<const char*>(c.keys + 96 * j), 96);
        if (P.cached) {
            auto it = kc.slot.find(kb);
            if (it != kc.slot.end()) {
                P.ktab[j] = it->second;
                P.hits++;
                continue;
            }
        }
        auto f = fresh.find(kb);
        if (f != fresh.end()) {
            P.ktab[j] = KC_CAP + f->second;
            continue;
        }
        const uint32_t e = (uint32_t)fresh.size();
        fresh.emplace(std::move(kb), e);
        P.ktab[j] = KC_CAP + e;
        P.fill_slot.push_back(e);
        P.fill_keys.insert(P.fill_keys.end(), c.keys + 96 * j, c.keys + 96 * (j + 1));
    }
    P.remap.resize(c.n_idx);
    for (size_t t = 0; t < c.n_idx; t++) P.remap[t] = P.ktab[c.pk_idx[t]];
    // key-side cofactor clearing (wave path): items whose keys are all in the cache use the keys'
    // [h_eff] pk records and line tables, and their hash skips the h_eff chain
    P.kside = P.wavem && P.cached && kc.lines_slots;
    P.kmode.resize(P.kside ? c.n : 0);
    for (size_t i = 0; i < P.kmode.size(); i++) {
        bool all = c.pk_cnt[i] > 0;
        for (uint32_t j = 0; j < c.pk_cnt[i] && all; j++) all = P.remap[c.pk_off[i] + j] < KC_CAP;
        P.kmode[i] = all ? 1u : 0u;
    }
}

// messages to hash ahead of need, packed for k_blsw_h2c_ahead: offsets | slots | lengths | bytes
struct AheadPack {
    std::vector<uint32_t> slot, len;
    std::vector<uint64_t> off;
    std::vector<uint8_t> msg;
    size_t n() const { return slot.size(); }
    void push(uint32_t ring_slot, const uint8_t* m, uint32_t l) {
        slot.push_back(ring_slot);
        len.push_back(l);
        off.push_back(msg.size());
        msg.insert(msg.end(), m, m + l);
    }
    void write(void* o_off, void* o_slot, void* o_len, void* o_msg) const {
        if (!n()) return;
        std::memcpy(o_off, off.data(), 8 * n());
        std::memcpy(o_slot, slot.data(), 4 * n());
        std::memcpy(o_len, len.data(), 4 * n());
        if (!msg.empty()) std::memcpy(o_msg, msg.data(), msg.size());
    }
};
void launch_ahead(hipStream_t s, size_t n, const uint8_t* msg, const uint64_t* off, const uint32_t* len,
                  const uint8_t* dst, size_t dl, void* ring_rec, const uint32_t* slot) {
    hipLaunchKernelGGL(k_blsw_h2c_ahead, dim3((unsigned)n), dim3(64), 0, s, (uint32_t)n, msg, off, len, dst,
                       (uint32_t)dl, static_cast<uint32_t*>(ring_rec), slot);
}

// the device's message ring (small wave calls): hits pinned, one slot reserved per distinct missing
// message and per ahead message that is neither cached nor a duplicate
void plan_msg_ring(nwv::BlsMsgRing& R, const CallIn& c, const Ahead* ahead, MsgSlots& ms, CallPlan& P) {
    const size_t n = c.n;
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
        P.mcount[2]++;
        if (c.msg_len[i] > nwv::MsgKey::MAX_MSG) continue;
        const nwv::MsgKey k = nwv::MsgKey::make(c.dst, c.dl, c.msg_base + c.msg_off[i], c.msg_len[i]);
        const uint32_t s = R.lookup_pin(k);
        if (s != nwv::BlsMsgRing::NONE) {
            hsrc[i] = s;
            ms.pinned.push_back(s);
            P.mcount[2]--;
            P.mcount[P.kside && P.kmode[i] ? 0 : 1]++;
            continue;
        }
        hpub[i] = take(k, UINT32_MAX, false);
    }
    AheadPack ap;
    for (size_t j = 0; ahead && j < ahead->n; j++) {
        if (ahead->len[j] > nwv::MsgKey::MAX_MSG) continue;
        const nwv::MsgKey k = nwv::MsgKey::make(c.dst, c.dl, ahead->base + ahead->off[j], ahead->len[j]);
        if (R.contains(k)) continue;
        const uint32_t r = take(k, ahead->gate ? ahead->gate[j] : UINT32_MAX, true);
        if (r != MR_NONE) ap.push(r, ahead->base + ahead->off[j], ahead->len[j]);
    }
    P.n_ah = ap.n();
    P.r_hsrc = 8 * P.n_ah;
    P.r_hpub = P.r_hsrc + 4 * n;
    P.r_aslot = P.r_hpub + 4 * n;
    P.r_alen = P.r_aslot + 4 * P.n_ah;
    P.r_amsg = P.r_alen + 4 * P.n_ah;
    P.rsec.assign(P.r_amsg + ap.msg.size() + 1, 0);
    uint8_t* r = P.rsec.data();
    ap.write(r, r + P.r_aslot, r + P.r_alen, r + P.r_amsg);
    std::memcpy(r + P.r_hsrc, hsrc.data(), 4 * n);
    std::memcpy(r + P.r_hpub, hpub.data(), 4 * n);
}

// the device's aggregate-key ring (small wave calls): the key-side items of 2 to 1,024 keys.  A hit
// is pinned and its item becomes a one-key item on the ring slot, in arrays of the call's own (made
// only when some item hit); a set missed for the second time reserves a slot for k_blsw_apk_fill
// (one item of the call per set)
void plan_apk_ring(nwv::BlsApkRing& R, const CallIn& c, ApkSlots& as, CallPlan& P) {
    const size_t n = c.n;
    std::vector<uint32_t> hit(n, nwv::BlsApkRing::NONE);
    for (size_t i = 0; i < n; i++) {
        if (!P.kmode[i] || !nwv::ApkKey::eligible(c.pk_cnt[i])) continue;
        nwv::ApkKey k = nwv::ApkKey::make(P.remap.data() + c.pk_off[i], c.pk_cnt[i]);
        const uint32_t s = R.lookup_pin(k);
        if (s != nwv::BlsApkRing::NONE) {
            hit[i] = s;
            as.pinned.push_back(s);
            P.acount[0]++;
            continue;
        }
        P.acount[1]++;
        bool mine = false;  // an earlier item of this call fills the set already
        for (const ApkSlots::Fresh& f : as.fresh) mine = mine || f.key == k;
        if (mine) continue;
        bool noted = false;
        const uint32_t r = R.miss(k, &noted);
        if (noted) P.acount[2]++;
        if (r != nwv::BlsApkRing::NONE) as.fresh.push_back({r, (uint32_t)i, std::move(k)});
    }
    if (P.acount[0]) {
        P.a_off.assign(c.pk_off, c.pk_off + n);
        P.a_cnt.assign(c.pk_cnt, c.pk_cnt + n);
        P.a_idx = P.remap;
        for (size_t i = 0; i < n; i++) {
            if (hit[i] == nwv::BlsApkRing::NONE) continue;
            P.a_off[i] = (uint32_t)P.a_idx.size();
            P.a_cnt[i] = 1;
            P.a_idx.push_back(AR_BASE + hit[i]);
        }
    }
    for (const ApkSlots::Fresh& f : as.fresh) P.a_fill.push_back(f.item);
    for (const ApkSlots::Fresh& f : as.fresh) P.a_fill.push_back(f.slot);
    P.n_fill = as.fresh.size();
}

// the whole plan.  It reserves and pins ring slots (S gives them back) and reads the key cache, so
// the caller holds its lane and the cache's shared lock
int plan_call(BlsDev& d, BlsLane& L, const CallIn& c, const Ahead* ahead, CallSlots& S, CallPlan& P) {
    const BlsEnv& env = bls_env();
    const size_t n = c.n;
    P.group_item = (d.flags & NWV_FLAG_BLS_PER_ITEM) != 0;
    P.batch = !P.group_item && (d.flags & NWV_FLAG_BLS_BATCH) != 0;
    P.wavem = !P.group_item && !P.batch;
    // wave-per-item hashing and G1 checks while the call has fewer items than the chip has SIMDs
    // (latency); above that, one item per lane keeps every lane busy (throughput)
    P.wave_small = P.wavem && n <= env.wave_max;
    // the wave batch check (one final exponentiation per group of wb_grp items): large wave calls
    // of at least nwv_bls_set_wave_batch_min items
    const size_t wb_min = d.wave_batch_min.load(std::memory_order_relaxed);
    P.wbatch = P.wavem && !P.wave_small && wb_min > 0 && n >= wb_min;
    P.wb_ng = P.wbatch ? (n + env.wb_grp - 1) / env.wb_grp : 0;
    P.wb_m = P.wbatch ? n + P.wb_ng : 0;
    // the dense key-sum stage (bls_apk_dense.h): large wave calls of at least
    // nwv_bls_set_apk_dense_min items; NWV_BLS_APK_LANES forces the lanes an item gets (4, 8, 16)
    const size_t ad_min = d.apk_dense_min.load(std::memory_order_relaxed);
    P.ad_run = P.wavem && !P.wave_small && ad_min > 0 && n >= ad_min;
    P.cached = !(d.flags & NWV_FLAG_NO_KEYCACHE) && d.kc.rec.p != nullptr;
    plan_keys(d.kc, c, P);
    // the key-transposed batch check (bls_key_batch.h): large wave calls of at least
    // nwv_bls_set_key_batch_min items (every item's keys cached is what the key side already asks)
    const size_t kb_min = d.key_batch_min.load(std::memory_order_relaxed);
    P.kb_cand = P.wavem && !P.wave_small && P.kside && kb_min > 0 && n >= kb_min;
    // (the dense stage reads the caller's key numbers and the key table itself: an ascending list is
    // ascending in those, not in cache slots)
    if (P.ad_run) nwv::apk_dense_split(n, P.kside ? P.kmode.data() : nullptr, c.pk_cnt, P.ads);
    P.ad_lanes = P.ad_run ? nwv::apk_dense_lanes(P.ads.dense.size(), env.ad_forced) : 0;
    // verified signatures stay decoded in the device's ring (BlsSigCache) for aggregates
    // (n <= 1,024 whatever NWV_BLS_WAVE_MAX says: the calls in flight on a device's lanes then hold
    // at most kMaxBusySlots busy slots)
    P.keep = P.wave_small && n <= 1024 && !(d.flags & NWV_FLAG_NO_SIGCACHE);
    if (P.keep) {
        int rc = d.sc.reserve(n, S.kept.slots);
        if (rc) return rc;
        S.kept.sc = &d.sc;
        S.kept.n = n;
    }
    P.use_ring = P.wave_small && n <= 1024 && d.mr.on.load(std::memory_order_acquire) && c.dl <= nwv::MsgKey::MAX_DST;
    if (P.use_ring) {
        S.ms.ring = &d.mr.ring;
        S.ms.streams[0] = L.stream;
        S.ms.streams[1] = L.side[0];
        plan_msg_ring(d.mr.ring, c, ahead, S.ms, P);
    }
    P.use_apk = P.wave_small && n <= 1024 && P.kside && d.ar.on.load(std::memory_order_acquire);
    if (P.use_apk) {
        S.as.ring = &d.ar.ring;
        S.as.streams[0] = L.stream;
        S.as.streams[1] = L.side[0];
        plan_apk_ring(d.ar.ring, c, S.as, P);
    }
    const bool a_hit = !P.a_idx.empty();
    P.k_off = a_hit ? P.a_off.data() : c.pk_off;
    P.k_cnt = a_hit ? P.a_cnt.data() : c.pk_cnt;
    P.k_idx = a_hit ? &P.a_idx : &P.remap;
    // the per-stage timing events of a small call only on a NWV_FLAG_BLS_STAGE_TIMES context: else
    // just the two that order the streams (the others cost a single verification ~0.1 ms:
    // 2.85 -> 2.72-2.81 ms, profiles/round6_bls_stage_timing_ab.json)
    P.no_timing = !(d.flags & NWV_FLAG_BLS_STAGE_TIMES);
    return NWV_OK;
}

// the call's typed buffers: the arena's sections on the device (the host side is filled from the
// arena's parts), the scratch sections, the pinned words behind the arena
struct CallBufs {
    size_t n = 0, dl = 0;
    // arena (device side)
    const uint8_t *keys, *sigs, *msg, *dst, *seed, *amsg;
    const uint32_t *kslot, *off, *cnt, *idx, *mlen, *km, *scs, *hsrc, *hpub, *aslot, *alen, *fill_item, *fill_slot,
        *dlist, *rlist, *idx0, *ktab;
    const uint64_t *moff, *aoff;
    // scratch: item sig / H / apk records, the status arrays, the group batch check's shares
    // (W-order Fp12 + Jacobian G1 per item) and its verdict word, the wave engine's records
    uint32_t *srec, *hrec, *arec, *frec, *jrec, *prec, *hh, *ajrec;
    int32_t *st, *ssig, *sapk, *okw, *sdec, *ssub, *spair;
    // the wave batch check's scratch: F records, [r] H, [r] sig, the groups' S_g, in-batch flags,
    // the groups' verdict words
    uint32_t *wf, *wp, *wj, *wsg, *winb;
    int32_t* wgok;
    // the dense key sums' scratch: the key table's total and flag, the items' modes
    uint32_t *dtot, *dmode;
    KeyTab kt;
    // pinned, behind the arena: the batch verdict word, the wave batch check's group verdicts, the
    // dense key sums' per-item modes
    int32_t *h_ok, *h_gok;
    uint32_t* h_dmode;
};

hipError_t trec(const CallPlan& P, BlsLane& L, int k, hipStream_t s) {
    return P.no_timing ? hipSuccess : hipEventRecord(L.ev[k], s);
}
// the call's keys the cache does not hold, decoded into the scratch table
void launch_keys_fill(hipStream_t s, const CallPlan& P, const CallBufs& B) {
    if (P.n_dec())
        hipLaunchKernelGGL(k_bls_keys_fill, dim3(kBlocks(P.n_dec())), dim3(BLS_LANES), 0, s, (uint32_t)P.n_dec(),
                           B.keys, B.kslot, const_cast<uint32_t*>(B.kt.rs), const_cast<int32_t*>(B.kt.ss));
}
// the tail of every path: the statuses to the caller (with one more copy, when given), the stream
// synchronised
int copy_back(hipStream_t s, const CallBufs& B, int32_t* status, void* xdst = nullptr, const void* xsrc = nullptr,
              size_t xbytes = 0) {
    BLS_HIP(hipGetLastError());
    BLS_HIP(hipMemcpyAsync(status, B.st, 4 * B.n, hipMemcpyDeviceToHost, s));
    if (xbytes) BLS_HIP(hipMemcpyAsync(xdst, xsrc, xbytes, hipMemcpyDeviceToHost, s));
    BLS_HIP(hipStreamSynchronize(s));
    return NWV_OK;
}
// the wave paths' tail: the statuses in the oracle's order first (sc_rec: the verified records
// into the ring slots this call reserved)
int wave_status_back(hipStream_t s, const CallBufs& B, int32_t* status, void* sc_rec, void* xdst = nullptr,
                     const void* xsrc = nullptr, size_t xbytes = 0) {
    hipLaunchKernelGGL(k_blsw_status, dim3(kBlocks(B.n)), dim3(BLS_LANES), 0, s, (uint32_t)B.n, B.sdec, B.ssub,
                       B.sapk, B.spair, B.st, B.srec, static_cast<uint32_t*>(sc_rec), sc_rec ? B.scs : nullptr);
    return copy_back(s, B, status, xdst, xsrc, xbytes);
}

// The small wave call (path 3): a call of up to wave_max items on two streams (8 concurrent calls
// then fit 16 hardware queues one to one): side 0 decodes the keys the cache does not hold, then
// hashes to G1 and sums the keys in one launch (k_blsw_pre); main decodes the signatures, then runs
// the pairing checks and the signatures' G1 checks in one launch (k_blsw_pair_sub)
int run_small(BlsDev& d, BlsLane& L, CallPlan& P, const CallBufs& B, const CallIn& c, int32_t* status,
              CallSlots& S, uint64_t* mstat, uint64_t* astat, CallStats& T) {
    const size_t n = c.n;
    const hipStream_t s0 = L.stream, s1 = L.side[0];
    T.untimed = P.no_timing;
    T.path = 3;
    BLS_HIP(trec(P, L, 0, s1));
    launch_keys_fill(s1, P, B);
    BLS_HIP(trec(P, L, 1, s1));
    BLS_HIP(trec(P, L, 5, s1));
    if (P.use_ring)
        hipLaunchKernelGGL(k_blsw_pre_r, dim3((unsigned)(2 * n)), dim3(64), 0, s1, (uint32_t)n, B.msg, B.moff, B.mlen,
                           B.dst, (uint32_t)B.dl, B.hh, B.kt, B.off, B.cnt, B.idx, B.km, B.ajrec, B.sapk,
                           static_cast<uint32_t*>(d.mr.rec.p), B.hsrc, B.hpub);
    else
        hipLaunchKernelGGL(k_blsw_pre, dim3((unsigned)(2 * n)), dim3(64), 0, s1, (uint32_t)n, B.msg, B.moff, B.mlen,
                           B.dst, (uint32_t)B.dl, B.hh, B.kt, B.off, B.cnt, B.idx, B.km, B.ajrec, B.sapk);
    if (P.n_fill) BLS_HIP(hipEventRecord(L.sev[2], s1));
    BLS_HIP(trec(P, L, 2, s1));
    BLS_HIP(trec(P, L, 6, s1));
    BLS_HIP(trec(P, L, 3, s0));
    hipLaunchKernelGGL(k_blsw_sigdec, dim3(kBlocks(n)), dim3(BLS_LANES), 0, s0, (uint32_t)n, B.sigs, B.srec, B.sdec);
    BLS_HIP(trec(P, L, 4, s0));
    BLS_HIP(hipEventRecord(L.sev[1], s0));
    // the ahead messages on the main stream, idle from here on: the pairing, on side 0, does
    // not wait for them
    if (P.n_ah) launch_ahead(s0, P.n_ah, B.amsg, B.aoff, B.alen, B.dst, B.dl, d.mr.rec.p, B.aslot);
    // the aggregate-key fills on the main stream too, behind the key sums: they run beside the
    // pairing kernel, which reads the sums and never the slots being filled
    if (P.n_fill) {
        BLS_HIP(hipStreamWaitEvent(s0, L.sev[2], 0));
        hipLaunchKernelGGL(k_blsw_apk_fill, dim3((unsigned)P.n_fill), dim3(64), 0, s0, (uint32_t)P.n_fill, B.fill_item,
                           B.fill_slot, B.ajrec, B.sapk, static_cast<uint32_t*>(d.ar.rec.p),
                           static_cast<uint32_t*>(d.ar.lines.p));
    }
    S.kept.stream = s1;  // k_blsw_status writes the ring slots there
    // the rest runs on side 0 behind the hash, which ends after the signatures' decode (one
    // lane each, ~0.45 ms against ~0.57 ms): its wait on the decode is already met, so the
    // cross-queue hand-off (~25 us in the single-verify trace) is off the critical path
    BLS_HIP(hipStreamWaitEvent(s1, L.sev[1], 0));
    BLS_HIP(trec(P, L, 7, s1));
    hipLaunchKernelGGL(k_blsw_pair_sub, dim3((unsigned)(2 * n)), dim3(64), 0, s1, (uint32_t)n, B.srec, B.sdec, B.hh, 1,
                       B.ajrec, B.sapk, B.kt, B.off, B.cnt, B.idx, B.km, B.spair, B.ssub);
    BLS_HIP(trec(P, L, 8, s1));
    int rc = wave_status_back(s1, B, status, P.keep ? d.sc.rec.p : nullptr);
    if (rc) return rc;
    if (P.n_ah || P.n_fill) BLS_HIP(hipStreamSynchronize(s0));
    if (P.keep) {
        d.sc.publish(n, c.sigs, status, S.kept.slots);
        S.kept.sc = nullptr;
    }
    // H(m) is a function of dst and message alone: a miss is published whatever its item's
    // status; an ahead message only behind its gate
    S.ms.finish(status, P.mcount);
    if (mstat)
        for (int k = 0; k < 5; k++) mstat[k] += P.mcount[k];
    // a set is a function of the key cache's slots alone, but it is kept only behind a verified
    // aggregate: peers cannot churn the ring without valid certificates
    S.as.finish(status, P.acount);
    if (astat)
        for (int k = 0; k < 4; k++) astat[k] += P.acount[k];
    return NWV_OK;
}

// the large calls' prologue: side 0 decodes the keys the cache does not hold and sums every item's
// keys, side 1 hashes every item's message to G1 (the statuses are not known yet); ev[10] and
// ev[11] mark their ends
int large_sides(BlsLane& L, const CallPlan& P, const CallBufs& B, const CallIn& c) {
    const size_t n = c.n, n_dn = P.ads.dense.size(), n_rest = P.ads.rest.size();
    if (!L.side[1] && nwv::lane_stream_create(&L.side[1], L.high) != hipSuccess)
        return nwv_internal_set_err(NWV_ERR_HIP, "bls stream");
    const hipStream_t s1 = L.side[0], s2 = L.side[1];
    BLS_HIP(hipStreamWaitEvent(s2, L.sev[0], 0));
    BLS_HIP(hipEventRecord(L.ev[0], s1));
    launch_keys_fill(s1, P, B);
    BLS_HIP(hipEventRecord(L.ev[1], s1));
    if (P.wavem && n_dn) {
        // the dense stage: the key table's total, the dense items L lanes each, then the items
        // left to the per-item code through their list (all three write disjoint records)
        const DenseKeys dk{B.kt.hrc, B.kt.sc, B.ktab, (uint32_t)c.n_keys, KC_CAP};
        hipLaunchKernelGGL(k_blsd_total, dim3(1), dim3(64), 0, s1, dk, B.dtot);
        const unsigned per = 64 / P.ad_lanes, blocks = (unsigned)((n_dn + per - 1) / per);
        auto* kern = P.ad_lanes == 16 ? k_blsd_apk<16> : P.ad_lanes == 8 ? k_blsd_apk<8> : k_blsd_apk<4>;
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), 0, s1, (uint32_t)n_dn, B.dlist, dk, B.off, B.cnt, B.idx0,
                           B.dtot, B.ajrec, B.sapk, B.dmode);
        if (n_rest)
            hipLaunchKernelGGL(k_blsw_apk_list, dim3((unsigned)n_rest), dim3(64), 0, s1, (uint32_t)n_rest, B.rlist,
                               B.kt, B.off, B.cnt, B.idx, B.km, B.ajrec, B.sapk);
    } else if (P.wavem)
        hipLaunchKernelGGL(k_blsw_apk, dim3((unsigned)n), dim3(64), 0, s1, (uint32_t)n, B.kt, B.off, B.cnt, B.idx, B.km,
                           B.ajrec, B.sapk);
    else
        hipLaunchKernelGGL(k_bls_apk_g, dim3(gBlocks(n)), dim3(BLS_LANES), 0, s1, (uint32_t)n, B.kt, B.off, B.cnt, B.idx,
                           B.arec, B.sapk);
    BLS_HIP(hipEventRecord(L.ev[2], s1));
    BLS_HIP(hipEventRecord(L.ev[10], s1));
    BLS_HIP(hipEventRecord(L.ev[5], s2));
    // hash to G1 on lane pairs
    hipLaunchKernelGGL(k_bls_h2c_2, dim3((unsigned)((n + BLS_LANES / 2 - 1) / (BLS_LANES / 2))), dim3(BLS_LANES), 0, s2,
                       (uint32_t)n, B.msg, B.moff, B.mlen, B.dst, (uint32_t)B.dl, B.hrec, B.km);
    BLS_HIP(hipEventRecord(L.ev[6], s2));
    BLS_HIP(hipEventRecord(L.ev[11], s2));
    return NWV_OK;
}

// LDS bytes of a packed pairing wave (k_blsw_pair_k, k_blsw_mill_k)
size_t pack_lds(const BlsEnv& env) {
    return (size_t)4 * (wave::KP_WORDS + env.pack * wave::SW * wave::NSLOTS_PC) + env.lds_pad;
}
// the per-item pairing checks of items [lo, lo + m): every item's own final exponentiation
void pair_per_item(hipStream_t s0, const CallBufs& B, size_t lo, size_t m) {
    const BlsEnv& env = bls_env();
    if (env.pack > 1)
        hipLaunchKernelGGL(k_blsw_pair_k, dim3((unsigned)((m + env.pack - 1) / env.pack)), dim3(64), pack_lds(env), s0,
                           (uint32_t)m, env.pack, B.srec + G1_REC_WORDS * lo, B.sdec + lo, B.hrec + G1_REC_WORDS * lo, 0,
                           B.ajrec + G2J_WORDS * lo, B.sapk + lo, B.kt, B.off + lo, B.cnt + lo, B.idx,
                           B.km ? B.km + lo : nullptr, B.spair + lo);
    else
        hipLaunchKernelGGL(k_blsw_pair, dim3((unsigned)m), dim3(64), env.lds_pad, s0, (uint32_t)m,
                           B.srec + G1_REC_WORDS * lo, B.sdec + lo, B.hrec + G1_REC_WORDS * lo, 0,
                           B.ajrec + G2J_WORDS * lo, B.sapk + lo, B.kt, B.off + lo, B.cnt + lo, B.idx,
                           B.km ? B.km + lo : nullptr, B.spair + lo);
}
// The per-item launches behind a batch check's rejected groups (need[i] != 0).  A launch over a few
// items costs one item's whole chain (~3 ms) however few they are, so marked items less than
// RECHECK_GAP items apart share a launch with the accepted items between them (~1 us an item
// there).  Returns the items the launches covered.
constexpr size_t RECHECK_GAP = 1024;
template <class Fn>
void pair_recheck(hipStream_t s0, const CallBufs& B, const std::vector<uint8_t>& need, Fn per_range) {
    for (const auto& r : nwv::recheck_ranges(B.n, need.data(), RECHECK_GAP)) {
        pair_per_item(s0, B, r.first, r.second - r.first);
        per_range(r.first, r.second);
    }
}

// The key-transposed check (paths 6 and 7).  *done = false when its plan does not run: the call
// then takes the stage it takes with the setting off.
int pair_key_batch(BlsDev& d, BlsLane& L, const CallPlan& P, const CallBufs& B, const CallIn& c, CallStats& T,
                   bool* done) {
    const BlsEnv& env = bls_env();
    const size_t n = c.n;
    const hipStream_t s0 = L.stream;
    int rc;
    *done = false;
    // the pre-pairing statuses come back first: the plan groups the items they leave
    if ((rc = L.kb_st.ensure(12 * n + 64))) return rc;
    int32_t* h_dec = static_cast<int32_t*>(L.kb_st.p);
    int32_t *h_apk = h_dec + n, *h_gok = h_apk + n;
    BLS_HIP(hipMemcpyAsync(h_dec, B.sdec, 4 * n, hipMemcpyDeviceToHost, s0));
    BLS_HIP(hipMemcpyAsync(h_apk, B.sapk, 4 * n, hipMemcpyDeviceToHost, s0));
    BLS_HIP(hipStreamSynchronize(s0));
    std::vector<uint8_t> ok(n), el(n);
    for (size_t i = 0; i < n; i++) {
        ok[i] = h_dec[i] == ST_OK && h_apk[i] == ST_OK;
        // (a compressed identity has bit 6 of its first byte set; the kernels check again)
        el[i] = ok[i] && P.kmode[i] && !(c.sigs[48 * i] & 0x40);
    }
    nwv::KeyBatchPlan K;
    nwv::key_batch_plan(n, ok.data(), el.data(), c.pk_off, c.pk_cnt, P.remap.data(), d.kc.used, env.kb_grp,
                        env.kb_ratio, K);
    if (!K.run) return NWV_OK;
    const size_t ne = K.items.size(), ng = K.groups(), M = K.entries(), C = K.cidx.size(), KM = M + ng;
    // the plan's lists, one copy: items | goff | eslot | egrp | coff | cidx | 0..M-1 | ones
    Layout u;
    const auto u_items = u.packed<uint32_t>(4 * ne), u_goff = u.packed<uint32_t>(4 * (ng + 1)),
               u_eslot = u.packed<uint32_t>(4 * M), u_egrp = u.packed<uint32_t>(4 * M),
               u_coff = u.packed<uint32_t>(4 * (M + 1)), u_cidx = u.packed<uint32_t>(4 * C),
               u_iota = u.packed<uint32_t>(4 * M), u_ones = u.packed<uint32_t>(4 * M);
    if ((rc = L.kb_up.ensure(u.end)) || (rc = L.kb_in.ensure(u.end))) return rc;
    void* up = L.kb_up.p;
    std::memcpy(u_items.at(up), K.items.data(), 4 * ne);
    std::memcpy(u_goff.at(up), K.goff.data(), 4 * (ng + 1));
    std::memcpy(u_eslot.at(up), K.eslot.data(), 4 * M);
    std::memcpy(u_egrp.at(up), K.egrp.data(), 4 * M);
    std::memcpy(u_coff.at(up), K.coff.data(), 4 * (M + 1));
    std::memcpy(u_cidx.at(up), K.cidx.data(), 4 * C);
    for (size_t m = 0; m < M; m++) {
        u_iota.at(up)[m] = (uint32_t)m;
        u_ones.at(up)[m] = 1u;
    }
    void* ki = L.kb_in.p;
    BLS_HIP(hipMemcpyAsync(ki, up, u.end, hipMemcpyHostToDevice, s0));
    const uint32_t *items = u_items.at(ki), *eslot = u_eslot.at(ki), *ones = u_ones.at(ki);
    // the check's records: [r] H and [r] sig per position, S_g per group, the Miller
    // entries' hash sides, Qs and F records, the groups' poison and verdict words
    Layout k;
    const auto k_hj = k.aligned<uint32_t>(4 * G1J_REC_WORDS * ne), k_sj = k.aligned<uint32_t>(4 * G1J_REC_WORDS * ne),
               k_sg = k.aligned<uint32_t>(4 * G1_REC_WORDS * ng), k_p = k.aligned<uint32_t>(4 * G1H_REC_WORDS * KM),
               k_q = k.aligned<uint32_t>(4 * G2J_WORDS * KM), k_f = k.aligned<uint32_t>(4 * FB_REC_WORDS * KM),
               k_poi = k.aligned<uint32_t>(4 * ng);
    const auto k_gok = k.packed<int32_t>(4 * ng + 4);
    if ((rc = L.kb_work.ensure(k.end))) return rc;
    void* kw = L.kb_work.p;
    uint32_t *khj = k_hj.at(kw), *ksj = k_sj.at(kw), *ksg = k_sg.at(kw), *kp = k_p.at(kw), *kq = k_q.at(kw),
             *kf = k_f.at(kw), *kpoi = k_poi.at(kw);
    int32_t* kgok = k_gok.at(kw);
    const uint32_t G = env.kb_grp, gmax = (uint32_t)std::min<size_t>(G, ne);
    uint32_t kmax = 0;
    for (size_t g = 0; g < ng; g++) kmax = std::max(kmax, K.goff[g + 1] - K.goff[g]);
    BLS_HIP(hipMemsetAsync(kpoi, 0, 8 * ng, s0));  // no poison; a group whose tree does not finish stays rejected
    hipLaunchKernelGGL(k_blsk_rlc_pts, dim3(kBlocks(2 * ne)), dim3(BLS_LANES), 0, s0, (uint32_t)ne, G, items, B.srec,
                       B.hrec, B.sdec, B.sapk, B.seed, khj, ksj, kpoi);
    for (uint32_t m = gmax; m > 1; m = (m + 1) / 2)
        hipLaunchKernelGGL(k_blsw_sfold, dim3(kBlocks(ng * ((m + 1) / 2))), dim3(BLS_LANES), 0, s0, (uint32_t)ne, G,
                           (uint32_t)ng, m, ksj);
    hipLaunchKernelGGL(k_blsk_key_sums, dim3((unsigned)M), dim3(64), 0, s0, (uint32_t)M, u_coff.at(ki), u_cidx.at(ki),
                       eslot, u_egrp.at(ki), khj, B.kt, kp, kq, kpoi);
    hipLaunchKernelGGL(k_blsk_sig_items, dim3(kBlocks(ng)), dim3(BLS_LANES), 0, s0, (uint32_t)ng, G, (uint32_t)M, ksj,
                       ksg, kp, kq);
    // every key entry as a one-key key-side item of its own: key list entry m = slot eslot[m]
    const MillArgs ma{(uint32_t)M, ksg, ones, kf};
    hipLaunchKernelGGL(k_blsw_mill_k, dim3((unsigned)((KM + env.pack - 1) / env.pack)), dim3(64), pack_lds(env), s0,
                       (uint32_t)KM, env.pack, ma, kp, kq, B.kt, u_iota.at(ki), ones, eslot, ones);
    for (uint32_t s = 1;; s *= WB_FAN) {
        const uint32_t ents = (kmax + 1 + s - 1) / s, wpg = (ents + WB_FAN - 1) / WB_FAN;
        hipLaunchKernelGGL(k_blsk_ffold, dim3((unsigned)(ng * wpg)), dim3(64), 0, s0, (uint32_t)ng, u_goff.at(ki),
                           (uint32_t)M, wpg, s, wpg == 1 ? 1 : 0, kf, kpoi, kgok);
        if (wpg == 1) break;
    }
    hipLaunchKernelGGL(k_blsk_mark, dim3(kBlocks(ne)), dim3(BLS_LANES), 0, s0, (uint32_t)ne, G, items, kgok, B.spair);
    BLS_HIP(hipGetLastError());
    BLS_HIP(hipMemcpyAsync(h_gok, kgok, 4 * ng, hipMemcpyDeviceToHost, s0));
    BLS_HIP(hipStreamSynchronize(s0));
    // per item: the OK items outside the groups and every rejected group's items
    std::vector<uint8_t> need(n, 0), ing(n, 0);
    for (uint32_t i : K.outside) need[i] = 1;
    for (uint32_t i : K.items) ing[i] = 1;
    for (size_t g = 0; g < ng; g++) {
        if (h_gok[g] == 1) continue;
        T.kb[1]++;
        for (uint32_t p = K.gfirst[g]; p < K.gfirst[g + 1]; p++) need[K.items[p]] = 1;
    }
    pair_recheck(s0, B, need, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) T.kb[2] += ing[i];
    });
    T.kb[0] = ng;
    T.kb[3] = KM;
    T.kb[4] = ne;
    T.path = T.kb[1] ? 7 : 6;
    *done = true;
    return NWV_OK;
}

// The wave batch check (paths 4 and 5): one final exponentiation per group of wb_grp items, then
// every rejected group's items per item
int pair_wave_batch(BlsLane& L, const CallPlan& P, const CallBufs& B, CallStats& T) {
    const BlsEnv& env = bls_env();
    const size_t n = B.n;
    const hipStream_t s0 = L.stream;
    const uint32_t G = (uint32_t)env.wb_grp, ng = (uint32_t)P.wb_ng, gmax = (uint32_t)std::min<size_t>(env.wb_grp, n);
    BLS_HIP(hipMemsetAsync(B.wgok, 0, 4 * P.wb_ng, s0));  // a group whose tree does not finish stays rejected
    hipLaunchKernelGGL(k_blsw_rlc_pts, dim3(kBlocks(2 * n)), dim3(BLS_LANES), 0, s0, (uint32_t)n, B.srec, B.hrec, B.sdec,
                       B.sapk, B.km, B.seed, B.wp, B.wj, B.winb, B.spair);
    for (uint32_t m = gmax; m > 1; m = (m + 1) / 2)
        hipLaunchKernelGGL(k_blsw_sfold, dim3(kBlocks((size_t)ng * ((m + 1) / 2))), dim3(BLS_LANES), 0, s0, (uint32_t)n,
                           G, ng, m, B.wj);
    hipLaunchKernelGGL(k_blsw_sig_items, dim3(kBlocks(ng)), dim3(BLS_LANES), 0, s0, (uint32_t)n, G, ng, B.wj, B.wsg,
                       B.wp, B.ajrec);
    const MillArgs ma{(uint32_t)n, B.wsg, B.winb, B.wf};
    hipLaunchKernelGGL(k_blsw_mill_k, dim3((unsigned)((P.wb_m + env.pack - 1) / env.pack)), dim3(64), pack_lds(env), s0,
                       (uint32_t)P.wb_m, env.pack, ma, B.wp, B.ajrec, B.kt, B.off, B.cnt, B.idx, B.km);
    for (uint32_t s = 1;; s *= WB_FAN) {
        const uint32_t ents = (gmax + 1 + s - 1) / s, wpg = (ents + WB_FAN - 1) / WB_FAN;
        hipLaunchKernelGGL(k_blsw_ffold, dim3(ng * wpg), dim3(64), 0, s0, (uint32_t)n, G, wpg, s, wpg == 1 ? 1 : 0,
                           B.wf, B.wgok);
        if (wpg == 1) break;
    }
    hipLaunchKernelGGL(k_blsw_mark, dim3(kBlocks(n)), dim3(BLS_LANES), 0, s0, (uint32_t)n, G, B.wgok, B.winb, B.spair);
    BLS_HIP(hipGetLastError());
    BLS_HIP(hipMemcpyAsync(B.h_gok, B.wgok, 4 * P.wb_ng, hipMemcpyDeviceToHost, s0));
    BLS_HIP(hipStreamSynchronize(s0));
    std::vector<uint8_t> need(n, 0);
    T.wb[0] = P.wb_ng;
    for (size_t g = 0; g < P.wb_ng; g++) {
        if (B.h_gok[g] == 1) continue;
        T.wb[1]++;
        std::fill(need.begin() + g * env.wb_grp, need.begin() + std::min(n, (g + 1) * env.wb_grp), 1);
    }
    pair_recheck(s0, B, need, [&](size_t lo, size_t hi) { T.wb[2] += hi - lo; });
    T.path = T.wb[1] ? 5 : 4;
    return NWV_OK;
}

// The large wave call: the one-lane-per-item decode + G1 check of the group path, which keeps every
// lane busy (an all-Ok subgroup column), then every item's pairing check on a wave by one of three
// stages: the key-transposed check, the wave batch check, or per item (path 3)
int run_large_wave(BlsDev& d, BlsLane& L, const CallPlan& P, const CallBufs& B, const CallIn& c, int32_t* status,
                   CallStats& T) {
    const size_t n = c.n, n_dn = P.ads.dense.size();
    const hipStream_t s0 = L.stream;
    int rc = large_sides(L, P, B, c);
    if (rc) return rc;
    BLS_HIP(hipEventRecord(L.ev[3], s0));
    hipLaunchKernelGGL(k_bls_sigs, dim3(kBlocks(n)), dim3(BLS_LANES), 0, s0, (uint32_t)n, B.sigs, B.srec, B.sdec);
    BLS_HIP(hipMemsetAsync(B.ssub, 0, 4 * n, s0));
    BLS_HIP(hipEventRecord(L.ev[4], s0));
    BLS_HIP(hipStreamWaitEvent(s0, L.ev[10], 0));
    BLS_HIP(hipStreamWaitEvent(s0, L.ev[11], 0));
    BLS_HIP(hipEventRecord(L.ev[7], s0));
    if ((bls_env().pack > 1 || P.wbatch || P.kb_cand) && ensure_pair_script()) return NWV_ERR_HIP;
    T.path = 3;
    bool kb_done = false;
    if (P.kb_cand && (rc = pair_key_batch(d, L, P, B, c, T, &kb_done))) return rc;
    if (!kb_done && P.wbatch) {
        if ((rc = pair_wave_batch(L, P, B, T))) return rc;
    } else if (!kb_done) {
        pair_per_item(s0, B, 0, n);
    }
    BLS_HIP(hipEventRecord(L.ev[8], s0));
    if ((rc = wave_status_back(s0, B, status, nullptr, B.h_dmode, B.dmode, 4 * n_dn))) return rc;
    if (P.ad_run) {
        for (size_t q = 0; q < n_dn; q++) T.ad[B.h_dmode[q] ? 1 : 0]++;
        T.ad[2] = P.ads.rest.size();
        T.ad[3] = P.ad_lanes;
    }
    return NWV_OK;
}

// The group engines (8 lanes an item): per item (path 0), or one batch check over the call (path 1)
// and per item only when that rejects (path 2)
int run_group(BlsLane& L, const CallPlan& P, const CallBufs& B, const CallIn& c, int32_t* status, CallStats& T) {
    const size_t n = c.n;
    const hipStream_t s0 = L.stream;
    int rc = large_sides(L, P, B, c);
    if (rc) return rc;
    // main: signatures, then the join
    BLS_HIP(hipEventRecord(L.ev[3], s0));
    hipLaunchKernelGGL(k_bls_sigs, dim3(kBlocks(n)), dim3(BLS_LANES), 0, s0, (uint32_t)n, B.sigs, B.srec, B.ssig);
    BLS_HIP(hipEventRecord(L.ev[4], s0));
    BLS_HIP(hipStreamWaitEvent(s0, L.ev[10], 0));
    BLS_HIP(hipStreamWaitEvent(s0, L.ev[11], 0));
    hipLaunchKernelGGL(k_bls_status, dim3(kBlocks(n)), dim3(BLS_LANES), 0, s0, (uint32_t)n, B.ssig, B.sapk, B.st);
    BLS_HIP(hipEventRecord(L.ev[7], s0));
    auto per_item = [&]() {
        hipLaunchKernelGGL(k_bls_pair, dim3(gBlocks(n)), dim3(BLS_LANES), 0, s0, (uint32_t)n, B.srec, B.hrec, B.arec,
                           B.st);
    };
    if (P.batch) {
        hipLaunchKernelGGL(k_bls_rlc_pts, dim3(gBlocks(n)), dim3(BLS_LANES), 0, s0, (uint32_t)n, B.srec, B.hrec, B.st,
                           B.seed, B.prec, B.jrec);
        for (uint32_t m = (uint32_t)n; m > 1; m = (m + 1) / 2)
            hipLaunchKernelGGL(k_bls_sfold, dim3(kBlocks(m / 2)), dim3(BLS_LANES), 0, s0, m, B.jrec);
        hipLaunchKernelGGL(k_bls_sig_item, dim3(1), dim3(BLS_LANES), 0, s0, (uint32_t)n, B.jrec, B.prec, B.arec);
        hipLaunchKernelGGL(k_bls_rlc_ml, dim3(gBlocks(n + 1)), dim3(BLS_LANES), 0, s0, (uint32_t)(n + 1), B.prec, B.arec,
                           B.frec);
        for (uint32_t m = (uint32_t)n + 1; m > 1; m = (m + 1) / 2)
            hipLaunchKernelGGL(k_bls_ffold, dim3(gBlocks(m / 2)), dim3(BLS_LANES), 0, s0, m, B.frec);
        hipLaunchKernelGGL(k_bls_final, dim3(1), dim3(BLS_LANES), 0, s0, B.frec, B.okw);
        BLS_HIP(hipMemcpyAsync(B.h_ok, B.okw, 4, hipMemcpyDeviceToHost, s0));
        BLS_HIP(hipStreamSynchronize(s0));
        BLS_HIP(hipGetLastError());
        T.path = *B.h_ok == 1 ? 1 : 2;
        if (*B.h_ok != 1) per_item();  // the batch check rejected: name the failing items exactly
    } else {
        per_item();
        T.path = 0;
    }
    BLS_HIP(hipEventRecord(L.ev[8], s0));
    return copy_back(s0, B, status);
}

// stage times of the completed call, its path and key counts -> the device's "last call"
int record_last(BlsDev& d, BlsLane& L, const CallPlan& P, const CallStats& T) {
    const int pairs[5][2] = {{0, 1}, {3, 4}, {5, 6}, {1, 2}, {7, 8}};  // keys, sigs, h2c, apk, pairing
    double ms5[5] = {0, 0, 0, 0, 0};
    for (int k = 0; k < 5 && !T.untimed; k++) {
        float ms = 0;
        BLS_HIP(hipEventElapsedTime(&ms, L.ev[pairs[k][0]], L.ev[pairs[k][1]]));
        ms5[k] = ms;
    }
    std::lock_guard<std::mutex> g(d.stat_mu);
    std::memcpy(d.last_ms, ms5, sizeof ms5);
    d.last_path = T.path;
    d.last_keys[0] = P.hits;
    d.last_keys[1] = P.n_dec();
    std::memcpy(d.last_batch, T.wb, sizeof T.wb);
    std::memcpy(d.last_kbatch, T.kb, sizeof T.kb);
    std::memcpy(d.last_apkd, T.ad, sizeof T.ad);
    return NWV_OK;
}

// nwv_bls_verify_many on one lane of a device: lease, plan, buffers, one H2D copy, the path's
// function, the bookkeeping
int verify_on(BlsDev& d, const CallIn& c, int32_t* status, const Ahead* ahead = nullptr, uint64_t* mstat = nullptr,
              uint64_t* astat = nullptr, bool latency = false) {
    // (declaration order is a condition, see CallSlots: destroyed in reverse, the ring slots go
    // back before the key-cache lock drops and before the lane returns to the pool)
    LaneLease lane(d, latency);
    if (lane.rc()) return lane.rc();
    BlsLane& L = *lane;
    std::shared_lock<std::shared_mutex> kc_hold(d.kc.mu);  // records stay put while our kernels read them
    CallSlots S;
    CallPlan P;
    int rc = plan_call(d, L, c, ahead, S, P);
    if (rc) return rc;
    static const uint8_t zero[8] = {0};
    const size_t n = c.n, n_dec = P.n_dec(), nk_idx = P.k_idx->size(), n_dn = P.ads.dense.size(),
                 n_rest = P.ads.rest.size();
    uint8_t seed[32];
    nwv_internal_fill_seed(nullptr, seed);  // the batch coefficients' key: OS entropy per call
    Arena a;
    const auto o_keys = a.add<uint8_t>(n_dec ? (const void*)P.fill_keys.data() : zero, 96 * n_dec + 8);
    const auto o_kslot = a.add<uint32_t>(n_dec ? (const void*)P.fill_slot.data() : zero, 4 * n_dec + 4);
    const auto o_sigs = a.add<uint8_t>(c.sigs, 48 * n);
    const auto o_off = a.add<uint32_t>(P.k_off, 4 * n), o_cnt = a.add<uint32_t>(P.k_cnt, 4 * n),
               o_idx = a.add<uint32_t>(nk_idx ? (const void*)P.k_idx->data() : zero, 4 * nk_idx + 4);
    const auto o_msg = a.add<uint8_t>(c.msg_bytes ? (const void*)c.msg_base : zero, c.msg_bytes + 1);
    const auto o_moff = a.add<uint64_t>(c.msg_off, 8 * n);
    const auto o_mlen = a.add<uint32_t>(c.msg_len, 4 * n);
    const auto o_dst = a.add<uint8_t>(c.dst, c.dl), o_seed = a.add<uint8_t>(seed, 32);
    const auto o_kmode = a.add<uint32_t>(P.kside ? (const void*)P.kmode.data() : zero, 4 * P.kmode.size() + 4),
               o_scs = a.add<uint32_t>(P.keep ? (const void*)S.kept.slots.data() : zero, 4 * S.kept.slots.size() + 4);
    // (one section for everything the ring adds: a single verification still fits stage_h2d's arguments)
    const auto o_ring = P.use_ring ? a.add<uint8_t>(P.rsec.data(), P.rsec.size()) : Sec<const uint8_t>{};
    const auto o_fill = P.n_fill ? a.add<uint32_t>(P.a_fill.data(), 8 * P.n_fill) : Sec<const uint32_t>{};
    const auto o_dlist = n_dn ? a.add<uint32_t>(P.ads.dense.data(), 4 * n_dn) : Sec<const uint32_t>{},
               o_rlist = n_dn && n_rest ? a.add<uint32_t>(P.ads.rest.data(), 4 * n_rest) : Sec<const uint32_t>{},
               o_idx0 = n_dn ? a.add<uint32_t>(c.pk_idx, 4 * c.n_idx) : Sec<const uint32_t>{},
               o_ktab = n_dn ? a.add<uint32_t>(P.ktab.data(), 4 * c.n_keys) : Sec<const uint32_t>{};
    // (pinned, behind the arena: the batch verdict word, the wave batch check's group verdicts, the
    // dense key sums' per-item modes)
    const size_t h_dmode = al256(al256(a.total) + 64 + 4 * P.wb_ng);
    if ((rc = L.stage.ensure(h_dmode + 4 * n_dn)) || (rc = L.in.ensure(a.total))) return rc;
    uint8_t* h = static_cast<uint8_t*>(L.stage.p);
    a.fill(h);
    // scratch: the call's key records + statuses, then CallBufs's sections in its order
    const bool batch = P.batch, wavem = P.wavem;
    Layout w;
    const auto w_krec = w.packed<uint32_t>(4 * G2_REC_WORDS * n_dec);
    const auto w_kst = w.packed<int32_t>(4 * n_dec + 4);
    const auto w_srec = w.aligned<uint32_t>(4 * G1_REC_WORDS * n), w_hrec = w.packed<uint32_t>(4 * G1_REC_WORDS * n),
               w_arec = w.packed<uint32_t>(4 * G2_REC_WORDS * (n + 1));
    const auto w_st = w.packed<int32_t>(4 * n), w_ssig = w.aligned<int32_t>(4 * n), w_sapk = w.aligned<int32_t>(4 * n),
               w_ok = w.aligned<int32_t>(4);
    const auto w_frec = w.aligned<uint32_t>(4 * F12_REC_WORDS * (batch ? n + 1 : 0)),
               w_jrec = w.aligned<uint32_t>(4 * G1J_REC_WORDS * (batch ? n : 0)),
               w_prec = w.aligned<uint32_t>(4 * G1J_REC_WORDS * (batch ? n + 1 : 0) + 4),
               w_hh = w.aligned<uint32_t>(4 * G1H_REC_WORDS * (wavem ? n : 0));
    const auto w_sdec = w.aligned<int32_t>(4 * n), w_ssub = w.aligned<int32_t>(4 * n),
               w_spair = w.aligned<int32_t>(4 * n + 4);
    const auto w_aj = w.aligned<uint32_t>(4 * G2J_WORDS * (wavem ? n + P.wb_ng : 0) + 4),
               w_wf = w.aligned<uint32_t>(4 * FB_REC_WORDS * P.wb_m), w_wp = w.aligned<uint32_t>(4 * G1H_REC_WORDS * P.wb_m),
               w_wj = w.aligned<uint32_t>(4 * G1J_REC_WORDS * (P.wbatch ? n : 0)),
               w_wsg = w.aligned<uint32_t>(4 * G1_REC_WORDS * P.wb_ng), w_winb = w.aligned<uint32_t>(4 * (P.wbatch ? n : 0));
    const auto w_wgok = w.aligned<int32_t>(4 * P.wb_ng + 4);
    const auto w_dtot = w.aligned<uint32_t>(4 * (n_dn ? DT_WORDS : 0)), w_dmode = w.aligned<uint32_t>(4 * n_dn + 4);
    if ((rc = L.work.ensure(w.end))) return rc;
    void* in = L.in.p;
    void* wk = L.work.p;
    const bool lines = P.cached && d.kc.lines_slots;
    CallBufs B;
    B.n = n;
    B.dl = c.dl;
    B.keys = o_keys.at(in), B.sigs = o_sigs.at(in), B.msg = o_msg.at(in), B.dst = o_dst.at(in), B.seed = o_seed.at(in);
    B.kslot = o_kslot.at(in), B.off = o_off.at(in), B.cnt = o_cnt.at(in), B.idx = o_idx.at(in), B.mlen = o_mlen.at(in);
    B.moff = o_moff.at(in);
    B.km = P.kside ? o_kmode.at(in) : nullptr;
    B.scs = o_scs.at(in);
    const uint8_t* ring = o_ring.at(in);
    B.aoff = Sec<uint64_t>{o_ring.off}.at(in);
    B.hsrc = Sec<uint32_t>{o_ring.off + P.r_hsrc}.at(in), B.hpub = Sec<uint32_t>{o_ring.off + P.r_hpub}.at(in);
    B.aslot = Sec<uint32_t>{o_ring.off + P.r_aslot}.at(in), B.alen = Sec<uint32_t>{o_ring.off + P.r_alen}.at(in);
    B.amsg = ring + P.r_amsg;
    B.fill_item = o_fill.at(in), B.fill_slot = o_fill.at(in) + P.n_fill;
    B.dlist = o_dlist.at(in), B.rlist = o_rlist.at(in), B.idx0 = o_idx0.at(in), B.ktab = o_ktab.at(in);
    B.srec = w_srec.at(wk), B.hrec = w_hrec.at(wk), B.arec = w_arec.at(wk), B.frec = w_frec.at(wk);
    B.jrec = w_jrec.at(wk), B.prec = w_prec.at(wk), B.hh = w_hh.at(wk), B.ajrec = w_aj.at(wk);
    B.st = w_st.at(wk), B.ssig = w_ssig.at(wk), B.sapk = w_sapk.at(wk), B.okw = w_ok.at(wk);
    B.sdec = w_sdec.at(wk), B.ssub = w_ssub.at(wk), B.spair = w_spair.at(wk);
    B.wf = w_wf.at(wk), B.wp = w_wp.at(wk), B.wj = w_wj.at(wk), B.wsg = w_wsg.at(wk), B.winb = w_winb.at(wk);
    B.wgok = w_wgok.at(wk);
    B.dtot = w_dtot.at(wk), B.dmode = w_dmode.at(wk);
    B.kt = KeyTab{P.cached ? static_cast<const uint32_t*>(d.kc.rec.p) : nullptr,
                  P.cached ? static_cast<const int32_t*>(d.kc.st.p) : nullptr,
                  w_krec.at(wk),
                  w_kst.at(wk),
                  lines ? static_cast<const uint32_t*>(d.kc.lines.p) : nullptr,
                  P.cached ? static_cast<const uint32_t*>(d.kc.hrec.p) : nullptr,
                  P.use_apk ? static_cast<const uint32_t*>(d.ar.rec.p) : nullptr,
                  P.use_apk ? static_cast<const uint32_t*>(d.ar.lines.p) : nullptr};
    B.h_ok = Sec<int32_t>{al256(a.total)}.at(h), B.h_gok = Sec<int32_t>{al256(a.total) + 64}.at(h);
    B.h_dmode = Sec<uint32_t>{h_dmode}.at(h);
    const hipStream_t s0 = L.stream;
    S.kept.stream = s0;
    BLS_HIP(nwv_stage::stage_h2d(in, h, a.total, s0));  // small calls: through kernel arguments
    BLS_HIP(hipEventRecord(L.sev[0], s0));
    BLS_HIP(hipStreamWaitEvent(L.side[0], L.sev[0], 0));
    CallStats T;
    if (P.wave_small) rc = run_small(d, L, P, B, c, status, S, mstat, astat, T);
    else if (P.wavem) rc = run_large_wave(d, L, P, B, c, status, T);
    else rc = run_group(L, P, B, c, status, T);
    return rc ? rc : record_last(d, L, P, T);
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
        AheadPack ap;
        size_t j = j0;
        for (; j < n && ap.n() < chunk; j++) {
            if ((sel && !sel[j]) || len[j] > nwv::MsgKey::MAX_MSG) continue;
            const nwv::MsgKey k = nwv::MsgKey::make(dst, dl, base + off[j], len[j]);
            if (R.contains(k)) continue;
            bool dup = false;
            for (const MsgSlots::Fresh& f : ms.fresh) dup = dup || f.key == k;
            if (dup) continue;
            const uint32_t r = R.reserve();
            if (r == nwv::BlsMsgRing::NONE) continue;  // every slot in use by calls in flight
            ms.fresh.push_back({r, k, UINT32_MAX, true});
            ap.push(r, base + off[j], len[j]);
        }
        j0 = j;
        const size_t m = ap.n();
        if (!m) continue;
        Layout o;
        const auto o_off = o.packed<uint64_t>(8 * m);
        const auto o_slot = o.packed<uint32_t>(4 * m), o_len = o.packed<uint32_t>(4 * m);
        const auto o_dst = o.packed<uint8_t>(al256(dl + 1)), o_msg = o.packed<uint8_t>(ap.msg.size() + 1);
        if ((rc = L.stage.ensure(o.end)) || (rc = L.in.ensure(o.end))) return rc;
        void* h = L.stage.p;
        void* in = L.in.p;
        ap.write(h, o_slot.at(h), o_len.at(h), o_msg.at(h));
        std::memcpy(o_dst.at(h), dst, dl);
        BLS_HIP(nwv_stage::stage_h2d(in, h, o.end, L.stream));
        launch_ahead(L.stream, m, o_msg.at(in), o_off.at(in), o_len.at(in), o_dst.at(in), dl, d.mr.rec.p, o_slot.at(in));
        BLS_HIP(hipGetLastError());
        BLS_HIP(hipStreamSynchronize(L.stream));
        ms.finish(nullptr, nullptr);
    }
    return NWV_OK;
}

// a per-device threshold of the context (nwv_bls_set_*_min / nwv_bls_*_min), and the counters of the
// calling thread's last verify call (nwv_bls_last_*)
int set_min(nwv_ctx* ctx, std::atomic<size_t> BlsDev::*field, size_t n) {
    BlsCtx* c;
    int rc = ctx_of(ctx, &c);
    if (rc) return rc;
    for (BlsDev* d : c->devs) (d->*field).store(n, std::memory_order_relaxed);
    return NWV_OK;
}
size_t get_min(const nwv_ctx* ctx, std::atomic<size_t> BlsDev::*field) {
    BlsCtx* c;
    if (ctx_of(const_cast<nwv_ctx*>(ctx), &c)) return 0;
    return (c->devs[0]->*field).load(std::memory_order_relaxed);
}
template <size_t N>
int last_counters(nwv_ctx* ctx, uint64_t (BlsDev::*field)[N], uint64_t* out) {
    if (!out) return nwv_internal_set_err(NWV_ERR_ARG, "null argument");
    BlsDev* d;
    int rc = last_dev_of(ctx, &d);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(d->stat_mu);
    for (size_t k = 0; k < N; k++) out[k] = (d->*field)[k];
    return NWV_OK;
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
    BlsDev* d;
    int rc = dev_at(ctx, device_index, &c, &d);
    if (rc) return rc;
    const nwv::PlaceEntry e = c->place->get((size_t)device_index);
    const uint64_t v[6] = {e.ranges[NWV_ENGINE_BLS], e.items[NWV_ENGINE_BLS], e.out_ranges, e.peak,
                           (uint64_t)d->ordinal, c->devs.size()};
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
    const size_t v = nwv::latency_clamp(n, bls_env().shard_min);
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
    BlsDev* d;
    int rc = dev_at(ctx, device_index, &c, &d);
    if (rc) return rc;
    d->pool.counters(out);
    return NWV_OK;
}
__attribute__((visibility("hidden"))) int nwv_bls_diag_qos_priority(nwv_ctx* ctx, int device_index, int out[3]) {
    BlsCtx* c;
    BlsDev* d;
    int rc = dev_at(ctx, device_index, &c, &d);
    if (rc) return rc;
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
    const auto ranges = bls_shard_ranges(n, c->devs.size(), bls_env().shard_min);
    const auto tickets = nwv::place_ranges(*c->place, ranges, NWV_ENGINE_BLS);
    t_last_dev[ctx] = tickets[0].dev();
    if (ranges.size() == 1) {
        BlsDev& d = *c->devs[tickets[0].dev()];
        // (a single range of at most nwv_latency_max items is latency class: lane_pool.h)
        const CallIn call{n_keys, keys, n, sigs, pk_off, pk_cnt, pk_idx, n_idx, msg_base, msg_off, msg_len, msg_bytes,
                          dst, dst_len};
        return verify_on(d, call, status, ah.n ? &ah : nullptr, mstat.v, mstat.a, n <= d.latency_max.load());
    }
    std::vector<std::string> err(ranges.size());
    std::vector<MsgStat> rstat(ranges.size());  // (the ranges run on threads of their own)
    rc = bls_for_ranges(ranges, [&](size_t k, size_t lo, size_t hi) -> int {
        size_t ni = 0, mb = 0;  // the range's own key-index and message extents
        for (size_t i = lo; i < hi; i++) {
            ni = std::max<size_t>(ni, (size_t)pk_off[i] + pk_cnt[i]);
            mb = std::max<size_t>(mb, msg_off[i] + msg_len[i]);
        }
        const CallIn call{n_keys, keys, hi - lo, sigs + 48 * lo, pk_off + lo, pk_cnt + lo, pk_idx, ni, msg_base,
                          msg_off + lo, msg_len + lo, mb, dst, dst_len};
        const int e = verify_on(*c->devs[tickets[k].dev()], call, status + lo, nullptr, rstat[k].v, rstat[k].a);
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

int nwv_bls_set_wave_batch_min(nwv_ctx* ctx, size_t n) { return set_min(ctx, &BlsDev::wave_batch_min, n); }
size_t nwv_bls_wave_batch_min(const nwv_ctx* ctx) { return get_min(ctx, &BlsDev::wave_batch_min); }
int nwv_bls_last_batch(nwv_ctx* ctx, uint64_t out[3]) { return last_counters(ctx, &BlsDev::last_batch, out); }

int nwv_bls_set_key_batch_min(nwv_ctx* ctx, size_t n) { return set_min(ctx, &BlsDev::key_batch_min, n); }
size_t nwv_bls_key_batch_min(const nwv_ctx* ctx) { return get_min(ctx, &BlsDev::key_batch_min); }
int nwv_bls_last_key_batch(nwv_ctx* ctx, uint64_t out[5]) { return last_counters(ctx, &BlsDev::last_kbatch, out); }

int nwv_bls_set_apk_dense_min(nwv_ctx* ctx, size_t n) { return set_min(ctx, &BlsDev::apk_dense_min, n); }
size_t nwv_bls_apk_dense_min(const nwv_ctx* ctx) { return get_min(ctx, &BlsDev::apk_dense_min); }
int nwv_bls_last_apk_dense(nwv_ctx* ctx, uint64_t out[4]) { return last_counters(ctx, &BlsDev::last_apkd, out); }

int nwv_bls_last_keys(nwv_ctx* ctx, uint64_t out[2]) { return last_counters(ctx, &BlsDev::last_keys, out); }

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
            if (sc.holds_all(n, sigs48)) holder = j;
        }
    const nwv::Ticket ticket = holder < c->devs.size() ? nwv::Ticket(*c->place, holder, (uint64_t)n, NWV_ENGINE_BLS)
                                                       : nwv::Ticket(*c->place, (uint64_t)n, NWV_ENGINE_BLS);
    BlsDev* d = c->devs[ticket.dev()];
    LaneLease lane(*d, n <= d->latency_max.load());
    if ((rc = lane.rc())) return rc;
    BlsLane& L = *lane;
    // scratch: records, statuses, the sum tree's two partial-sum levels, the output, decode statuses
    const size_t n_part = (n + wave::G1SUM_N - 1) / wave::G1SUM_N + 1;  // g1_sum_per
    Layout w;
    const auto w_rec = w.aligned<uint32_t>(4 * G1_REC_WORDS * n);
    const auto w_st = w.aligned<int32_t>(4 * n);
    const auto w_pa = w.aligned<uint32_t>(4 * G1P_WORDS * n_part), w_pb = w.aligned<uint32_t>(4 * G1P_WORDS * n_part);
    const auto w_out = w.aligned<uint8_t>(64);
    const auto w_ost = w.packed<int32_t>(8), w_st2 = w.aligned<int32_t>(4 * n);
    if ((rc = L.in.ensure(48 * n)) || (rc = L.work.ensure(w.end)) || (rc = L.stage.ensure(128))) return rc;
    void* wk = L.work.p;
    uint32_t* rec = w_rec.at(wk);
    int32_t *st = w_st.at(wk), *sdec = w_st2.at(wk);
    // the sum of the records at `in` (through the positions idx_d when given) as a tree of
    // k_blsw_g1_sum levels; the last (one block) takes the first bad status of st_d when given
    auto sum_tree = [&](const uint32_t* in, const uint32_t* idx_d, const int32_t* st_d) {
        uint32_t m = (uint32_t)n;
        const uint32_t* src = in;
        int hom = 0, flip = 0;
        while (m > (uint32_t)wave::G1SUM_N) {
            const uint32_t per = g1_sum_per(m);
            const uint32_t nb = (m + per - 1) / per;
            uint32_t* dst = (flip ? w_pb : w_pa).at(wk);
            hipLaunchKernelGGL(k_blsw_g1_sum, dim3(nb), dim3(64), 0, L.stream, m, src, idx_d, hom, dst, per);
            src = dst;
            idx_d = nullptr;
            hom = 1;
            m = nb;
            flip ^= 1;
        }
        hipLaunchKernelGGL(k_blsw_g1_sum_fin, dim3(1), dim3(64), 0, L.stream, m, src, idx_d, hom,
                           st_d ? (uint32_t)n : 0u, st_d, w_out.at(wk), w_ost.at(wk));
    };
    auto fetch = [&]() -> int {
        BLS_HIP(hipGetLastError());
        uint8_t* hs = static_cast<uint8_t*>(L.stage.p);
        BLS_HIP(hipMemcpyAsync(hs, w_out.at(wk), 64 + 8, hipMemcpyDeviceToHost, L.stream));
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
        std::vector<uint32_t> pos(n <= SC_CAP ? n : 0);
        if (d->sc.holds_all(n, sigs48, pos.data())) {
            BLS_HIP(nwv_stage::stage_h2d(L.in.p, pos.data(), 4 * n, L.stream));
            sum_tree(static_cast<const uint32_t*>(d->sc.rec.p), static_cast<const uint32_t*>(L.in.p), nullptr);
            return fetch();
        }
    }
    BLS_HIP(nwv_stage::stage_h2d(L.in.p, sigs48, 48 * n, L.stream));
    const uint8_t* sig_d = static_cast<const uint8_t*>(L.in.p);
    if (n <= 1024) {  // decode on one lane each, the G1 checks on a wave each
        hipLaunchKernelGGL(k_blsw_sigdec, dim3(kBlocks(n)), dim3(BLS_LANES), 0, L.stream, (uint32_t)n, sig_d, rec, sdec);
        hipLaunchKernelGGL(k_blsw_sub, dim3((unsigned)n), dim3(64), 0, L.stream, (uint32_t)n, rec, sdec, st);
        hipLaunchKernelGGL(k_bls_st_join, dim3(kBlocks(n)), dim3(BLS_LANES), 0, L.stream, (uint32_t)n, sdec, st);
    } else {
        hipLaunchKernelGGL(k_bls_sigs, dim3(kBlocks(n)), dim3(BLS_LANES), 0, L.stream, (uint32_t)n, sig_d, rec, st);
    }
    sum_tree(rec, nullptr, st);
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
