// Host build of the key side of a BLS call that uses the aggregate-key ring
// (narwhal_amd/csrc/bls_verify.h: w_apk_fill, the item function of k_blsw_apk_fill, with
// w_key_lines and w_pairing_check_g beside it) -- TEST INFRASTRUCTURE ONLY:
// tests/test_bls_apk_ring_hostemu.py fills a slot from a set's key sum and runs a miss item's and a
// hit item's pairing check with the same interpreter and stage tables the kernels run, on the CPU.
#include <vector>

#define BLS_GROUP_HOST_EMU 1
#include "../../narwhal_amd/csrc/bls_verify.h"

using namespace bls;

namespace {

// a wave whose slots start out as `fill` in every word: a result may not depend on what an
// earlier program left behind
wave::Wave fresh_wave(std::vector<uint32_t>& wm, uint32_t fill) {
    wm.assign(wave::WM_WORDS, fill);
    wave::Wave w;
    w.wm = wm.data() + wave::KP_WORDS;
    return w;
}
void st_g2j(uint32_t* o, const jac<fp2>& p) {
    st_f2(o, p.x);
    st_f2(o + 2 * NL, p.y);
    st_f2(o + 4 * NL, p.z);
    o[6 * NL] = p.inf ? 1u : 0u;
}

}  // namespace

extern "C" {

int bah_rec_words() { return G2_REC_WORDS; }
int bah_jac_words() { return G2J_REC_WORDS; }
int bah_line_words() { return wave::NSTEPS * 6 * wave::SW; }

// registration's [h_eff] pk record of a key (key_decode, then k_bls_key_heff's lane); the key's
// status
int bah_key_heff(const uint8_t* pk96, uint32_t* hrec) {
    uint32_t rec[G2_REC_WORDS];
    const int32_t st = key_decode(pk96, rec);
    if (st != ST_OK) return st;
    fp2 x, y;
    ld_g2(rec, x, y);
    g2_to_affine_vt(x, y, jac_mul64(jac_from_affine(x, y), BLS_H_EFF));
    st_g2(hrec, x, y, false);
    return ST_OK;
}
// n field elements made canonical in place (a record's limbs stand for a value in [0, 2p))
void bah_canon(uint32_t* words, int n) {
    for (int k = 0; k < n; k++) st_fp(words + NL * k, fp_canon(ld_fp(words + NL * k)));
}
// registration's line table of a record (k_blsw_key_lines' wave)
void bah_key_lines(const uint32_t* rec, uint32_t fill, uint32_t* lines) {
    std::vector<uint32_t> wm;
    w_key_lines(fresh_wave(wm, fill), rec, lines);
}
// the key sum of a key-side item of cnt >= 2 keys as blsw_apk_item forms it: lane j adds records
// j, j + 64, ..., then lane l takes lane l + h for h = 32 .. 1.  aj: the Jacobian record (the
// identity, zeroed, when the status is not OK); the item's key status
int bah_sum(const uint32_t* hrecs, size_t cnt, uint32_t* aj) {
    jac<fp2> acc[64];
    for (int l = 0; l < 64; l++) {
        acc[l].inf = true;
        acc[l].x = acc[l].y = acc[l].z = f2_zero();
        for (size_t j = (size_t)l; j < cnt; j += 64) {
            fp2 x, y;
            ld_g2(hrecs + (size_t)G2_REC_WORDS * j, x, y);
            acc[l] = jac_add(acc[l], jac_from_affine(x, y));
        }
    }
    for (int h = 32; h >= 1; h >>= 1)
        for (int l = 0; l < h; l++) acc[l] = jac_add(acc[l], acc[l + h]);
    int32_t st = ST_OK;
    if (cnt == 0) st = ST_AGGR_MISMATCH;
    else if (acc[0].inf) st = ST_PK_INFINITY;
    if (st != ST_OK) {
        acc[0].inf = true;
        acc[0].x = acc[0].y = acc[0].z = f2_zero();
    }
    st_g2j(aj, acc[0]);
    return st;
}
// the fill of a ring slot from a key sum and its status: 1 when the slot was written
int bah_fill(const uint32_t* aj, int st, uint32_t fill, uint32_t* rec, uint32_t* lines) {
    std::vector<uint32_t> wm;
    return w_apk_fill(fresh_wave(wm, fill), aj, st, rec, lines) ? 1 : 0;
}
// a one-key item's key sum: the record copied with Z = 1 (blsw_apk_item's cnt == 1 branch)
void bah_one_key(const uint32_t* rec, uint32_t* aj) {
    for (int t = 0; t < 4 * NL; t++) aj[t] = rec[t];
    st_fp(aj + 4 * NL, k_one());
    st_fp(aj + 5 * NL, fp_zero());
    aj[6 * NL] = 0u;
}
// a key-side item's pairing verdict (blsw_pair_item): the raw hash of msg, the signature's record,
// the Jacobian key sum aj, and the key's line table or null (computed lines).  The signature must
// decode (its G1 membership is another kernel's business).
int bah_verdict(const uint8_t* sig48, const uint8_t* msg, size_t n, const uint8_t* dst, size_t dl, const uint32_t* aj,
                const uint32_t* lines, uint32_t fill) {
    uint32_t srec[G1_REC_WORDS], hrec[G1H_REC_WORDS];
    fp x, y;
    bool inf;
    const int32_t st = g1_decompress(x, y, inf, sig48);
    if (st != ST_OK) return st;
    st_g1(srec, inf ? fp_zero() : x, inf ? fp_zero() : y, inf);
    std::vector<uint32_t> wm;
    const wave::Wave w = fresh_wave(wm, fill);
    w_hash_to_g1(w, msg, (uint32_t)n, dst, (uint32_t)dl, hrec, false);
    return w_pairing_check_g(w, srec, hrec, true, aj, true, lines) ? ST_OK : ST_VERIFY_FAIL;
}

}  // extern "C"
