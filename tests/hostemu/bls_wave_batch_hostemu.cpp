// Host build of the wave engine's batch check (narwhal_amd/csrc/bls_verify.h: wb_points, wb_sfold,
// wb_sig_item, wave::miller_script, w_ffold_step, w_group_final) -- TEST INFRASTRUCTURE ONLY:
// tests/test_bls_wave_batch_hostemu.py runs one group through the stages the kernels of
// nwv_bls.hip run, with the same interpreter and stage tables, on the CPU.
#include <vector>

#define BLS_GROUP_HOST_EMU 1
#include "../../narwhal_amd/csrc/bls_verify.h"

using namespace bls;

namespace {

// one Miller item as the packed kernel sets a bank up (pair_flat): PA = (x, -y) of the signature
// record or zeros, PB = the homogeneous hash record or the identity, QB = a Jacobian G2 record,
// then the script's ops.  lines = the item's line table (fixed mode) or null.  script_len < 0: the
// script's own length.  Writes the F record; its count word is 1 only when the script ran.
void miller_item(const uint32_t* sig_rec, const uint32_t* hh_rec, const uint32_t* q_jac, const uint32_t* lines,
                 int script_len, uint32_t* f_out) {
    using namespace wave;
    std::vector<uint32_t> bank(WM_WORDS_PC, 0);
    Wave w;
    w.wm = bank.data() + KP_WORDS;
    init_slots_pc(w);
    w.zero(REG_PA, 2);
    w.zero(REG_PB, 3);
    w.zero(REG_QB, 6);
    if (sig_rec && !sig_rec[2 * NL]) {
        w.put_words(REG_PA, sig_rec, 1);
        w.put_fp(REG_PA + 1, fp_neg(ld_fp(sig_rec + NL)));
    }
    if (!hh_rec[3 * NL]) w.put_words(REG_PB, hh_rec, 3);
    else w.put_fp(REG_PB + 2, k_one());
    w.put_words(REG_QB, q_jac, 6);
    w.zero(REG_F, 12);
    w.put_fp(REG_F, k_one());
    w.copy_slots(REG_TB, REG_QB, 6);
    static SOp ops[SCRIPT_MAX];
    const bool fixed = lines != nullptr;
    int cnt = miller_script(fixed, ops);
    if (script_len >= 0 && script_len < cnt) cnt = script_len;
    int steps = 0;
    for (int i = 0; i < cnt; i++) {
        const SOp& o = ops[i];
        if (sop_kind(o) == SOP_LINES) {
            w.put_words(REG_LA, &T_G2_LINES[o.a][0][0], 6);
            if (fixed) w.put_words(REG_LB, lines + (size_t)o.a * 6 * NL, 6);
            steps++;
        } else if (sop_kind(o) == SOP_INV) {
            w.invert_slot((int)o.a, (int)o.b);
        } else {
            w.run(Prog{o.a, (uint16_t)(o.b & 0xffffu), (uint16_t)(o.b >> 16)}, (int)(o.c & 0xffffu));
        }
    }
    const bool ran = cnt > 0 && steps == NSTEPS;
    for (int t = 0; t < 12 * NL; t++) f_out[t] = ran ? w.wm[SW * REG_F + t] : 0u;
    f_out[12 * NL] = ran ? 1u : 0u;
    f_out[12 * NL + 1] = 0u;
}

void q_jac_from_affine(const uint32_t* g2_rec, uint32_t* out) {
    for (int t = 0; t < 4 * NL; t++) out[t] = g2_rec[t];
    st_fp(out + 4 * NL, k_one());
    st_fp(out + 5 * NL, fp_zero());
    out[6 * NL] = 0u;
}

}  // namespace

extern "C" {

// 1 when miller_script's ops are pairing_script's ops before its P_CONJ_F run (and that run
// follows them), the next_run links of the cut script name its own RUN ops, and the last is -1
int bh_wb_script_is_prefix(int fixed) {
    using namespace wave;
    static SOp full[SCRIPT_MAX], cut[SCRIPT_MAX];
    const int nf = pairing_script(fixed != 0, full), nc = miller_script(fixed != 0, cut);
    if (nc <= 0 || nc >= nf) return 0;
    for (int i = 0; i < nc; i++)
        if (full[i].a != cut[i].a || full[i].b != cut[i].b || full[i].c != cut[i].c) return 0;
    const SOp& nx = full[nc];
    if (sop_kind(nx) != SOP_RUN || nx.a != P_CONJ_F.off) return 0;
    int lines = 0;
    for (int i = 0; i < nc; i++) {
        if (sop_kind(cut[i]) == SOP_LINES) lines++;
        if (sop_kind(cut[i]) == SOP_INV) return 0;  // the inversion belongs to the final exponentiation
        int j = i + 1;
        while (j < nc && sop_kind(cut[j]) != SOP_RUN) j++;
        if (cut[i].next_run != (j < nc ? j : -1)) return 0;
    }
    return lines == NSTEPS ? 1 : 0;
}
int bh_wb_script_len(int fixed) {
    static wave::SOp ops[wave::SCRIPT_MAX];
    return wave::miller_script(fixed != 0, ops);
}

// One group of n one-key items (signature sigs + 48 i, key pks + 96 i, 32-byte message msgs + 32 i)
// through the wave batch check's stages.  modes[i]: 0 = hash cleared, computed lines; 1 = hash
// cleared, the key's precomputed line table; 2 = the key-side form (H0 not cofactor-cleared, the
// key record [h_eff] pk, its line table).  script_len < 0: the Miller script whole; else cut to
// that many ops (0: an empty script).  fan: records a tree step multiplies (>= 2).  Returns 1 accept, 0 reject, -1 when an item does not decode.
int bh_wb_group(size_t n, const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs, const int* modes,
                const uint8_t* seed, const uint8_t* dst, size_t dl, int script_len, uint32_t fan) {
    using namespace wave;
    const size_t m = n + 1;
    std::vector<uint32_t> frec(FB_REC_WORDS * m), jrec(G1J_REC_WORDS * n), prec(G1H_REC_WORDS * m),
        qrec(G2J_REC_WORDS * m), sg(G1_REC_WORDS);
    std::vector<std::vector<uint32_t>> tabs(n);
    Wave full;
    std::vector<uint32_t> fullm(WM_WORDS);
    full.wm = fullm.data() + KP_WORDS;
    for (size_t i = 0; i < n; i++) {
        uint32_t srec[G1_REC_WORDS], hrec[G1_REC_WORDS], krec[G2_REC_WORDS], arec[G2_REC_WORDS];
        const uint32_t idx = 0;
        int32_t kst = key_decode(pks + 96 * i, krec);
        if (sig_decode(sigs + 48 * i, srec) != ST_OK || kst != ST_OK || apk_record(krec, &kst, &idx, 1, arec) != ST_OK)
            return -1;
        if (modes[i] == 2) {  // H0 = the two maps' sum, the key record [h_eff] pk (k_bls_key_heff)
            const jac<fp> h0 = jac_add(h2c_map(msgs + 32 * i, 32, dst, (uint32_t)dl, 0),
                                       h2c_map(msgs + 32 * i, 32, dst, (uint32_t)dl, 1));
            fp x = fp_zero(), y = fp_zero();
            if (!h0.inf) g1_to_affine(x, y, h0);
            st_g1(hrec, x, y, h0.inf);
            fp2 ax, ay;
            ld_g2(arec, ax, ay);
            g2_to_affine(ax, ay, jac_mul64(jac_from_affine(ax, ay), BLS_H_EFF));
            st_g2(arec, ax, ay, false);
        } else {
            h2c_record(msgs + 32 * i, 32, dst, (uint32_t)dl, hrec);
        }
        if (modes[i] != 0) {
            tabs[i].resize((size_t)NSTEPS * 6 * NL);
            w_key_lines(full, arec, tabs[i].data());
        }
        q_jac_from_affine(arec, qrec.data() + G2J_REC_WORDS * i);
        if (srec[2 * NL])  // an identity signature stays out of the batch (not used by the tests)
            wb_neutral(prec.data() + G1H_REC_WORDS * i, jrec.data() + G1J_REC_WORDS * i);
        else
            wb_points(srec, hrec, rlc_scalar(seed, (uint32_t)i), prec.data() + G1H_REC_WORDS * i,
                      jrec.data() + G1J_REC_WORDS * i);
    }
    for (uint32_t lv = (uint32_t)n; lv > 1; lv = (lv + 1) / 2)
        for (uint32_t j = 0; j < (lv + 1) / 2; j++) wb_sfold(jrec.data(), j, lv, (uint32_t)n);
    wb_sig_item(jrec.data(), sg.data(), prec.data() + G1H_REC_WORDS * n, qrec.data() + G2J_REC_WORDS * n);
    for (size_t i = 0; i < n; i++)
        miller_item(nullptr, prec.data() + G1H_REC_WORDS * i, qrec.data() + G2J_REC_WORDS * i,
                    tabs[i].empty() ? nullptr : tabs[i].data(), script_len, frec.data() + FB_REC_WORDS * i);
    // the signature item: -S_g against g2's own lines, g2's table again on its unused pair
    miller_item(sg.data(), prec.data() + G1H_REC_WORDS * n, qrec.data() + G2J_REC_WORDS * n,
                &T_G2_LINES[0][0][0], script_len, frec.data() + FB_REC_WORDS * n);
    if (fan < 2) fan = WB_FAN;
    // the product tree, fan records a step, every step on a bank of NSLOTS_PC slots
    std::vector<uint32_t> bank(WM_WORDS_PC, 0);
    Wave w;
    w.wm = bank.data() + KP_WORDS;
    auto at = [&](uint32_t p) { return (const uint32_t*)(frec.data() + (size_t)FB_REC_WORDS * p); };
    for (uint32_t s = 1;; s *= fan) {
        const uint32_t ents = ((uint32_t)m + s - 1) / s, waves = (ents + fan - 1) / fan;
        for (uint32_t wv = 0; wv < waves; wv++) {
            const uint32_t p0 = wv * fan * s;
            const uint32_t cnt = w_ffold_step(w, at, p0, s, (uint32_t)m, fan);
            if (waves == 1) return cnt == (uint32_t)m && w_group_final(w) ? 1 : 0;
            uint32_t* o = frec.data() + (size_t)FB_REC_WORDS * p0;
            for (int t = 0; t < 12 * NL; t++) o[t] = w.wm[SW * REG_F + t];
            o[12 * NL] = cnt;
        }
    }
}

}  // extern "C"
