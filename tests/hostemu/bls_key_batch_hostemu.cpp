// Host build of the key-transposed batch check (narwhal_amd/csrc/bls_key_batch.h's plan;
// bls_verify.h: wb_point_s on both sides, kb_lane_sum and the key sums' tree, wb_store_hom,
// kb_key_q_word, wb_sfold, wb_sig_item, wave::miller_script, w_ffold_step, w_group_final) -- TEST
// INFRASTRUCTURE ONLY: tests/test_bls_key_batch_hostemu.py runs a call's groups through the stages
// the kernels of nwv_bls.hip run, with the same interpreter and stage tables, on the CPU, and
// compares each group's value after the final exponentiation with the product of its items' own
// pairing values raised to their coefficients (the scalar code of bls381.h).
#include "bls_wave_batch_hostemu.cpp"  // miller_item: a Miller entry as the packed kernel sets a bank up

#include "../../narwhal_amd/csrc/bls_key_batch.h"

namespace {

bool f12_same(const fp12& a, const fp12& b) {
    uint32_t x[F12_REC_WORDS], y[F12_REC_WORDS];
    st_f12(x, a);
    st_f12(y, b);
    for (int k = 0; k < 12; k++)
        if (!ops<fp>::eq(ld_fp(x + NL * k), ld_fp(y + NL * k))) return false;
    return true;
}
fp12 f12_pow64(const fp12& a, uint64_t k) {
    fp12 acc = f12_one();
    for (int b = 63; b >= 0; b--) {
        acc = f12_sqr(acc);
        if ((k >> b) & 1) acc = f12_mul(acc, a);
    }
    return acc;
}

}  // namespace

extern "C" {

// A call of n items over nk registered keys: item i has signature sigs + 48 i, the 32-byte message
// msgs + 32 i and the key list klist[koff[i] .. + kcnt[i]) (key numbers, with multiplicity).  Every
// item is key-side: H0 not cofactor-cleared, the keys' [h_eff] pk records and line tables.  Groups
// of `group` items (no group is dropped), trees of `fan` records a step (< 2: WB_FAN).  skew >= 0:
// that item's coefficient multiplies its hash contributions only (its signature enters with 1).
// Per group g: verdict[g] = 1 accept / 0 reject; same[g] = 1 when the group's value after the
// final exponentiation equals prod_i t_i^{r_i}, t_i = FE(f(-sig_i, g2) f(H0_i, [h_eff] apk_i)) by
// the scalar code; ref_one[g] = 1 when that product is 1; millers[g] = the group's Miller entries.
// Returns the number of groups, or -1 when an input does not decode.
int bh_kb_groups(size_t n, const uint8_t* sigs, size_t nk, const uint8_t* pks, const uint32_t* koff,
                 const uint32_t* kcnt, const uint32_t* klist, const uint8_t* msgs, const uint8_t* seed,
                 const uint8_t* dst, size_t dl, uint32_t group, uint32_t fan, int skew, int32_t* verdict,
                 int32_t* same, int32_t* ref_one, uint32_t* millers) {
    using namespace wave;
    Wave full;
    std::vector<uint32_t> fullm(WM_WORDS);
    full.wm = fullm.data() + KP_WORDS;
    // the registered keys: [h_eff] pk and its line table
    std::vector<uint32_t> hk(G2_REC_WORDS * nk);
    std::vector<std::vector<uint32_t>> tabs(nk);
    for (size_t k = 0; k < nk; k++) {
        uint32_t krec[G2_REC_WORDS];
        if (key_decode(pks + 96 * k, krec) != ST_OK) return -1;
        fp2 ax, ay;
        ld_g2(krec, ax, ay);
        g2_to_affine(ax, ay, jac_mul64(jac_from_affine(ax, ay), BLS_H_EFF));
        st_g2(hk.data() + G2_REC_WORDS * k, ax, ay, false);
        tabs[k].resize((size_t)NSTEPS * 6 * NL);
        w_key_lines(full, hk.data() + G2_REC_WORDS * k, tabs[k].data());
    }
    std::vector<uint32_t> srec(G1_REC_WORDS * n), hrec(G1_REC_WORDS * n);
    for (size_t i = 0; i < n; i++) {
        if (sig_decode(sigs + 48 * i, srec.data() + G1_REC_WORDS * i) != ST_OK || srec[G1_REC_WORDS * i + 2 * NL])
            return -1;
        const jac<fp> h0 = jac_add(h2c_map(msgs + 32 * i, 32, dst, (uint32_t)dl, 0),
                                   h2c_map(msgs + 32 * i, 32, dst, (uint32_t)dl, 1));
        fp x = fp_zero(), y = fp_zero();
        if (!h0.inf) g1_to_affine(x, y, h0);
        st_g1(hrec.data() + G1_REC_WORDS * i, x, y, h0.inf);
    }
    std::vector<uint8_t> ok(n, 1);
    nwv::KeyBatchPlan P;
    nwv::key_batch_plan(n, ok.data(), ok.data(), koff, kcnt, klist, (uint32_t)nk, group, 0, P);
    if (!P.run) return 0;
    const size_t ne = P.items.size(), ng = P.groups(), M = P.entries(), KM = M + ng;
    std::vector<uint32_t> hj(G1J_REC_WORDS * ne), sj(G1J_REC_WORDS * ne), sg(G1_REC_WORDS * ng),
        prec(G1H_REC_WORDS * KM), qrec(G2J_REC_WORDS * KM), frec(FB_REC_WORDS * KM);
    // k_blsk_rlc_pts
    for (size_t e = 0; e < ne; e++) {
        const uint32_t i = P.items[e];
        const uint64_t r = rlc_scalar(seed, i);
        wb_point_s(hrec.data() + G1_REC_WORDS * i, r, hj.data() + G1J_REC_WORDS * e);
        wb_point_s(srec.data() + G1_REC_WORDS * i, (int)i == skew ? 1u : r, sj.data() + G1J_REC_WORDS * e);
    }
    // k_blsw_sfold's levels
    const uint32_t gmax = (uint32_t)(group < ne ? group : ne);
    for (uint32_t m = gmax; m > 1; m = (m + 1) / 2)
        for (uint32_t g = 0; g < ng; g++)
            for (uint32_t j = 0; j < (m + 1) / 2; j++)
                wb_sfold(sj.data() + (size_t)G1J_REC_WORDS * g * group, j, m,
                         (uint32_t)(group < ne - g * group ? group : ne - g * group));
    // k_blsk_key_sums: 64 lanes' shares, the six-level tree
    for (size_t m = 0; m < M; m++) {
        jac<fp> acc[64];
        for (uint32_t l = 0; l < 64; l++)
            acc[l] = kb_lane_sum(hj.data(), P.cidx.data() + P.coff[m], P.coff[m + 1] - P.coff[m], l, 64);
        for (int h = 32; h >= 1; h >>= 1)
            for (int l = 0; l < h; l++) acc[l] = jac_add(acc[l], acc[l + h]);
        wb_store_hom(prec.data() + G1H_REC_WORDS * m, acc[0]);
        for (int wd = 0; wd < G2J_REC_WORDS; wd++)
            qrec[G2J_REC_WORDS * m + wd] = kb_key_q_word(hk.data() + G2_REC_WORDS * P.eslot[m], wd);
    }
    // k_blsk_sig_items, the Miller pass
    for (size_t g = 0; g < ng; g++)
        wb_sig_item(sj.data() + (size_t)G1J_REC_WORDS * g * group, sg.data() + G1_REC_WORDS * g,
                    prec.data() + G1H_REC_WORDS * (M + g), qrec.data() + G2J_REC_WORDS * (M + g));
    for (size_t m = 0; m < M; m++)
        miller_item(nullptr, prec.data() + G1H_REC_WORDS * m, qrec.data() + G2J_REC_WORDS * m, tabs[P.eslot[m]].data(),
                    -1, frec.data() + FB_REC_WORDS * m);
    for (size_t g = 0; g < ng; g++)
        miller_item(sg.data() + G1_REC_WORDS * g, prec.data() + G1H_REC_WORDS * (M + g),
                    qrec.data() + G2J_REC_WORDS * (M + g), &T_G2_LINES[0][0][0], -1, frec.data() + FB_REC_WORDS * (M + g));
    if (fan < 2) fan = WB_FAN;
    std::vector<uint32_t> bank(WM_WORDS_PC, 0);
    Wave w;
    w.wm = bank.data() + KP_WORDS;
    for (uint32_t g = 0; g < ng; g++) {
        // k_blsk_ffold's levels
        const uint32_t e0 = P.goff[g], keys = P.goff[g + 1] - e0, m = keys + 1;
        millers[g] = m;
        auto at = [&](uint32_t p) { return frec.data() + (size_t)FB_REC_WORDS * (p < keys ? e0 + p : M + g); };
        fp12 val = f12_one();
        for (uint32_t s = 1;; s *= fan) {
            const uint32_t ents = (m + s - 1) / s, waves = (ents + fan - 1) / fan;
            bool done = false;
            for (uint32_t wv = 0; wv < waves; wv++) {
                const uint32_t p0 = wv * fan * s;
                const uint32_t cnt = w_ffold_step(w, at, p0, s, m, fan);
                if (waves == 1) {
                    const bool one = w_group_final(w);
                    verdict[g] = cnt == m && one ? 1 : 0;
                    val = ld_f12(w.wm + SW * REG_F);
                    done = true;
                    break;
                }
                uint32_t* o = at(p0);
                for (int t = 0; t < 12 * NL; t++) o[t] = w.wm[SW * REG_F + t];
                o[12 * NL] = cnt;
            }
            if (done) break;
        }
        // the group's items one by one, scalar code
        fp12 ref = f12_one();
        for (uint32_t p = P.gfirst[g]; p < P.gfirst[g + 1]; p++) {
            const uint32_t i = P.items[p];
            jac<fp2> apk;
            apk.inf = true;
            apk.x = apk.y = apk.z = f2_zero();
            for (uint32_t j = 0; j < kcnt[i]; j++) {
                fp2 kx, ky;
                ld_g2(hk.data() + G2_REC_WORDS * klist[koff[i] + j], kx, ky);
                apk = jac_add(apk, jac_from_affine(kx, ky));
            }
            if (apk.inf || hrec[G1_REC_WORDS * i + 2 * NL]) return -1;
            fp px[2], py[2];
            fp2 qx[2], qy[2];
            px[0] = ld_fp(srec.data() + G1_REC_WORDS * i);
            py[0] = fp_neg(ld_fp(srec.data() + G1_REC_WORDS * i + NL));
            qx[0] = k_g2x();
            qy[0] = k_g2y();
            px[1] = ld_fp(hrec.data() + G1_REC_WORDS * i);
            py[1] = ld_fp(hrec.data() + G1_REC_WORDS * i + NL);
            g2_to_affine(qx[1], qy[1], apk);
            ref = f12_mul(ref, f12_pow64(final_exp(miller_loop2(2, px, py, qx, qy)), rlc_scalar(seed, i)));
        }
        same[g] = f12_same(val, ref) ? 1 : 0;
        ref_one[g] = f12_is_one(ref) ? 1 : 0;
    }
    return (int)ng;
}

}  // extern "C"
