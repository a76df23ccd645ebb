// comb_pass_hostemu.cpp -- TEST-ONLY host build of the comb pass kernel's per-signature arithmetic
// (narwhal_amd/csrc/comb_kernels.hip k_ed_comb_pass4 / k_ed_comb_pass16) with limb-bound
// assertions (NWV_BOUNDS_CHECK).  The kernel's lane functions (comb.h: comb_scalars, comb_record,
// comb_lane_sum, comb_join, comb_pass_equal) run on the CPU, workgroup by workgroup as the kernel
// lays the work out: COMB_PASS_G signatures hashed side by side, their R's decompressed four a
// wave and doubled three times each (comb_hostemu.cpp's rows_mul8: k_ed_comb's wave 0, which the
// pass kernel's decompression waves repeat), each signature's lane sums over 64 / L positions
// joined in the kernel's level order, lane t + o into lane t.  Beside the kernel's sum, the
// 64-term sum of comb_term (k_ed_comb's terms) and a plain double-and-add product as references.
// Never part of the product.
#include "comb_hostemu.cpp"

namespace {

bool same_point(const ge_p3& a, const ge_p3& b) {
    return fe_eq(fe_mul(a.X, b.Z), fe_mul(b.X, a.Z)) && fe_eq(fe_mul(a.Y, b.Z), fe_mul(b.Y, a.Z));
}

// [x] P by double-and-add from the top bit (no table of the product's)
ge_p3 scalar_mul(const ge_p3& P, const uint32_t x[8]) {
    ge_p3 acc = ge_p3_identity();
    for (int bit = 255; bit >= 0; bit--) {
        acc = ge_p3_dbl(acc);
        if ((x[bit >> 5] >> (bit & 31)) & 1u) acc = p3_add(acc, P);
    }
    return acc;
}
ge_p3 base_point() {
    uint32_t bw[8];
    ge_basepoint_words(bw);
    ge_p3 B;
    ge_decompress(bw, B);
    return B;
}

// A signature's sum on its L lanes in the kernel's order: lane t walks positions 64 t / L ..,
// level o joins lane t + o into lane t for t = 0 mod 2 o.  idle: lanes whose digits are all zero.
// false: a digit would index past a table.
bool pass_sum(Comb& B, Comb& A, const int ds[COMB_TABLES], const int dk[COMB_TABLES], int L, ge_p3& out, int* idle) {
    for (int j = 0; j < COMB_TABLES; j++) {
        // (a zero digit loads entry 1 and selects the neutral record)
        if (!B.need(j, ds[j]) || !A.need(j, dk[j]) || !B.need(j, 1) || !A.need(j, 1)) return false;
    }
    const int P = COMB_TABLES / L;
    std::vector<ge_p3> S((size_t)L);
    if (idle) *idle = 0;
    for (int t = 0; t < L; t++) {
        S[t] = comb_lane_sum(B.e.data(), A.e.data(), P * t, P, ds + P * t, dk + P * t);
        bool z = true;
        for (int p = 0; p < P; p++) z = z && ds[P * t + p] == 0 && dk[P * t + p] == 0;
        if (idle && z) (*idle)++;
    }
    for (int o = 1; o < L; o <<= 1)
        for (int t = 0; t + o < L; t += 2 * o) S[t] = comb_join(S[t], S[t + o]);
    out = S[0];
    return true;
}

// k_ed_comb's terms summed one after the other
ge_p3 term_sum(Comb& B, Comb& A, const int ds[COMB_TABLES], const int dk[COMB_TABLES]) {
    ge_p3 Q = ge_p3_identity();
    for (int j = 0; j < COMB_TABLES; j++) Q = p3_add(Q, comb_term(B.e.data(), A.e.data(), j, ds[j], dk[j]));
    return Q;
}

// [8] R's record of one encoding, as a decompression wave leaves it
void r8_of(const uint8_t enc[32], uint32_t rrec[32]) {
    const uint8_t* e4[COMB_G] = {enc, nullptr, nullptr, nullptr};
    uint32_t rr[COMB_G * 32] = {};
    rows_mul8(e4, 1, rr);
    std::memcpy(rrec, rr, 32 * sizeof(uint32_t));
}

}  // namespace

extern "C" {

int he_comb_pass_group() { return COMB_PASS_G; }

// k_ed_comb_pass<L> over n signatures (arguments as he_comb_verify's).  Returns 0, -1 when a digit
// would index past a table, -2 when a signature's lane-joined sum is not comb_term's 64-term sum.
int he_comb_pass_verify(int L, uint32_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                        const uint64_t* off, const uint32_t* len, uint8_t* verdict) {
    if (L != 4 && L != 16) return -3;
    Comb& B = comb_of_b();
    constexpr int G = COMB_PASS_G;
    for (uint32_t base = 0; base < n; base += G) {  // one workgroup
        const int cnt = (int)(n - base < (uint32_t)G ? n - base : G);
        static int dg[G][2][COMB_TABLES];
        bool hok[G];
        for (int g = 0; g < cnt; g++) {  // wave 0, lanes 0..cnt - 1
            const uint32_t i = base + g;
            uint32_t Aw[8], Rw[8], Sw[8];
            words(pk + 32 * (size_t)i, Aw);
            words(sig + 64 * (size_t)i, Rw);
            words(sig + 64 * (size_t)i + 32, Sw);
            std::vector<uint8_t> m(len[i] + 64, 0);  // (the hash over-reads past a message, masked)
            if (len[i]) std::memcpy(m.data(), msg + off[i], len[i]);
            hok[g] = comb_scalars(Aw, Rw, Sw, m.data(), len[i], dg[g][0], dg[g][1]);
        }
        uint32_t rrec[G * 32] = {};
        for (int first = 0; first < cnt; first += 4) {  // decompression wave first / 4
            const uint8_t* enc[COMB_G] = {nullptr, nullptr, nullptr, nullptr};
            const int c4 = cnt - first < 4 ? cnt - first : 4;
            for (int q = 0; q < c4; q++) enc[q] = sig + 64 * (size_t)(base + first + q);
            rows_mul8(enc, c4, rrec + 32 * first);
        }
        for (int g = 0; g < cnt; g++) {  // the sum waves: L lanes a signature
            const uint32_t i = base + g;
            KeyComb& A = comb_of_key(pk + 32 * (size_t)i);
            ge_p3 S;
            if (!pass_sum(B, A.comb, dg[g][0], dg[g][1], L, S, nullptr)) return -1;
            if (!same_point(S, term_sum(B, A.comb, dg[g][0], dg[g][1]))) return -2;
            verdict[i] = (comb_pass_equal(S, rrec + 32 * g) && A.aok && hok[g] && rrec[32 * g + 31] == 0u) ? 1 : 0;
        }
    }
    return 0;
}

// A challenge scalar fed straight to the recoding and the lane sums.  With A = [a]B, R = [r]B and
// s = r + k a (+ 1 when spoil) the equation [s]B = R + [k]A holds for the forced k (k < l), or
// misses by B.  out[0]: the kernel form's verdict; out[1]: 1 when the lane-joined sum is
// comb_term's 64-term sum and the double-and-add [s - k a]B; out[2]: lanes whose digits are all
// zero; out[3]: 1 when a digit was out of range.
int he_comb_pass_forced_k(int L, const uint8_t* k32, const uint8_t* a32, const uint8_t* r32, int spoil, int32_t out[4]) {
    if (L != 4 && L != 16) return -3;
    uint32_t k[8], a[8], r[8], ka[8], s[8];
    words(k32, k);
    words(a32, a);
    words(r32, r);
    const ge_p3 Bp = base_point();
    const ge_p3 A = scalar_mul(Bp, a), R = scalar_mul(Bp, r);
    sc_mul(k, a, ka);
    sc_add(ka, r, s);
    uint32_t e[8];  // s - k a: r, or r + 1
    std::memcpy(e, r, sizeof(e));
    if (spoil) {
        const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
        uint32_t t[8];
        sc_add(s, one, t);
        std::memcpy(s, t, sizeof(s));
        sc_add(r, one, e);
    }
    int ds[COMB_TABLES], dk[COMB_TABLES];
    comb_digits(s, ds);
    comb_digits(k, dk);
    uint32_t aw[8], rw[8];
    ge_compress(A, aw);
    ge_compress(R, rw);
    KeyComb& KA = comb_of_key(reinterpret_cast<const uint8_t*>(aw));
    ge_p3 S;
    int idle = 0;
    out[3] = pass_sum(comb_of_b(), KA.comb, ds, dk, L, S, &idle) ? 0 : 1;
    if (out[3]) return -1;
    out[2] = idle;
    out[1] = (same_point(S, term_sum(comb_of_b(), KA.comb, ds, dk)) && same_point(S, scalar_mul(Bp, e))) ? 1 : 0;
    uint32_t rrec[32];
    r8_of(reinterpret_cast<const uint8_t*>(rw), rrec);
    out[0] = (comb_pass_equal(S, rrec) && KA.aok && rrec[31] == 0u) ? 1 : 0;
    return 0;
}

// Digits fed straight to the lane sums (values the recoding never or rarely gives: +8 everywhere,
// whole lanes at zero).  A = [a]B; e32: sum_j (ds_j - dk_j a) 16^j mod l, worked out by the caller.
// out[0]: the lane-joined sum is comb_term's 64-term sum; out[1]: it is the double-and-add [e]B;
// out[2]: the kernel form accepts R = [e]B; out[3]: it rejects R = [e + 1]B; out[4]: lanes whose
// digits are all zero.  Returns -1 when a digit is out of range.
int he_comb_pass_digits(int L, const uint8_t* a32, const int32_t* ds32, const int32_t* dk32, const uint8_t* e32,
                        int32_t out[5]) {
    if (L != 4 && L != 16) return -3;
    uint32_t a[8], e[8], e1[8];
    words(a32, a);
    words(e32, e);
    const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    sc_add(e, one, e1);
    int ds[COMB_TABLES], dk[COMB_TABLES];
    for (int j = 0; j < COMB_TABLES; j++) {
        ds[j] = ds32[j];
        dk[j] = dk32[j];
    }
    const ge_p3 Bp = base_point();
    uint32_t aw[8];
    ge_compress(scalar_mul(Bp, a), aw);
    KeyComb& KA = comb_of_key(reinterpret_cast<const uint8_t*>(aw));
    ge_p3 S;
    int idle = 0;
    if (!pass_sum(comb_of_b(), KA.comb, ds, dk, L, S, &idle)) return -1;
    out[4] = idle;
    out[0] = same_point(S, term_sum(comb_of_b(), KA.comb, ds, dk)) ? 1 : 0;
    const ge_p3 E = scalar_mul(Bp, e), E1 = scalar_mul(Bp, e1);
    out[1] = same_point(S, E) ? 1 : 0;
    uint32_t w[8], rrec[32];
    ge_compress(E, w);
    r8_of(reinterpret_cast<const uint8_t*>(w), rrec);
    out[2] = (comb_pass_equal(S, rrec) && rrec[31] == 0u) ? 1 : 0;
    ge_compress(E1, w);
    r8_of(reinterpret_cast<const uint8_t*>(w), rrec);
    out[3] = (comb_pass_equal(S, rrec) && rrec[31] == 0u) ? 0 : 1;
    return 0;
}

}  // extern "C"
