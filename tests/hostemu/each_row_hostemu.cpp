// each_row_hostemu.cpp -- TEST-ONLY host build of the row kernel's per-signature arithmetic
// (narwhal_amd/csrc/each_kernels.hip k_ed_each_row) with limb-bound assertions (NWV_BOUNDS_CHECK).
// The functions the kernel calls from each.h (each_scalars / each_split_digits, each_record_coord,
// each_build_table, each_entry, each_straus, each_finish, each_is_identity, each_comb_term,
// each_cached_limbs) and the row field code (fe_row.h on the emulated wave) run on the CPU in the
// kernel's order: R on row 0 and A on row 1, their tables built in cached row form, the Straus pass
// over the 33 digit positions, [w]B added in row form, three doublings, the identity test on
// canonical limbs.  Two device-only pieces of the kernel are RESTATED here, not run:
// msm_kernels.hip's row_decompress (rows_decompress below: the same fe_row.h calls in the same
// order, the zero / sign tests lane-local) and the quad_p3_add tree (comb_sum: p3_add, the same
// field operations, in the tree's order); both have tests of their own, and the kernel body with
// its barriers, ballot bits and LDS layout runs only in tests/test_gpu_each_row.py.  Beside them
// the lane code (ed25519_lane.h) that the kernel follows: build_a_table, lane_straus_check_half.
// Never part of the product.
#define NWV_HD __host__ __device__ inline
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../narwhal_amd/csrc/each.h"

using namespace nwv;

namespace {

void words(const uint8_t* p, uint32_t w[8]) { std::memcpy(w, p, 32); }

rowf::RowConsts consts() {
    rowf::RowConsts k = rowf::row_consts();
    k.rot = 1;  // the device's rotation-form products
    return k;
}

// msm_kernels.hip row_decompress on the emulated wave: row q decompresses enc[q] and leaves its
// affine Niels record (y+x | y-x | 2dxy, 16-limb rows) in rec[48 q ..]; ok[q]: the encoding decodes
// (the zero / sign tests lane-local, as on lanes 0..2 of each row)
void rows_decompress(const uint8_t* const enc[4], uint32_t rec[4 * 48], bool ok[4]) {
    rowf::V y16;
    bool sign[4];
    for (int l = 0; l < 64; l++) {
        const int q = l >> 4, limb = l & 15;
        uint32_t v = (uint32_t)enc[q][2 * limb] | ((uint32_t)enc[q][2 * limb + 1] << 8);
        if (limb == 15) {
            sign[q] = (v >> 15) != 0;
            v &= 0x7FFFu;
        }
        y16.l[l] = v;
    }
    const rowf::RowConsts k = consts();
    rowf::V u, v, uv3, uv7, r, ri, c0, c1, c2;
    rowf::row_dec_pre(y16, k, u, v, uv3, uv7);
    const rowf::V pw = rowf::row_pow_p58(uv7, k);
    rowf::row_dec_mid(uv3, pw, u, v, k, r, ri, c0, c1, c2);
    auto limbs = [](const rowf::V& x, int q, uint32_t out[16]) {
        for (int i = 0; i < 16; i++) out[i] = x.l[16 * q + i];
    };
    rowf::V rr = r;
    for (int q = 0; q < 4; q++) {
        uint32_t a[16];
        bool z[3];
        const rowf::V* cs[3] = {&c0, &c1, &c2};
        for (int c = 0; c < 3; c++) {
            limbs(*cs[c], q, a);
            z[c] = fe_is_zero(fe_from_limbs16(a));
        }
        ok[q] = z[0] || z[1];
        if (z[1] || z[2])
            for (int i = 0; i < 16; i++) rr.l[16 * q + i] = ri.l[16 * q + i];
    }
    rowf::M flip;
    const rowf::V nrr = rowf::carry32(rowf::sub(rowf::bc(0), rr, k), k);
    for (int q = 0; q < 4; q++) {
        uint32_t a[16];
        limbs(rr, q, a);
        const bool negr = fe_is_negative(fe_from_limbs16(a)) != 0;
        for (int i = 0; i < 16; i++) flip.l[16 * q + i] = negr != sign[q];
    }
    const rowf::V x = rowf::sel(flip, rr, nrr);
    rowf::V ypx, ymx, xy2d;
    rowf::row_dec_record(x, y16, k, ypx, ymx, xy2d);
    for (int q = 0; q < 4; q++)
        for (int i = 0; i < 16; i++) {
            rec[48 * q + i] = ypx.l[16 * q + i];
            rec[48 * q + 16 + i] = ymx.l[16 * q + i];
            rec[48 * q + 32 + i] = xy2d.l[16 * q + i];
        }
}

// a decoded point's record from the lane code (one inversion), canonical limbs
void record_of(const ge_p3& P, uint32_t rec[48]) {
    const ge_precomp q = ge_p3_to_precomp(P);
    fe_to_limbs16(q.ypx, rec);
    fe_to_limbs16(q.ymx, rec + 16);
    fe_to_limbs16(q.xy2d, rec + 32);
}

// B's comb table (k_comb_table: entry 8 j + i - 1 = i 16^j B), filled as the digits ask
struct Comb {
    std::vector<uint32_t> e;
    std::vector<bool> have;
    std::vector<ge_p3> q;
    Comb() : e((size_t)COMB_WORDS, 0u), have(COMB_TABLES * COMB_ENTRIES, false) {
        uint32_t bw[8];
        ge_basepoint_words(bw);
        ge_p3 B;
        ge_decompress(bw, B);
        q.push_back(B);
        for (int j = 1; j < COMB_TABLES; j++) q.push_back(p3_dbl_n(q.back(), 4));
    }
    bool need(int j, int d) {
        const int m = d < 0 ? -d : d;
        if (m > COMB_ENTRIES) return false;
        if (m && !have[COMB_ENTRIES * j + m - 1]) {
            comb_entry_of(q[j], 0, m, e.data() + (size_t)MSM_PT_WORDS * (COMB_ENTRIES * j + m - 1));
            have[COMB_ENTRIES * j + m - 1] = true;
        }
        return true;
    }
};
Comb& comb_of_b() {
    static Comb* c = new Comb;
    return *c;
}

// the lane pipeline's basepoint tables (k_base_table)
const uint32_t* btab() {
    static std::vector<uint32_t>* t = [] {
        auto* v = new std::vector<uint32_t>((size_t)BTAB_WORDS, 0u);
        for (int j = 0; j < BASE_TABLE_ENTRIES; j++) {
            store_precomp_entry(v->data() + j * PRECOMP_ENTRY_WORDS, base_multiple(j));
            store_precomp_entry(v->data() + BASE128_TABLE_OFFSET + j * PRECOMP_ENTRY_WORDS, base128_multiple(j));
        }
        store_cached_entry(v->data() + BASE_TABLE_WORDS, ge_cached_identity());
        return v;
    }();
    return t->data();
}

// wave 1 after the digits: [w]B from the comb in the kernel's tree order, left in cached row form.
// false: a digit would index past the table.
bool comb_sum(const int dw[COMB_TABLES], uint32_t wsum[64]) {
    Comb& B = comb_of_b();
    std::vector<uint32_t> pts((size_t)64 * P3_WORDS);
    for (int lane = 0; lane < 64; lane++) {
        if (!B.need(lane, dw[lane])) return false;
        store_p3(pts.data() + P3_WORDS * lane, each_comb_term(B.e.data(), lane, dw[lane]));
    }
    // level o adds slot 2 o s + o into slot 2 o s (quad_p3_add runs p3_add's field operations)
    for (int o = 1; o < 64; o <<= 1)
        for (int s = 0; s < 32 / o; s++) {
            uint32_t* L = pts.data() + (size_t)P3_WORDS * 2 * o * s;
            store_p3(L, p3_add(load_p3(L), load_p3(L + (size_t)P3_WORDS * o)));
        }
    for (int q = 0; q < 4; q++) each_cached_limbs(load_p3(pts.data()), q, wsum + 16 * q);
    return true;
}

// wave 0 from the two records on: tables, Straus pass, + [w]B, [8], identity test
bool rows_check(const uint32_t rec_r[48], const uint32_t rec_a[48], const int* dr, const int* da,
                const uint32_t wsum[64]) {
    const rowf::RowConsts k = consts();
    std::vector<uint32_t> tab(2 * EACH_TABLE_WORDS);
    rowf::each_build_table(rec_r, tab.data(), k);
    rowf::each_build_table(rec_a, tab.data() + EACH_TABLE_WORDS, k);
    const rowf::RowP3 d = rowf::each_straus(tab.data(), tab.data() + EACH_TABLE_WORDS, dr, da, k);
    uint32_t out[48];
    rowf::each_finish(d, wsum, out, k);
    return each_is_identity(out);
}

// a cached row-form entry (64 words) as the lane code's ge_cached
ge_cached cached_of_rows(const uint32_t e[64]) {
    return ge_cached{fe_from_limbs16(e), fe_from_limbs16(e + 16), fe_from_limbs16(e + 48), fe_from_limbs16(e + 32)};
}
ge_cached cached_of_entry(const uint32_t* e) {
    return ge_cached{load_fe(e), load_fe(e + 10), load_fe(e + 20), load_fe(e + 30)};
}
// the same point: (Y+X : Y-X : 2Z : 2dT) are proportional (2Z of a table entry is never 0)
bool cached_same(const ge_cached& a, const ge_cached& b) {
    return fe_eq(fe_mul(a.YpX, b.Z2), fe_mul(b.YpX, a.Z2)) && fe_eq(fe_mul(a.YmX, b.Z2), fe_mul(b.YmX, a.Z2)) &&
           fe_eq(fe_mul(a.T2d, b.Z2), fe_mul(b.T2d, a.Z2)) && !fe_is_zero(fe_carry(a.Z2)) &&
           !fe_is_zero(fe_carry(b.Z2));
}

// [x]B by the lane code's fixed-base pass
ge_p3 base_mul(const uint32_t x[8]) {
    const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return straus_sB_minus_kA(zero, x, nullptr, btab(), btab() + BASE_TABLE_WORDS);
}

}  // namespace

extern "C" {

// k_ed_each_row over n signatures: pk n x 32, sig n x 64, message i = msg[off[i] .. off[i] + len[i]);
// verdict[i] = 1 accept, 0 reject.  Returns 0, or -1 when a digit would index past a table.
int he_each_verify(uint32_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, const uint64_t* off,
                   const uint32_t* len, uint8_t* verdict) {
    for (uint32_t i = 0; i < n; i++) {  // one workgroup
        const uint8_t* A = pk + 32 * (size_t)i;
        const uint8_t* R = sig + 64 * (size_t)i;
        const uint8_t* enc[4] = {R, A, R, A};
        uint32_t rec[4 * 48];
        bool ok[4];
        rows_decompress(enc, rec, ok);
        uint32_t Aw[8], Rw[8], Sw[8];
        words(A, Aw);
        words(R, Rw);
        words(R + 32, Sw);
        std::vector<uint8_t> m(len[i] + 64, 0);  // (the hash over-reads past a message, masked)
        if (len[i]) std::memcpy(m.data(), msg + off[i], len[i]);
        int dr[EACH_DIGITS], da[EACH_DIGITS], dw[COMB_TABLES];
        const bool hok = each_scalars(Aw, Rw, Sw, m.data(), len[i], dr, da, dw);
        uint32_t wsum[64];
        if (!comb_sum(dw, wsum)) return -1;
        verdict[i] = (rows_check(rec, rec + 48, dr, da, wsum) && hok && ok[0] && ok[1]) ? 1 : 0;
    }
    return 0;
}

// k_ed_each_row_msm over n signatures: what k_msm_prep leaves after a batch MSM over per-signature
// keys -- every A's and R's point record (msm_store_point of the decompressed point, word 31 = 1
// when the encoding does not decode), k_i (sc_reduce512_fold of the challenge hash) and the s < l
// flag -- then the kernel's reuse form: the records converted to row limbs (each_record_coord), k
// loaded instead of hashed.
int he_each_verify_msm(uint32_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, const uint64_t* off,
                       const uint32_t* len, uint8_t* verdict) {
    for (uint32_t i = 0; i < n; i++) {
        uint32_t Aw[8], Rw[8], Sw[8], k[8], hw[16];
        words(pk + 32 * (size_t)i, Aw);
        words(sig + 64 * (size_t)i, Rw);
        words(sig + 64 * (size_t)i + 32, Sw);
        std::vector<uint8_t> m(len[i] + 64, 0);
        if (len[i]) std::memcpy(m.data(), msg + off[i], len[i]);
        // the prep
        uint32_t rec[2][MSM_PT_WORDS];
        const uint32_t* enc[2] = {Rw, Aw};
        for (int p = 0; p < 2; p++) {
            ge_p3 P;
            const bool ok = ge_decompress(enc[p], P);
            msm_store_point(rec[p], P);
            rec[p][MSM_PT_WORDS - 1] = ok ? 0u : 1u;
        }
        challenge_hash_words(Rw, Aw, m.data(), len[i], hw);
        sc_reduce512_fold(hw, k);
        const uint32_t flags = sc_is_canonical(Sw) ? FLAG_S_OK : 0u;
        // the pass
        uint32_t rows[2 * 48];
        for (int p = 0; p < 2; p++)
            for (int c = 0; c < 3; c++) each_record_coord(rec[p], c, rows + 48 * p + 16 * c);
        const uint32_t dec = (rec[0][MSM_PT_WORDS - 1] == 0u ? 1u : 0u) | (rec[1][MSM_PT_WORDS - 1] == 0u ? 2u : 0u);
        const bool sok = (flags & FLAG_S_OK) != 0u;
        int dr[EACH_DIGITS], da[EACH_DIGITS], dw[COMB_TABLES];
        each_split_digits(k, Sw, sok, dr, da, dw);
        uint32_t wsum[64];
        if (!comb_sum(dw, wsum)) return -1;
        verdict[i] = (rows_check(rows, rows + 48, dr, da, wsum) && sok && dec == 3u) ? 1 : 0;
    }
    return 0;
}

// the lane pipeline's verdict of one signature (ed25519_verify_lane: lane_straus_check_half)
int he_each_lane_verify(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint32_t len) {
    uint32_t Aw[8], Rw[8], Sw[8];
    words(pk, Aw);
    words(sig, Rw);
    words(sig + 32, Sw);
    std::vector<uint8_t> m(len + 64, 0);
    if (len) std::memcpy(m.data(), msg, len);
    std::vector<uint32_t> tbl(LANE_SCRATCH_WORDS);
    return ed25519_verify_lane(Aw, Rw, Sw, m.data(), len, tbl.data(), btab()) ? 1 : 0;
}

// The table of the point encoded at enc, built on rows from its row decompression, against
// build_a_table's entry by entry (bit j of the result: entry j differs), then every signed digit
// -8..8 as each_entry loads it against the lane code's conditional negation (bit 9 + d + 8).
// -1: the encoding does not decode (on either side, or the two sides disagree: -2).
int he_each_table_check(const uint8_t* enc32) {
    uint32_t w[8];
    words(enc32, w);
    ge_p3 P;
    const bool lok = ge_decompress(w, P);
    const uint8_t* enc[4] = {enc32, enc32, enc32, enc32};
    uint32_t rec[4 * 48];
    bool ok[4];
    rows_decompress(enc, rec, ok);
    if (lok != ok[0] || ok[0] != ok[1]) return -2;
    if (!lok) return -1;
    const rowf::RowConsts k = consts();
    std::vector<uint32_t> tab(EACH_TABLE_WORDS), ltab(A_TABLE_ENTRIES * CACHED_ENTRY_WORDS);
    rowf::each_build_table(rec + 48, tab.data(), k);  // (row 1's record, as the kernel takes A's)
    build_a_table(P, ltab.data());
    int bad = 0;
    for (int j = 0; j < EACH_ENTRIES; j++)
        if (!cached_same(cached_of_rows(tab.data() + 64 * j), cached_of_entry(ltab.data() + CACHED_ENTRY_WORDS * j)))
            bad |= 1 << j;
    for (int d = -8; d <= 8; d++) {
        const rowf::V v = rowf::each_entry(tab.data(), d, k);
        const ge_cached want =
            ge_cached_cneg(cached_of_entry(ltab.data() + CACHED_ENTRY_WORDS * (d < 0 ? -d : d)), d < 0);
        if (!cached_same(cached_of_rows(v.l), want)) bad |= 1 << (9 + d + 8);
    }
    return bad;
}

// A challenge scalar fed straight to the split and the loop.  With A = [a]B, R = [r]B and
// s = r + k a (+ 1 when spoil) the equation [s]B = R + [k]A holds for the forced k (k < l), or
// misses by B.  out[0]: the row form's verdict; out[1]: lane_straus_check_half's; out[2]: v < 0;
// out[3]: zero digits among the 66 of R's and A's coefficients; out[4]: 1 when a comb digit was
// out of range.
int he_each_forced_k(const uint8_t* k32, const uint8_t* a32, const uint8_t* r32, int spoil, int32_t out[5]) {
    uint32_t k[8], a[8], r[8], ka[8], s[8];
    words(k32, k);
    words(a32, a);
    words(r32, r);
    const ge_p3 A = base_mul(a), R = base_mul(r);
    sc_mul(k, a, ka);
    sc_add(ka, r, s);
    if (spoil) {
        const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
        uint32_t t[8];
        sc_add(s, one, t);
        std::memcpy(s, t, sizeof(s));
    }
    int dr[EACH_DIGITS], da[EACH_DIGITS], dw[COMB_TABLES];
    each_split_digits(k, s, true, dr, da, dw);
    uint32_t u[4], m[4];
    bool vneg;
    sc_half_split(k, u, m, vneg);
    out[2] = vneg ? 1 : 0;
    out[3] = 0;
    for (int i = 0; i < EACH_DIGITS; i++) out[3] += (dr[i] == 0) + (da[i] == 0);
    uint32_t wsum[64], rec_r[48], rec_a[48];
    out[4] = comb_sum(dw, wsum) ? 0 : 1;
    if (out[4]) return -1;
    record_of(R, rec_r);
    record_of(A, rec_a);
    out[0] = rows_check(rec_r, rec_a, dr, da, wsum) ? 1 : 0;
    std::vector<uint32_t> tbl(LANE_SCRATCH_WORDS);
    build_a_table(A, tbl.data());
    build_a_table(R, tbl.data() + R_ENTRY * CACHED_ENTRY_WORDS);
    out[1] = lane_straus_check_half(k, s, tbl.data(), btab()) ? 1 : 0;
    return 0;
}

}  // extern "C"
