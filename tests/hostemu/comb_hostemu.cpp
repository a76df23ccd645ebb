// comb_hostemu.cpp -- TEST-ONLY host build of the comb kernel's per-signature arithmetic
// (narwhal_amd/csrc/comb_kernels.hip k_ed_comb) with limb-bound assertions (NWV_BOUNDS_CHECK).
// The kernel's lane functions (comb.h: comb_scalars, comb_term, comb_cross, comb_cross_equal) and
// the row field code (fe_row.h on the emulated wave) run on the CPU, workgroup by workgroup as the
// kernel lays the work out: COMB_G signatures hashed side by side, their R's decompressed one per
// 16-lane row of one wave and then doubled three times each, each signature's 64 comb terms summed
// in the kernel's tree order, the projective comparison by its four cross products.  Never part
// of the product.
#define NWV_HD __host__ __device__ inline
#include <array>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../narwhal_amd/csrc/comb.h"
#include "../../narwhal_amd/csrc/fe_row.h"

using namespace nwv;

namespace {

void words(const uint8_t* p, uint32_t w[8]) { std::memcpy(w, p, 32); }

// One point's comb table (k_key_comb_fill / k_comb_table: entry 8 j + i - 1 = i 16^j P), filled
// entry by entry as the digits ask for them: q[j] = 16^j P by a chain of four doublings a table.
struct Comb {
    std::vector<uint32_t> e;
    std::vector<bool> have;
    std::vector<ge_p3> q;
    explicit Comb(const ge_p3& P) : e((size_t)COMB_WORDS, 0u), have(COMB_TABLES * COMB_ENTRIES, false) {
        q.push_back(P);
        for (int j = 1; j < COMB_TABLES; j++) q.push_back(p3_dbl_n(q.back(), 4));
    }
    // false: the digit is past the table
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
    static Comb* c = [] {
        uint32_t bw[8];
        ge_basepoint_words(bw);
        ge_p3 B;
        ge_decompress(bw, B);
        return new Comb(B);
    }();
    return *c;
}
// the key's table and whether the key decodes (an undecodable key gets the identity's table and
// fails on the key cache record's flag)
struct KeyComb {
    Comb comb;
    bool aok;
};
KeyComb& comb_of_key(const uint8_t* pk) {
    static std::map<std::array<uint8_t, 32>, KeyComb*> tabs;
    std::array<uint8_t, 32> k;
    std::memcpy(k.data(), pk, 32);
    auto it = tabs.find(k);
    if (it != tabs.end()) return *it->second;
    uint32_t w[8];
    words(pk, w);
    ge_p3 A;
    const bool aok = ge_decompress(w, A);
    if (!aok) A = ge_p3_identity();
    return *(tabs[k] = new KeyComb{Comb(A), aok});
}

// Wave 0 of the kernel on the emulated wave: row q decompresses encoding q (msm_kernels.hip
// row_decompress, the row products in the device's rotation form; the zero / sign tests lane-local
// as on lanes 0..2 of each row), then, one R after the other, every row loads the R's record and
// the wave doubles it three times from (2x : 2y : 2).  rrec: per row
// X | Y | Z of [8] R as ten-limb words and word 31 = 1 when the encoding does not decode.
void rows_mul8(const uint8_t* const enc[COMB_G], int cnt, uint32_t* rrec) {
    rowf::V y16;
    bool sign[4] = {false, false, false, false};
    for (int l = 0; l < 64; l++) {
        const int q = l >> 4, limb = l & 15;
        uint32_t v = 0;
        if (q < cnt) v = (uint32_t)enc[q][2 * limb] | ((uint32_t)enc[q][2 * limb + 1] << 8);
        if (limb == 15) {
            sign[q] = (v >> 15) != 0;
            v &= 0x7FFFu;
        }
        y16.l[l] = v;
    }
    rowf::RowConsts k = rowf::row_consts();
    k.rot = 1;
    rowf::V u, v, uv3, uv7, r, ri, c0, c1, c2;
    rowf::row_dec_pre(y16, k, u, v, uv3, uv7);
    const rowf::V pw = rowf::row_pow_p58(uv7, k);
    rowf::row_dec_mid(uv3, pw, u, v, k, r, ri, c0, c1, c2);
    auto limbs = [](const rowf::V& x, int q, uint32_t out[16]) {
        for (int i = 0; i < 16; i++) out[i] = x.l[16 * q + i];
    };
    bool ok[4];
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
    rowf::V two;
    for (int l = 0; l < 64; l++) two.l[l] = (l & 15) == 0 ? 2u : 0u;
    for (int q = 0; q < cnt; q++) {
        // a row doubling takes the whole wave: every row loads row q's record
        rowf::V yp, ym;
        for (int l = 0; l < 64; l++) {
            yp.l[l] = ypx.l[16 * q + (l & 15)];
            ym.l[l] = ymx.l[16 * q + (l & 15)];
        }
        rowf::RowP3 d{rowf::carry32(rowf::sub(yp, ym, k), k), rowf::carry32(yp + ym, k), two, rowf::bc(0)};
        for (int t = 0; t < 3; t++) d = rowf::row_dbl(d, k);
        uint32_t a[16];
        limbs(d.X, 0, a);
        store_fe(rrec + 32 * q, fe_from_limbs16(a));
        limbs(d.Y, 0, a);
        store_fe(rrec + 32 * q + 10, fe_from_limbs16(a));
        limbs(d.Z, 0, a);
        store_fe(rrec + 32 * q + 20, fe_from_limbs16(a));
        rrec[32 * q + 31] = ok[q] ? 0u : 1u;
    }
}

}  // namespace

extern "C" {

int he_comb_group() { return COMB_G; }

// k_ed_comb over n signatures: pk n x 32, sig n x 64, message i = msg[off[i] .. off[i] + len[i]);
// verdict[i] = 1 accept, 0 reject.  Returns 0, or -1 when a digit would index past a table.
int he_comb_verify(uint32_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, const uint64_t* off,
                   const uint32_t* len, uint8_t* verdict) {
    Comb& B = comb_of_b();
    for (uint32_t base = 0; base < n; base += COMB_G) {  // one workgroup
        const int cnt = (int)(n - base < (uint32_t)COMB_G ? n - base : COMB_G);
        int dg[COMB_G][2][COMB_TABLES];
        bool hok[COMB_G];
        const uint8_t* enc[COMB_G] = {nullptr, nullptr, nullptr, nullptr};
        for (int g = 0; g < cnt; g++) {  // wave 0, lanes 0..COMB_G - 1
            const uint32_t i = base + g;
            uint32_t Aw[8], Rw[8], Sw[8];
            words(pk + 32 * (size_t)i, Aw);
            words(sig + 64 * (size_t)i, Rw);
            words(sig + 64 * (size_t)i + 32, Sw);
            std::vector<uint8_t> m(len[i] + 64, 0);  // (the hash over-reads past a message, masked)
            if (len[i]) std::memcpy(m.data(), msg + off[i], len[i]);
            hok[g] = comb_scalars(Aw, Rw, Sw, m.data(), len[i], dg[g][0], dg[g][1]);
            enc[g] = sig + 64 * (size_t)i;
        }
        uint32_t rrec[COMB_G * 32] = {};
        rows_mul8(enc, cnt, rrec);  // wave 0 after the barrier
        for (int g = 0; g < cnt; g++) {  // comb wave g + 1
            const uint32_t i = base + g;
            KeyComb& A = comb_of_key(pk + 32 * (size_t)i);
            std::vector<uint32_t> pts((size_t)64 * P3_WORDS);
            for (int lane = 0; lane < 64; lane++) {
                if (!B.need(lane, dg[g][0][lane]) || !A.comb.need(lane, dg[g][1][lane])) return -1;
                store_p3(pts.data() + P3_WORDS * lane,
                         comb_term(B.e.data(), A.comb.e.data(), lane, dg[g][0][lane], dg[g][1][lane]));
            }
            // the kernel's tree: level o adds slot 2 o s + o into slot 2 o s (quad_p3_add runs
            // p3_add's field operations on the same operands), then three doublings of slot 0
            for (int o = 1; o < 64; o <<= 1)
                for (int s = 0; s < 32 / o; s++) {
                    uint32_t* L = pts.data() + (size_t)P3_WORDS * 2 * o * s;
                    store_p3(L, p3_add(load_p3(L), load_p3(L + (size_t)P3_WORDS * o)));
                }
            for (int r = 0; r < 3; r++) store_p3(pts.data(), p3_add(load_p3(pts.data()), load_p3(pts.data())));
            uint32_t x[32];
            for (int c = 0; c < 4; c++) comb_cross(pts.data(), rrec + 32 * g, c, x + 8 * c);
            verdict[i] = (comb_cross_equal(x) && A.aok && hok[g] && rrec[32 * g + 31] == 0u) ? 1 : 0;
        }
    }
    return 0;
}

}  // extern "C"
