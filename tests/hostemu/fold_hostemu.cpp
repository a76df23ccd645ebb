// fold_hostemu.cpp -- TEST-ONLY host build (NWV_BOUNDS_CHECK) of the pieces of k_msm_prep's second
// trimming: the reduction mod l by folding (sc25519.h), the unreduced sums of z_i s_i and their one
// reduction per batch (msm.h msm_zs_partial / msm_zs_total), the digit recoding that walks the
// scalar's words in order (msm.h msm_recode_rows), and the decompression that parks u, v and u v^3
// in a stash across the power (ge25519.h ge_decompress_stash).  Never part of the product.
#define NWV_HD __host__ __device__ inline
#include <cstring>
#include <vector>

#include "../../narwhal_amd/csrc/msm.h"

using namespace nwv;

extern "C" {

// n values of 16 words: fold[i] = sc_reduce512_fold, barrett[i] = sc_reduce512
void he_fold_reduce512(uint32_t n, const uint32_t* x, uint32_t* fold, uint32_t* barrett) {
    for (uint32_t i = 0; i < n; i++) {
        sc_reduce512_fold(x + 16 * (size_t)i, fold + 8 * (size_t)i);
        sc_reduce512(x + 16 * (size_t)i, barrett + 8 * (size_t)i);
    }
}
// n values of 12 words: fold[i] = sc_reduce384_fold, barrett[i] = sc_reduce512 of the value
void he_fold_reduce384(uint32_t n, const uint32_t* x, uint32_t* fold, uint32_t* barrett) {
    for (uint32_t i = 0; i < n; i++) {
        uint32_t w[16] = {0};
        std::memcpy(w, x + 12 * (size_t)i, 48);
        sc_reduce384_fold(x + 12 * (size_t)i, fold + 8 * (size_t)i);
        sc_reduce512(w, barrett + 8 * (size_t)i);
    }
}
// n pairs (z: 4 words, b: 8 words): prod[i] = sc_mul_4x8 (12 words), a[i] = its sc_reduce384_fold,
// ref[i] = sc_mul of the zero-extended z and b
void he_fold_zmul(uint32_t n, const uint32_t* z, const uint32_t* b, uint32_t* prod, uint32_t* a, uint32_t* ref) {
    for (uint32_t i = 0; i < n; i++) {
        uint32_t z8[8] = {0};
        std::memcpy(z8, z + 4 * (size_t)i, 16);
        sc_mul_4x8(z + 4 * (size_t)i, b + 8 * (size_t)i, prod + 12 * (size_t)i);
        sc_reduce384_fold(prod + 12 * (size_t)i, a + 8 * (size_t)i);
        sc_mul(z8, b + 8 * (size_t)i, ref + 8 * (size_t)i);
    }
}
// a hash workgroup of nt lanes as msm_scalars_block sums it: lane t's product z_t s_t in row t of
// an LDS-like array (rows MSM_ZS_WORDS + 1 words apart), the twelve column sums, the carry -> out
// (MSM_PARTIAL_WORDS words)
void he_fold_partial(uint32_t nt, const uint32_t* z, const uint32_t* s, uint32_t* out) {
    std::vector<uint32_t> lds((size_t)nt * (MSM_ZS_WORDS + 1), 0xdeadbeefu);
    for (uint32_t t = 0; t < nt; t++) {
        uint32_t zs[MSM_ZS_WORDS];
        sc_mul_4x8(z + 4 * (size_t)t, s + 8 * (size_t)t, zs);
        for (int k = 0; k < MSM_ZS_WORDS; k++) lds[(size_t)t * (MSM_ZS_WORDS + 1) + k] = zs[k];
    }
    unsigned long long col[MSM_ZS_WORDS];
    for (int k = 0; k < MSM_ZS_WORDS; k++) {
        unsigned long long c = 0;
        for (uint32_t r = 0; r < nt; r++) c += lds[(size_t)r * (MSM_ZS_WORDS + 1) + k];
        col[k] = c;
    }
    msm_zs_partial(col, out);
}
// nblk partials (MSM_PARTIAL_WORDS words each) as msm_bterm combines them: the thirteen column sums,
// then msm_zs_total -> r = their sum mod l
void he_fold_total(uint32_t nblk, const uint32_t* partial, uint32_t* r) {
    unsigned long long col[MSM_PARTIAL_WORDS] = {0};
    for (uint32_t q = 0; q < nblk; q++)
        for (int k = 0; k < MSM_PARTIAL_WORDS; k++) col[k] += partial[MSM_PARTIAL_WORDS * (size_t)q + k];
    msm_zs_total(col, r);
}

// layout: z-only (msm_make_layout_z(c_lo)) or msm_make_layout2(c_lo, c_hi, narrow_top); returns
// nw (0: no such layout) and nw_z in *nw_z
int he_fold_layout(int c_lo, int c_hi, int narrow_top, int zonly, int* nw_z, uint8_t* width, uint16_t* pos) {
    MsmLayout L;
    if (!(zonly ? msm_make_layout_z(c_lo, L) : msm_make_layout2(c_lo, c_hi, L, narrow_top != 0))) return 0;
    *nw_z = L.nw_z;
    for (int w = 0; w < L.nw; w++) width[w] = L.width[w], pos[w] = L.pos[w];
    return L.nw;
}
// n scalars (8 words) over the layout's first nw windows (zrange: nw_z, else nw): fresh[i][w] by
// msm_recode_rows into a row-major digit array of np = n + 3 columns (column i + 1; the rest must
// stay untouched: returns 0 if not), old[i][w] by msm_recode.  Rows are MSM_MAX_WINDOWS apart.
int he_fold_recode(int c_lo, int c_hi, int narrow_top, int zonly, int zrange, uint32_t n, const uint32_t* s,
                   int16_t* fresh, int16_t* old) {
    MsmLayout L;
    if (!(zonly ? msm_make_layout_z(c_lo, L) : msm_make_layout2(c_lo, c_hi, L, narrow_top != 0))) return 0;
    const int nw = zrange ? L.nw_z : L.nw;
    const uint64_t np = (uint64_t)n + 3;
    const int16_t FILL = 0x7abc;
    std::vector<int16_t> rows((size_t)MSM_MAX_WINDOWS * np, FILL);
    for (uint32_t i = 0; i < n; i++) {
        msm_recode_rows(s + 8 * (size_t)i, L, nw, rows.data() + i + 1, np);
        msm_recode(s + 8 * (size_t)i, L, nw, [&](int w, int d) { old[(size_t)i * MSM_MAX_WINDOWS + w] = (int16_t)d; });
    }
    int ok = 1;
    for (int w = 0; w < MSM_MAX_WINDOWS; w++)
        for (uint64_t c = 0; c < np; c++) {
            const int16_t v = rows[(size_t)w * np + c];
            if (w < nw && c >= 1 && c <= n) fresh[(size_t)(c - 1) * MSM_MAX_WINDOWS + w] = v;
            else if (v != FILL) ok = 0;
        }
    return ok;
}

// n encodings: ok[i] / rec[i] (the 32-word MSM point record) by ge_decompress_stash with lane i's
// stash in a word-major array of 64 lanes, ok_ref / rec_ref by ge_decompress.  Returns 1 when
// every lane's stash words stayed inside its own column (the other lanes' words are untouched).
int he_fold_decompress(uint32_t n, const uint8_t* enc, uint8_t* ok, uint32_t* rec, uint8_t* ok_ref, uint32_t* rec_ref) {
    constexpr int LANES = 64;
    int clean = 1;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t w[8];
        std::memcpy(w, enc + 32 * (size_t)i, 32);
        std::vector<uint32_t> sh((size_t)LANES * MSM_STASH_WORDS, 0x5a5a5a5au);
        const uint32_t lane = i % LANES;
        ge_p3 P, Q;
        ok[i] = ge_decompress_stash<LANES>(w, sh.data() + lane, P) ? 1 : 0;
        ok_ref[i] = ge_decompress(w, Q) ? 1 : 0;
        msm_store_point(rec + (size_t)MSM_PT_WORDS * i, P);
        msm_store_point(rec_ref + (size_t)MSM_PT_WORDS * i, Q);
        for (size_t k = 0; k < sh.size(); k++)
            if (k % LANES != lane && sh[k] != 0x5a5a5a5au) clean = 0;
    }
    return clean;
}

}  // extern "C"
