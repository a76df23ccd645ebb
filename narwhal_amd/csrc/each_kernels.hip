// each_kernels.hip -- one-launch per-signature verification over keys that have no comb table
// (gfx950): nwv_ed25519_verify_each and the pass that names the bad set after a batch MSM rejects,
// for small calls.  The lane pipeline (ed25519_kernels.hip: k_ed_hash, k_ed_points, k_ed_straus)
// puts a signature on a lane -- tables in HBM, a 132-doubling chain of lane-local multiplies --
// which fills the chip at 65,536 signatures and leaves it idle at 1,024.  Here a signature takes a
// workgroup of two waves (grid = n, k_ed_tiny's layout) and the same check, on half-size scalars
// (each.h), runs on 16-lane rows:
//   wave 0   R on row 0 and A on row 1 decompressed side by side (msm_kernels.hip row_decompress;
//            rows 2 and 3 duplicate them), their tables 0..8 R and 0..8 A built in LDS in cached
//            row form (positive multiples only: a negative digit swaps rows 0 and 1 of the entry
//            and negates row 2 as it is loaded), then, once wave 1's digits are in, the Straus
//            pass: 33 digit positions of four row doublings and two cached additions
//   wave 1   lane 0: k = SHA-512(R || A || M) mod l, s < l, the half-size split, w = m s mod l and
//            the digits; then, while wave 0 runs its chain, all 64 lanes sum [w]B from B's comb
//            (one entry a lane, the six-level tree of quad-lane additions, as k_ed_tiny sums
//            [s]B) and lanes 0..3 leave the sum in LDS in cached row form
//   wave 0   adds [w]B, doubles three times and lane 0 tests the identity on canonical limbs; the
//            verdict bit is or-ed into the call's verdict words (zeroed on the stream beforehand)
// Control flow is wave-uniform apart from the Euclid's iteration count on wave 1's lane 0.
//
// The reuse form, k_ed_each_row_msm, is the pass after a rejected batch MSM over per-signature
// keys: k_msm_prep left every R's and A's record in m_pts (y+x | y-x | 2dxy, word 31 = 1 when the
// encoding does not decode), k_i in kbuf and the s < l flag in flags, so wave 0 converts the two
// records to row limbs instead of decompressing (lanes 0..2 of rows 0 and 1, one coordinate each)
// and wave 1's lane 0 loads k instead of hashing -- what k_ed_points_msm does for the lane pipeline.
//
// This file is part of nwv_host.hip's translation unit and comes after msm_kernels.hip there: it
// uses that file's device-only row_decompress, quad_p3_add and msm_load8.
#include "each.h"

using namespace nwv;

struct EachArgs {
    const uint8_t* pk;      // [n][32]
    const uint8_t* sig;     // [n][64]
    const uint8_t* msg;     // message arena; off[n] / len[n] index it
    const uint64_t* off;
    const uint32_t* len;
    const uint32_t* bcomb;  // B's comb table
    unsigned long long* verdict;  // ceil(n / 64) words, zero at launch: bit i % 64 of word i / 64
    // the reuse form only: the rejected MSM's point records (A_i at record i, R_i at na + 1 + i),
    // its k_i (8 words each) and its flags (FLAG_S_OK)
    const uint32_t* pts;
    const uint32_t* kbuf;
    const uint32_t* flags;
    uint32_t na;
};

static constexpr int EACH_WAVES = 2;
template <bool MSM>
__device__ __forceinline__ void each_row_body(const EachArgs& a) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ uint32_t rsh[4 * 48];                 // wave 0's rows (48 words each), then X | Y | Z of the result
    __shared__ uint32_t tab[2 * EACH_TABLE_WORDS];   // 0..8 R, then 0..8 A
    __shared__ int dg[2][EACH_DIGITS];               // digits of R's and of A's coefficient, top first
    __shared__ int dw[COMB_TABLES];                  // comb digits of w
    __shared__ uint32_t hok, dec;                    // s < l; bit 0: R decodes, bit 1: A decodes
    __shared__ uint32_t pts[64 * P3_WORDS];          // the 64 comb terms, summed in place
    __shared__ uint32_t wsum[64];                    // [w]B in cached row form
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
    const uint32_t i = blockIdx.x;  // this workgroup's signature (grid = n)
    rowf::RowConsts k = rowf::row_consts();
    k.rot = 1;
    if (wv == 0) {
        const int row = lane >> 4, limb = lane & 15;
        if (MSM) {
            const uint32_t* er = a.pts + (size_t)MSM_PT_WORDS * ((size_t)a.na + 1 + i);
            const uint32_t* ea = a.pts + (size_t)MSM_PT_WORDS * i;
            if (row < 2 && limb < 3) each_record_coord(row ? ea : er, limb, rsh + 48 * row + 16 * limb);
            if (lane == 0) dec = (er[MSM_PT_WORDS - 1] == 0u ? 1u : 0u) | (ea[MSM_PT_WORDS - 1] == 0u ? 2u : 0u);
            rowf::lds_order();
        } else {
            // rows 0 and 2 decompress R, rows 1 and 3 A (the row products are wave-wide anyway)
            const uint8_t* enc = (row & 1) ? a.pk + 32 * (size_t)i : a.sig + 64 * (size_t)i;
            const uint32_t y16 = reinterpret_cast<const uint16_t*>(enc)[limb];
            const bool ok = row_decompress(y16, lane, row, limb, rsh + 48 * row);
            const unsigned long long okb = __ballot(ok);
            if (lane == 0) dec = (uint32_t)(okb & 1u) | ((uint32_t)(okb >> 16) & 1u) << 1;
        }
        rowf::each_build_table(rsh, tab, k);
        rowf::each_build_table(rsh + 48, tab + EACH_TABLE_WORDS, k);
    } else {
        if (lane == 0) {
            uint32_t Aw[8], Rw[8], Sw[8];
            msm_load8(a.sig + 64 * (size_t)i + 32, Sw);
            if (MSM) {
                uint32_t k[8];
#pragma unroll
                for (int q = 0; q < 8; q++) k[q] = a.kbuf[8 * (size_t)i + q];
                const bool sok = (a.flags[i] & FLAG_S_OK) != 0u;
                each_split_digits(k, Sw, sok, dg[0], dg[1], dw);
                hok = sok ? 1u : 0u;
            } else {
                msm_load8(a.pk + 32 * (size_t)i, Aw);
                msm_load8(a.sig + 64 * (size_t)i, Rw);
                hok = each_scalars(Aw, Rw, Sw, a.msg + a.off[i], a.len[i], dg[0], dg[1], dw) ? 1u : 0u;
            }
        }
        rowf::lds_order();
    }
    __syncthreads();  // tables and digits in LDS
    rowf::RowP3 d{0u, 0u, 0u, 0u};
    if (wv == 0) {
        d = rowf::each_straus(tab, tab + EACH_TABLE_WORDS, dg[0], dg[1], k);
    } else {
        store_p3(pts + P3_WORDS * lane, each_comb_term(a.bcomb, lane, dw[lane]));
        rowf::lds_order();
        // the 64 terms summed by lane quads, a tree in place: level o adds slot i + o into i
        const int q = lane & 3;
#pragma unroll 1
        for (int o = 1; o < 64; o <<= 1) {
#pragma unroll 1
            for (int g = lane >> 2; g < 32 / o; g += 16) quad_p3_add(pts, 2 * o * g, o, q);
            rowf::lds_order();
        }
        if (lane < 4) each_cached_limbs(load_p3(pts), lane, wsum + 16 * lane);
        rowf::lds_order();
    }
    __syncthreads();  // [w]B in LDS
    if (wv == 0) {
        rowf::each_finish(d, wsum, rsh, k);
        if (lane == 0) {
            const bool ok = each_is_identity(rsh) && hok != 0u && dec == 3u;
            if (ok) atomicOr(a.verdict + (i >> 6), 1ull << (i & 63));
        }
    }
#endif
}
extern "C" __global__ void __launch_bounds__(64 * EACH_WAVES) k_ed_each_row(EachArgs a) { each_row_body<false>(a); }
extern "C" __global__ void __launch_bounds__(64 * EACH_WAVES) k_ed_each_row_msm(EachArgs a) { each_row_body<true>(a); }
