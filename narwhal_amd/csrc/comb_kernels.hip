// comb_kernels.hip -- per-signature comb verification of registered-key batches above TINY_MAX
// (gfx950).  The equation and the tables are k_ed_tiny's (tiny_kernels.hip): signature i is
// accepted iff [8] R = [8]([s]B - [k]A), [s]B - [k]A summed from B's fixed-base comb and the
// registered key's (no doubling chain, no random coefficients, no fallback pass: the verdict bits
// are the exact ZIP-215 verdicts).  k_ed_tiny spends a CU on a signature; this kernel is laid out
// for throughput, COMB_G = 4 signatures a workgroup of five waves:
//   wave 0       lanes 0..3 hash the four signatures (k = SHA-512(R || A || M) mod l, s < l, the
//                signed radix-16 digits of s and k into LDS); after the first barrier it
//                decompresses the four R's, one per 16-lane row (msm_kernels.hip row_decompress),
//                and doubles each three times (row doublings take the whole wave: one R at a time)
//   waves 1..4   one signature each, after the first barrier: lane j adds digit position j's
//                entries of both combs (comb.h comb_term), the 64 terms are summed by the six-level
//                tree of quad-lane additions in LDS (quad_p3_add), then three quad doublings
//   after the second barrier, lanes 0..3 of each comb wave form the four cross products of the
//   projective comparison and lane 0 ors the verdict bit into the accumulated words.
// The wave of the last signature to arrive collects the ceil(n / 64) verdict words, writes the
// batch verdict into the lane's polled host word and leaves the workspace zeroed.
#include "comb.h"

using namespace nwv;

struct CombArgs {
    const uint8_t* pk;      // [n][32] each signature's key (the hash's A bytes)
    const uint8_t* sig;     // [n][64]
    const uint8_t* msg;     // message arena; off[n] / len[n] index it
    const uint64_t* off;
    const uint32_t* len;
    const uint32_t* kc;     // key cache records: word MSM_PT_WORDS - 1 of a slot = A did not decode
    const uint32_t* combs;  // per-key comb tables (COMB_WORDS words each)
    const uint32_t* bcomb;  // B's comb table
    const uint32_t* kslot;  // [n] signature i's key cache slot
    const uint32_t* cidx;   // [n] signature i's comb table
    // workspace, zero between calls: ws[0] arrivals, acc[ceil(n / 64)] accumulated verdict bits
    // (the last wave resets both); results: ws[1] (hseq << 2) | batch verdict (1 accept, 2 reject),
    // bits[ceil(n / 64)]
    uint32_t* ws;
    unsigned long long* acc;
    unsigned long long* bits;
    uint32_t* hword;        // the lane's polled host word or null: [0] the same word as ws[1]
    uint32_t n, hseq;
};

static constexpr int COMB_WAVES = COMB_G + 1;
// FUSED (k_ed_comb_fused, a typed call with the setting nwv_set_typed_fused): signature i's message
// is what typed_message (comb.h) makes of f.src[i], as in k_ed_tiny_fused.  The unfused
// instantiation is k_ed_comb as it was.
template <bool FUSED>
__device__ __forceinline__ void ed_comb_block(const CombArgs& a, const TypedFusedArgs& f) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ uint32_t rsh[COMB_G * 48];            // wave 0's rows (48 words each), then the cross products
    __shared__ uint32_t r8sh[48];                    // [8] R of one row on its way to ten-limb form
    __shared__ uint32_t rrec[COMB_G * 32];           // per row [8] R: X | Y | Z; word 31: 1 = R does not decode
    __shared__ int dg[COMB_G][2][COMB_TABLES];       // digits of s and of k
    __shared__ uint32_t hok[COMB_G];                 // s < l
    __shared__ uint32_t pts[COMB_G * 64 * P3_WORDS];  // each comb wave's 64 terms, summed in place
    __shared__ uint32_t dmsg[FUSED ? COMB_G * TYPED_DBUF_WORDS : 1];  // FUSED: each hashing lane's digest
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
    const uint32_t base = blockIdx.x * COMB_G;  // signature workgroups: ceil(n / COMB_G); base < n
    if (wv == 0 && lane < COMB_G) {
        const uint32_t i = base + lane;
        if (i < a.n) {
            uint32_t Aw[8], Rw[8], Sw[8];
            msm_load8(a.pk + 32 * (size_t)i, Aw);
            msm_load8(a.sig + 64 * (size_t)i, Rw);
            msm_load8(a.sig + 64 * (size_t)i + 32, Sw);
            const uint8_t* mp = a.msg + a.off[i];
            uint32_t ml = a.len[i];
            if (FUSED) mp = typed_message(f.src[i], mp, ml, dmsg + TYPED_DBUF_WORDS * lane, f.short_out);
            hok[lane] = comb_scalars(Aw, Rw, Sw, mp, ml, dg[lane][0], dg[lane][1]) ? 1u : 0u;
        }
    }
    __syncthreads();  // digits in LDS
    const int g = wv - 1;                                // comb wave g's signature
    const uint32_t i = base + (uint32_t)(wv ? g : 0);
    const bool live = wv > 0 && i < a.n;                 // wave-uniform
    uint32_t* mine = pts + 64 * P3_WORDS * (wv ? g : 0);
    if (wv == 0) {
        const int row = lane >> 4, limb = lane & 15;
        const uint32_t r = base + (uint32_t)row;  // rows past the end decompress y = 0; nobody reads them
        uint32_t y16 = 0u;
        if (r < a.n) y16 = reinterpret_cast<const uint16_t*>(a.sig + 64 * (size_t)r)[limb];
        uint32_t* sh = rsh + 48 * row;
        const bool ok = row_decompress(y16, lane, row, limb, sh);
        if (limb == 0) rrec[32 * row + 31] = ok ? 0u : 1u;
        // [8] R, one R after the other: a row doubling is a whole-wave operation (the four rows
        // square X, Y, Z and X + Y of ONE point), so every row loads row q's record and the wave
        // doubles it three times from (2x : 2y : 2), k_ed_tiny's form (one multiply latency each)
        rowf::RowConsts k = rowf::row_consts();
        k.rot = 1;
#pragma unroll 1
        for (int q = 0; q < COMB_G && base + (uint32_t)q < a.n; q++) {
            const uint32_t ypx = rsh[48 * q + limb], ymx = rsh[48 * q + 16 + limb];
            rowf::RowP3 d{rowf::carry32(rowf::sub(ypx, ymx, k), k), rowf::carry32(ypx + ymx, k),
                          rowf::sel(rowf::limb_is(0), 0u, 2u), 0u};
#pragma unroll 1
            for (int r2 = 0; r2 < 3; r2++) d = rowf::row_dbl(d, k);
            rowf::lds_order();
            if (row == 0) {
                r8sh[limb] = d.X;
                r8sh[16 + limb] = d.Y;
                r8sh[32 + limb] = d.Z;
            }
            rowf::lds_order();
            if (lane < 3) store_fe(&rrec[32 * q + 10 * lane], fe_from_limbs16(r8sh + 16 * lane));  // X | Y | Z
            rowf::lds_order();
        }
    } else if (live) {
        const uint32_t* ct = a.combs + (size_t)COMB_WORDS * a.cidx[i];
        store_p3(mine + P3_WORDS * lane, comb_term(a.bcomb, ct, lane, dg[g][0][lane], dg[g][1][lane]));
        rowf::lds_order();
        // the 64 terms summed by lane quads, a tree in place: level o adds slot i + o into i
        const int q = lane & 3;
#pragma unroll 1
        for (int o = 1; o < 64; o <<= 1) {
#pragma unroll 1
            for (int s = lane >> 2; s < 32 / o; s += 16) quad_p3_add(mine, 2 * o * s, o, q);
            rowf::lds_order();
        }
        // [8] P as three doublings on the first quad (an addition of the slot to itself)
        if (lane < 4)
#pragma unroll 1
            for (int r = 0; r < 3; r++) {
                quad_p3_add(mine, 0, 0, lane);
                rowf::lds_order();
            }
    }
    __syncthreads();  // every [8] R and [8]([s]B - [k]A) done
    uint32_t last = 0u;
    if (live) {
        // the four cross products on lanes 0..3 into wave 0's row (free after the barrier)
        uint32_t* x = rsh + 48 * g;
        if (lane < 4) comb_cross(mine, rrec + 32 * g, lane, x + 8 * lane);
        rowf::lds_order();
        if (lane == 0) {
            const bool aok = a.kc[(size_t)KC_SLOT_WORDS * a.kslot[i] + MSM_PT_WORDS - 1] == 0u;
            const bool ok = comb_cross_equal(x) && aok && hok[g] && rrec[32 * g + 31] == 0u;
            if (ok) atomicOr(a.acc + (i >> 6), 1ull << (i & 63));
            __threadfence();
            last = atomicAdd(a.ws, 1u) == a.n - 1 ? 1u : 0u;
        }
    }
    last = __shfl(last, 0);
    if (last) {  // (wave-uniform) every signature's verdict bit is in
        __threadfence();
        const uint32_t words = (a.n + 63) / 64;
        bool all = true;
        for (uint32_t w = lane; w < words; w += 64) {
            const unsigned long long b = atomicExch(a.acc + w, 0ull);
            const uint32_t rem = a.n - 64 * w;
            all = all && b == (rem >= 64 ? ~0ull : ((1ull << rem) - 1ull));
            a.bits[w] = b;
        }
        const bool every = __all(all ? 1 : 0) != 0;
        if (lane == 0) {
            a.ws[0] = 0u;
            const uint32_t v = (a.hseq << 2) | (every ? 1u : 2u);
            a.ws[1] = v;
            if (a.hword) __hip_atomic_store(a.hword, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
#endif
}

extern "C" __global__ void __launch_bounds__(64 * COMB_WAVES) k_ed_comb(CombArgs a) {
    ed_comb_block<false>(a, TypedFusedArgs{});
}
// A typed call above TINY_MAX in one launch: workgroups [0, f.sig_blocks) are k_ed_comb's over
// typed messages, the workgroups behind them hash the side preimages (k_ed_tiny_fused's layout).
extern "C" __global__ void __launch_bounds__(64 * COMB_WAVES) k_ed_comb_fused(CombArgs a, TypedFusedArgs f, B2SideArgs s) {
    if (blockIdx.x >= f.sig_blocks) {
        b2_side_block(s, blockIdx.x - f.sig_blocks);
        return;
    }
    ed_comb_block<true>(a, f);
}

// ---- the comb check as a per-signature pass behind a rejected batch MSM (k_ed_comb_pass) ----
// The verdict is k_ed_comb's, signature by signature; the layout is for passes of thousands of
// signatures.  COMB_PASS_G = 16 signatures a workgroup, three roles on waves of their own:
//   wave 0            lanes 0..15 hash one signature each (comb.h comb_scalars: k, s < l, the
//                     digits of s and k into LDS)
//   waves 1..4        decompress four R's each, one per 16-lane row, from the first instruction
//                     (nothing here waits for the hash), then double each three times by rows
//   the sum waves     after the one barrier: L lanes a signature, lane t walks digit positions
//                     64 t / L .. 64 (t + 1) / L - 1 of both combs with mixed additions
//                     (comb_lane_sum; a zero digit adds the neutral record, no branch), the lane
//                     sums join in log2 L levels through lane shuffles (comb_join), and the
//                     signature's first lane doubles three times, compares with [8] R
//                     (comb_pass_equal) and ors the verdict bit into the batch's verdict words
// L = 4: one sum wave (six waves a workgroup); L = 16: four (nine waves).  LDS holds the digits,
// the decompression rows and the [8] R records only: the partial sums stay in registers.
// The host zeroes the verdict words on the stream before the launch: a signature whose workgroup
// never ran stays rejected.
struct CombPassArgs {
    const uint8_t* pk;      // [n][32] each signature's key (the hash's A bytes)
    const uint8_t* sig;     // [n][64]
    const uint8_t* msg;     // message arena; off[n] / len[n] index it
    const uint64_t* off;
    const uint32_t* len;
    const uint32_t* kc;     // key cache records: word MSM_PT_WORDS - 1 of a slot = A did not decode
    const uint32_t* combs;  // per-key comb tables (COMB_WORDS words each)
    const uint32_t* bcomb;  // B's comb table
    const uint32_t* kslot;  // [n] signature i's key cache slot
    const uint32_t* cidx;   // [n] signature i's comb table
    unsigned long long* verdict;  // [ceil(n / 64)] zero at launch; bit i = signature i accepted
    uint32_t n;
};

static constexpr int COMB_PASS_DEC = COMB_PASS_G / 4;  // decompression waves
template <int L>
struct CombPassShape {
    static constexpr int SUM = COMB_PASS_G * L / 64;  // sum waves
    static constexpr int WAVES = 1 + COMB_PASS_DEC + SUM;
};

template <int L>
__device__ __forceinline__ void comb_pass_block(const CombPassArgs& a) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int G = COMB_PASS_G, DEC = COMB_PASS_DEC;
    __shared__ uint32_t rsh[G * 48];               // four rows (48 words each) a decompression wave
    __shared__ uint32_t r8sh[DEC * 48];            // [8] R of one row on its way to ten-limb form
    __shared__ uint32_t rrec[G * 32];              // per signature [8] R: X | Y | Z; word 31: 1 = R does not decode
    __shared__ int dg[G][2][COMB_TABLES];          // digits of s and of k
    __shared__ uint32_t hok[G];                    // s < l
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
    const uint32_t base = blockIdx.x * G;  // grid = ceil(n / G); base < n
    const int cnt = (int)(a.n - base < (uint32_t)G ? a.n - base : (uint32_t)G);  // live signatures
    if (wv == 0) {
        if (lane < cnt) {
            const uint32_t i = base + lane;
            uint32_t Aw[8], Rw[8], Sw[8];
            msm_load8(a.pk + 32 * (size_t)i, Aw);
            msm_load8(a.sig + 64 * (size_t)i, Rw);
            msm_load8(a.sig + 64 * (size_t)i + 32, Sw);
            hok[lane] = comb_scalars(Aw, Rw, Sw, a.msg + a.off[i], a.len[i], dg[lane][0], dg[lane][1]) ? 1u : 0u;
        }
    } else if (wv <= DEC) {
        const int first = 4 * (wv - 1);  // the wave's rows hold signatures first .. first + 3
        if (first < cnt) {               // (wave-uniform)
            const int row = lane >> 4, limb = lane & 15;
            uint32_t y16 = 0u;  // rows past the end decompress y = 0; nobody reads them
            if (first + row < cnt) y16 = reinterpret_cast<const uint16_t*>(a.sig + 64 * (size_t)(base + first + row))[limb];
            uint32_t* wsh = rsh + 192 * (wv - 1);
            const bool ok = row_decompress(y16, lane, row, limb, wsh + 48 * row);
            if (limb == 0) rrec[32 * (first + row) + 31] = ok ? 0u : 1u;
            // [8] R, one R after the other, as k_ed_comb's wave 0 does: every row loads row q's
            // record and the wave doubles it three times from (2x : 2y : 2)
            rowf::RowConsts k = rowf::row_consts();
            k.rot = 1;
            uint32_t* w8 = r8sh + 48 * (wv - 1);
#pragma unroll 1
            for (int q = 0; q < 4 && first + q < cnt; q++) {
                const uint32_t ypx = wsh[48 * q + limb], ymx = wsh[48 * q + 16 + limb];
                rowf::RowP3 d{rowf::carry32(rowf::sub(ypx, ymx, k), k), rowf::carry32(ypx + ymx, k),
                              rowf::sel(rowf::limb_is(0), 0u, 2u), 0u};
#pragma unroll 1
                for (int r2 = 0; r2 < 3; r2++) d = rowf::row_dbl(d, k);
                rowf::lds_order();
                if (row == 0) {
                    w8[limb] = d.X;
                    w8[16 + limb] = d.Y;
                    w8[32 + limb] = d.Z;
                }
                rowf::lds_order();
                if (lane < 3) store_fe(&rrec[32 * (first + q) + 10 * lane], fe_from_limbs16(w8 + 16 * lane));  // X | Y | Z
                rowf::lds_order();
            }
        }
    }
    __syncthreads();  // digits and every [8] R in LDS
    if (wv > DEC) {
        constexpr int P = COMB_TABLES / L;  // positions a lane
        const int grp = (wv - DEC - 1) * (64 / L) + lane / L, sub = lane % L;
        // lanes of a signature past the end run the last live one's arithmetic (every read stays
        // in bounds, the wave stays uniform) and store nothing
        const int gl = grp < cnt ? grp : cnt - 1;
        const uint32_t i = base + (uint32_t)gl;
        const uint32_t* ct = a.combs + (size_t)COMB_WORDS * a.cidx[i];
        ge_p3 S = comb_lane_sum(a.bcomb, ct, P * sub, P, dg[gl][0] + P * sub, dg[gl][1] + P * sub);
#pragma unroll 1
        for (int o = 1; o < L; o <<= 1) {
            // every lane adds lane + o's sum; those of lanes t = 0 mod 2 o are the tree's
            ge_p3 T;
            for (int q = 0; q < 10; q++) {
                T.X.v[q] = __shfl(S.X.v[q], (lane + o) & 63);
                T.Y.v[q] = __shfl(S.Y.v[q], (lane + o) & 63);
                T.Z.v[q] = __shfl(S.Z.v[q], (lane + o) & 63);
                T.T.v[q] = __shfl(S.T.v[q], (lane + o) & 63);
            }
            S = comb_join(S, T);
        }
        const bool eq = comb_pass_equal(S, rrec + 32 * gl);
        if (sub == 0 && grp < cnt) {
            const bool aok = a.kc[(size_t)KC_SLOT_WORDS * a.kslot[i] + MSM_PT_WORDS - 1] == 0u;
            if (eq && aok && hok[gl] && rrec[32 * gl + 31] == 0u) atomicOr(a.verdict + (i >> 6), 1ull << (i & 63));
        }
    }
#endif
}

extern "C" __global__ void __launch_bounds__(64 * CombPassShape<4>::WAVES) k_ed_comb_pass4(CombPassArgs a) {
    comb_pass_block<4>(a);
}
extern "C" __global__ void __launch_bounds__(64 * CombPassShape<16>::WAVES) k_ed_comb_pass16(CombPassArgs a) {
    comb_pass_block<16>(a);
}
