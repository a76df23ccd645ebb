// fe25519.h -- GF(2^255-19) arithmetic for gfx950 VALU, radix 2^25.5 (ten 32-bit limbs).
//
// Replaces the field layer of curve25519-dalek-ng 4.1.1 (u64_backend, radix 2^51).  On CDNA4 the natural multiply is the
// 32x32->64 multiply-accumulate `v_mad_u64_u32`, so limbs are 26/25 bits wide and a
// product is 100 multiply-adds into ten 64-bit column accumulators.  Everything here is
// __host__ __device__ so a test-only host build (tests/hostemu) can run it with limb-bound
// assertions enabled (NWV_BOUNDS_CHECK); the product only runs it on the GPU.
//
// Magnitude discipline (m = max limb / 2^26 or 2^25):
//   "L"  carried output of mul/sq/carry: m <= 1.01
//   add(L, L) -> m <= 2.02      sub(L, L) = a + 2p - b -> m <= 3.02 (b must be L)
//   mul/sq inputs must have m <= 3.36 (19 * limb must fit 32 bits; column sums < 2^64)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef NWV_HD
#define NWV_HD __host__ __device__ __forceinline__
#endif

// Scheduling fence around every field multiply: hipcc otherwise interleaves the independent
// multiplies of a point formula (4-way ILP) and doubles the VGPR footprint; one multiply
// already carries ten independent accumulation chains, so occupancy is worth more.
#if defined(__HIP_DEVICE_COMPILE__)
#define NWV_SEQ() __builtin_amdgcn_sched_barrier(0)
#else
#define NWV_SEQ() ((void)0)
#endif

#ifdef NWV_BOUNDS_CHECK
#include <assert.h>
#define NWV_ASSERT(x) assert(x)
#else
#define NWV_ASSERT(x) ((void)0)
#endif

// host-emulation op counting (tests/hostemu, -DNWV_COUNT_OPS): algorithmic multiply counts
// per phase, the numerator of the VALU roofline in bench.py
#ifdef NWV_COUNT_OPS
extern unsigned long long nwv_count_mul, nwv_count_sq;
#define NWV_COUNT(x) (++(x))
#else
#define NWV_COUNT(x) ((void)0)
#endif

namespace nwv {

struct fe {
    uint32_t v[10];
};

static constexpr uint32_t M26 = (1u << 26) - 1;
static constexpr uint32_t M25 = (1u << 25) - 1;

NWV_HD constexpr int limb_bits(int i) { return (i & 1) ? 25 : 26; }

NWV_HD void fe_check(const fe& a, double m) {
#ifdef NWV_BOUNDS_CHECK
    for (int i = 0; i < 10; i++) NWV_ASSERT((double)a.v[i] <= m * (double)(1u << limb_bits(i)));
#else
    (void)a; (void)m;
#endif
}

NWV_HD fe fe_zero() { fe r; for (int i = 0; i < 10; i++) r.v[i] = 0; return r; }
NWV_HD fe fe_one() { fe r = fe_zero(); r.v[0] = 1; return r; }
NWV_HD fe fe_small(uint32_t x) { fe r = fe_zero(); r.v[0] = x; return r; }

NWV_HD fe fe_add(const fe& a, const fe& b) {
    fe r;
#pragma unroll
    for (int i = 0; i < 10; i++) r.v[i] = a.v[i] + b.v[i];
    return r;
}

// a - b + 2p; b must be carried (limb0 <= 2^27-38, others <= 2^(bits+1)-2)
NWV_HD fe fe_sub(const fe& a, const fe& b) {
    fe_check(b, 1.9);
    fe r;
    r.v[0] = a.v[0] + 0x7FFFFDAu - b.v[0];
#pragma unroll
    for (int i = 1; i < 10; i++) r.v[i] = a.v[i] + ((i & 1) ? 0x3FFFFFEu : 0x7FFFFFEu) - b.v[i];
    return r;
}
NWV_HD fe fe_neg(const fe& b) { return fe_sub(fe_zero(), b); }

// weak reduction of 32-bit limbs (inputs up to ~2^31): every limb ends below 2^26/2^25
// except limb 1, which may exceed 2^25 by < 2^7.
NWV_HD fe fe_carry(const fe& a) {
    fe r = a;
    uint32_t c;
    c = r.v[0] >> 26; r.v[0] &= M26; r.v[1] += c;
    c = r.v[4] >> 26; r.v[4] &= M26; r.v[5] += c;
    c = r.v[1] >> 25; r.v[1] &= M25; r.v[2] += c;
    c = r.v[5] >> 25; r.v[5] &= M25; r.v[6] += c;
    c = r.v[2] >> 26; r.v[2] &= M26; r.v[3] += c;
    c = r.v[6] >> 26; r.v[6] &= M26; r.v[7] += c;
    c = r.v[3] >> 25; r.v[3] &= M25; r.v[4] += c;
    c = r.v[7] >> 25; r.v[7] &= M25; r.v[8] += c;
    c = r.v[4] >> 26; r.v[4] &= M26; r.v[5] += c;
    c = r.v[8] >> 26; r.v[8] &= M26; r.v[9] += c;
    c = r.v[9] >> 25; r.v[9] &= M25; r.v[0] += 19 * c;
    c = r.v[0] >> 26; r.v[0] &= M26; r.v[1] += c;
    return r;
}

// carry of ten 64-bit column sums (each < 2^63) into a carried element
NWV_HD fe fe_carry64(uint64_t h[10]) {
    uint64_t c;
    c = h[0] >> 26; h[1] += c; h[0] &= M26;
    c = h[4] >> 26; h[5] += c; h[4] &= M26;
    c = h[1] >> 25; h[2] += c; h[1] &= M25;
    c = h[5] >> 25; h[6] += c; h[5] &= M25;
    c = h[2] >> 26; h[3] += c; h[2] &= M26;
    c = h[6] >> 26; h[7] += c; h[6] &= M26;
    c = h[3] >> 25; h[4] += c; h[3] &= M25;
    c = h[7] >> 25; h[8] += c; h[7] &= M25;
    c = h[4] >> 26; h[5] += c; h[4] &= M26;
    c = h[8] >> 26; h[9] += c; h[8] &= M26;
    c = h[9] >> 25; h[0] += c * 19; h[9] &= M25;
    fe r;
#pragma unroll
    for (int i = 2; i < 10; i++) r.v[i] = (uint32_t)h[i];
    // last carry in 32 bits: limbs 0 and 1 leave as plain 32-bit values (keeps the compiler
    // from carrying them as 64-bit quantities into the next multiply)
    r.v[0] = (uint32_t)h[0] & M26;
    r.v[1] = (uint32_t)h[1] + (uint32_t)(h[0] >> 26);
    return r;
}

NWV_HD uint64_t mad(uint32_t a, uint32_t b, uint64_t c) { return (uint64_t)a * b + c; }

// a * b + c as one v_mad_u64_u32 the optimiser cannot take apart: a column sum that starts from
// the carry of the column below keeps that carry as the 64-bit addend of its first multiply-add
// (LLVM otherwise reassociates the sum and adds the carry with a v_lshl_add_u64 of its own).
// The host path is the same arithmetic in plain C++.
// The compiler pads an asm statement that names a register a recent asm statement wrote with
// s_nop, so the interleaved chains of a product write their (unused) carry-outs to different
// registers: chain 0 to vcc, the others each to an SGPR pair of its own (`sink`, kept live
// through the chain so that no two chains are given the same pair).
template <int CHAIN>
NWV_HD uint64_t mad_pin(uint32_t a, uint32_t b, uint64_t c, uint64_t& sink) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint64_t d;
    if constexpr (CHAIN == 0)
        asm("v_mad_u64_u32 %0, vcc, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c) : "vcc");
    else
        asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(d), "+s"(sink) : "v"(a), "v"(b), "v"(c));
    return d;
#else
    (void)sink;
    return (uint64_t)a * b + c;
#endif
}

// acc + a[0] b[0] + ... + a[n-1] b[n-1] as n dependent v_mad_u64_u32 in ONE asm statement (a
// whole column sum): the compiler pads between asm statements, never inside one, and the
// hardware interlocks a multiply-add on the one before it.
#if defined(__HIP_DEVICE_COMPILE__)
#define NWV_MAD1(A, B) "v_mad_u64_u32 %0, vcc, %" #A ", %" #B ", %0\n\t"
#define NWV_AB(t) "v"(a[t]), "v"(b[t])
#endif
NWV_HD uint64_t mad_col(int n, const uint32_t* a, const uint32_t* b, uint64_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    switch (n) {  // n is a constant after unrolling
        case 4:
            asm(NWV_MAD1(1, 2) NWV_MAD1(3, 4) NWV_MAD1(5, 6) NWV_MAD1(7, 8)
                : "+v"(acc) : NWV_AB(0), NWV_AB(1), NWV_AB(2), NWV_AB(3) : "vcc");
            break;
        case 5:
            asm(NWV_MAD1(1, 2) NWV_MAD1(3, 4) NWV_MAD1(5, 6) NWV_MAD1(7, 8) NWV_MAD1(9, 10)
                : "+v"(acc) : NWV_AB(0), NWV_AB(1), NWV_AB(2), NWV_AB(3), NWV_AB(4) : "vcc");
            break;
        case 6:
            asm(NWV_MAD1(1, 2) NWV_MAD1(3, 4) NWV_MAD1(5, 6) NWV_MAD1(7, 8) NWV_MAD1(9, 10) NWV_MAD1(11, 12)
                : "+v"(acc) : NWV_AB(0), NWV_AB(1), NWV_AB(2), NWV_AB(3), NWV_AB(4), NWV_AB(5) : "vcc");
            break;
        case 9:
            asm(NWV_MAD1(1, 2) NWV_MAD1(3, 4) NWV_MAD1(5, 6) NWV_MAD1(7, 8) NWV_MAD1(9, 10) NWV_MAD1(11, 12)
                NWV_MAD1(13, 14) NWV_MAD1(15, 16) NWV_MAD1(17, 18)
                : "+v"(acc)
                : NWV_AB(0), NWV_AB(1), NWV_AB(2), NWV_AB(3), NWV_AB(4), NWV_AB(5), NWV_AB(6), NWV_AB(7), NWV_AB(8)
                : "vcc");
            break;
        case 10:
            asm(NWV_MAD1(1, 2) NWV_MAD1(3, 4) NWV_MAD1(5, 6) NWV_MAD1(7, 8) NWV_MAD1(9, 10) NWV_MAD1(11, 12)
                NWV_MAD1(13, 14) NWV_MAD1(15, 16) NWV_MAD1(17, 18) NWV_MAD1(19, 20)
                : "+v"(acc)
                : NWV_AB(0), NWV_AB(1), NWV_AB(2), NWV_AB(3), NWV_AB(4), NWV_AB(5), NWV_AB(6), NWV_AB(7), NWV_AB(8),
                  NWV_AB(9)
                : "vcc");
            break;
        default:
            __builtin_trap();  // no column of a product has another length
    }
    return acc;
#else
    for (int t = 0; t < n; t++) acc += (uint64_t)a[t] * b[t];
    return acc;
#endif
}

// How the ten column sums of a product are accumulated and carried (measured by
// tools/ubench_field):
//   FE_COLS_PLAIN   ten independent sums, then fe_carry64 adds each carry into the next sum
//   FE_COLS_SERIAL  one chain 0 -> 1 -> ... -> 9: every sum but the first starts from the carry
//                   of the column below (no carry adds, every multiply-add depends on the last)
//   FE_COLS_TWO     two chains, 0 -> 1 -> 2 -> 3 and 4 -> 5 -> ... -> 9, their multiply-adds
//                   interleaved; the carry 3 -> 4 -> 5 is added after the chains as fe_carry64
//                   does.  Limb for limb the result fe_carry64 gives.
//   FE_COLS_HALVES  two chains of five columns, 0 -> ... -> 4 and 5 -> ... -> 9, then 4 -> 5 -> 6
//   FE_COLS_THREE   three chains, 0 -> 1 -> 2, 3 -> 4 -> 5 and 6 -> ... -> 9, then 2 -> 3 -> 4
//                   and 5 -> 6 -> 7
// Every form ends with the wrap 9 -> 0 -> 1 (times 19) in the carried limbs, and every form's
// result is carried ("L", m <= 1.01); the one-chain form leaves limbs 0 and 2..9 below their
// width and only limb 1 above it (by the wrap's last carry, < 2^17).
// | FE_COLS_BYCOL: each column sum is one asm statement (mad_col) and the chains alternate column
// by column; without it every multiply-add is a statement of its own and the chains alternate
// term by term.
enum { FE_COLS_PLAIN = 0, FE_COLS_SERIAL = 1, FE_COLS_TWO = 2, FE_COLS_HALVES = 3, FE_COLS_THREE = 4,
       FE_COLS_BYCOL = 8 };
// The kernels' form: one chain, a statement per column.  It has the fewest instructions (no carry
// add is left) and was the fastest form of squaring and of multiply at every occupancy measured
// (profiles/seeded_ubench_field_seeded.jsonl), one wave per SIMD included.
#ifndef NWV_FE_FORM
#define NWV_FE_FORM (FE_COLS_SERIAL | FE_COLS_BYCOL)
#endif

// term i of column k: the product a * b (false: the column has no such term).
// Multiply: f_i g_j with i + j = k (mod 10), doubled when i and j are both odd (radix 2^25.5)
// and multiplied by 19 when i + j >= 10 (2^255 = 19); f2 = odd limbs doubled, g19 = 19 g.
// Squaring (55 products): pair (i < j) is doubled on f_i, the odd/odd doubling and the 19 of the
// wrap go on f_j; diagonal terms carry the odd doubling and the wrap on one side.  A wrapping
// pair of an even i with j = 7 or 9 is f_i (38 f_j) instead of (2 f_i)(19 f_j): 38 f_7 and 38 f_9
// exist for the odd/odd pairs and the diagonal, so 19 f_7, 19 f_9 and 2 f_8 are never formed
// (13 scaled operands instead of 16); every product keeps its value.
template <bool SQ>
NWV_HD bool fe_term(const uint32_t* f, const uint32_t* f2, const uint32_t* g, const uint32_t* g19, int k, int i,
                    uint32_t& a, uint32_t& b) {
    const int j = (k - i + 10) % 10;
    const bool wrap = (i + j) >= 10;
    const bool dbl = (i & 1) && (j & 1);
    if (SQ) {
        if (j < i) return false;
        if (wrap && !(i & 1) && (j == 7 || j == 9)) {
            a = f[i];
            b = f[j] * 38u;
            return true;
        }
        a = (i == j) ? f[i] : (f[i] << 1);
        b = f[j] * ((dbl ? 2u : 1u) * (wrap ? 19u : 1u));
    } else {
        a = dbl ? f2[i] : f[i];
        b = wrap ? g19[j] : g[j];
    }
    return true;
}

// Column sums in one, two or three chains (chain c > 0 starts at column H2, H3; 0 = no such
// chain), their multiply-adds interleaved term by term; each column after a chain's first is
// seeded with the carry of the column below.  Then the carry of each chain's last column goes
// into the next chain's (already carried) head and on into the column after it, and the wrap.
// Every pre-carry sum, carry-in included, stays below 2^63 for inputs of magnitude <= 3.36.
template <int H2, int H3, bool BYCOL, bool SQ>
NWV_HD fe fe_cols_seeded(const uint32_t* f, const uint32_t* f2, const uint32_t* g, const uint32_t* g19) {
    static_assert(H3 == 0 || (H2 > 0 && H3 >= H2 + 3 && H3 <= 8), "chain 1 carries its head's successor itself");
    static_assert(H2 == 0 || H3 != 0 || H2 <= 8, "the last chain has two columns or more");
    constexpr int NCH = H3 ? 3 : H2 ? 2 : 1;
    constexpr int head[3] = {0, H2, H3};
    constexpr int ncol[3] = {H2 ? H2 : 10, H2 ? (H3 ? H3 : 10) - H2 : 0, H3 ? 10 - H3 : 0};
    constexpr int maxcol = ncol[0] > ncol[1] ? (ncol[0] > ncol[2] ? ncol[0] : ncol[2])
                                             : (ncol[1] > ncol[2] ? ncol[1] : ncol[2]);
    uint64_t acc[3] = {0, 0, 0}, sink[3] = {0, 0, 0};
    uint32_t h[10];
#pragma unroll
    for (int cs = 0; cs < maxcol; cs++) {
        if constexpr (BYCOL) {
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const int nc = c == 0 ? ncol[0] : c == 1 ? ncol[1] : ncol[2];
                if (cs >= nc) continue;
                const int k = (c == 0 ? head[0] : c == 1 ? head[1] : head[2]) + cs;
                uint32_t ta[10], tb[10];
                int n = 0;
#pragma unroll
                for (int i = 0; i < 10; i++)
                    if (fe_term<SQ>(f, f2, g, g19, k, i, ta[n], tb[n])) n++;
                if (cs == 0) {
                    acc[c] = mad_col(n - 1, ta + 1, tb + 1, (uint64_t)ta[0] * tb[0]);
                } else {
                    NWV_ASSERT(acc[c] < (1ull << 63));
                    h[k - 1] = (uint32_t)acc[c] & ((k - 1) & 1 ? M25 : M26);
                    acc[c] = mad_col(n, ta, tb, acc[c] >> limb_bits(k - 1));
                }
            }
            continue;
        }
        bool started[3] = {false, false, false};
#pragma unroll
        for (int i = 0; i < 10; i++) {
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const int nc = c == 0 ? ncol[0] : c == 1 ? ncol[1] : ncol[2];
                if (cs >= nc) continue;
                const int k = (c == 0 ? head[0] : c == 1 ? head[1] : head[2]) + cs;
                uint32_t a, b;
                if (!fe_term<SQ>(f, f2, g, g19, k, i, a, b)) continue;
                if (!started[c]) {
                    started[c] = true;
                    if (cs == 0) {
                        acc[c] = (uint64_t)a * b;
                        continue;
                    }
                    NWV_ASSERT(acc[c] < (1ull << 63));
                    h[k - 1] = (uint32_t)acc[c] & ((k - 1) & 1 ? M25 : M26);
                    acc[c] >>= limb_bits(k - 1);
                }
                acc[c] = c == 0   ? mad_pin<0>(a, b, acc[c], sink[0])
                         : c == 1 ? mad_pin<1>(a, b, acc[c], sink[1])
                                  : mad_pin<2>(a, b, acc[c], sink[2]);
            }
        }
    }
#pragma unroll
    for (int c = 1; c < NCH; c++) {
        const int hd = c == 1 ? head[1] : head[2];
        NWV_ASSERT(acc[c - 1] < (1ull << 63));
        h[hd - 1] = (uint32_t)acc[c - 1] & ((hd - 1) & 1 ? M25 : M26);
        const uint64_t t = h[hd] + (acc[c - 1] >> limb_bits(hd - 1));
        h[hd] = (uint32_t)t & (hd & 1 ? M25 : M26);
        h[hd + 1] += (uint32_t)(t >> limb_bits(hd));
    }
    NWV_ASSERT(acc[NCH - 1] < (1ull << 63));
    h[9] = (uint32_t)acc[NCH - 1] & M25;
    const uint64_t t0 = h[0] + (acc[NCH - 1] >> 25) * 19;
    fe r;
#pragma unroll
    for (int i = 2; i < 10; i++) r.v[i] = h[i];
    // last carry in 32 bits, as fe_carry64
    r.v[0] = (uint32_t)t0 & M26;
    r.v[1] = h[1] + (uint32_t)(t0 >> 26);
    return r;
}

// the chains of a column-sum form: second and third head
NWV_HD constexpr int fe_form_h2(int form) {
    return (form & 7) == FE_COLS_TWO ? 4 : (form & 7) == FE_COLS_HALVES ? 5 : (form & 7) == FE_COLS_THREE ? 3 : 0;
}
NWV_HD constexpr int fe_form_h3(int form) { return (form & 7) == FE_COLS_THREE ? 6 : 0; }

template <int FORM>
NWV_HD fe fe_mul_form(const fe& f, const fe& g) {
    NWV_SEQ();
    NWV_COUNT(nwv_count_mul);
    fe_check(f, 3.36);
    fe_check(g, 3.36);
    uint32_t g19[10], f2[10];
#pragma unroll
    for (int i = 0; i < 10; i++) {
        g19[i] = g.v[i] * 19u;
        f2[i] = (i & 1) ? (f.v[i] << 1) : f.v[i];
    }
    fe r;
    if constexpr (FORM == FE_COLS_PLAIN) {
        uint64_t h[10];
#pragma unroll
        for (int k = 0; k < 10; k++) {
            uint64_t acc = 0;
#pragma unroll
            for (int i = 0; i < 10; i++) {
                uint32_t a, b;
                fe_term<false>(f.v, f2, g.v, g19, k, i, a, b);
                acc = mad(a, b, acc);
            }
            NWV_ASSERT(acc < (1ull << 63));
            h[k] = acc;
        }
        r = fe_carry64(h);
    } else {
        constexpr bool bycol = (FORM & FE_COLS_BYCOL) != 0;
        r = fe_cols_seeded<fe_form_h2(FORM), fe_form_h3(FORM), bycol, false>(f.v, f2, g.v, g19);
    }
    NWV_SEQ();
    return r;
}

template <int FORM>
NWV_HD fe fe_sq_form(const fe& f) {
    NWV_SEQ();
    NWV_COUNT(nwv_count_sq);
    fe_check(f, 3.36);
    fe r;
    if constexpr (FORM == FE_COLS_PLAIN) {
        uint64_t h[10];
#pragma unroll
        for (int k = 0; k < 10; k++) h[k] = 0;
#pragma unroll
        for (int i = 0; i < 10; i++) {
#pragma unroll
            for (int j = i; j < 10; j++) {
                uint32_t a, b;
                fe_term<true>(f.v, nullptr, nullptr, nullptr, (i + j) % 10, i, a, b);
                h[(i + j) % 10] = mad(a, b, h[(i + j) % 10]);
            }
        }
#pragma unroll
        for (int k = 0; k < 10; k++) NWV_ASSERT(h[k] < (1ull << 63));
        r = fe_carry64(h);
    } else {
        constexpr bool bycol = (FORM & FE_COLS_BYCOL) != 0;
        r = fe_cols_seeded<fe_form_h2(FORM), fe_form_h3(FORM), bycol, true>(f.v, nullptr, nullptr, nullptr);
    }
    NWV_SEQ();
    return r;
}

NWV_HD fe fe_mul(const fe& f, const fe& g) { return fe_mul_form<NWV_FE_FORM>(f, g); }
NWV_HD fe fe_sq(const fe& f) { return fe_sq_form<NWV_FE_FORM>(f); }
// f times a compile-time constant (fe_d, fe_d2, fe_sqrtm1): the plain form, in which the
// constant's words and their multiples of 19 stay scalar operands; an asm statement's operands
// are all VGPRs, twenty more live registers around such a product.
NWV_HD fe fe_mul_const(const fe& f, const fe& c) { return fe_mul_form<FE_COLS_PLAIN>(f, c); }

NWV_HD void fe_pin(fe& a);
NWV_HD fe fe_sqn(fe f, int n) {
#pragma unroll 1
    for (int i = 0; i < n; i++) {
        fe_pin(f);  // loop-carried limbs stay plain 32-bit values
        f = fe_sq(f);
    }
    return f;
}

// canonical little-endian 8x32-bit words of a (value reduced into [0, p))
NWV_HD void fe_freeze(const fe& a, uint32_t w[8]) {
    NWV_SEQ();
    fe h = fe_carry(fe_carry(a));
    uint32_t q = (h.v[0] + 19) >> 26;
#pragma unroll
    for (int i = 1; i < 10; i++) q = (h.v[i] + q) >> limb_bits(i);
    h.v[0] += 19 * q;
    uint32_t c;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        c = h.v[i] >> limb_bits(i);
        h.v[i] &= (i & 1) ? M25 : M26;
        h.v[i + 1] += c;
    }
    h.v[9] &= M25;
    // pack limbs at bit positions 0,26,51,77,102,128,153,179,204,230
    w[0] = h.v[0] | (h.v[1] << 26);
    w[1] = (h.v[1] >> 6) | (h.v[2] << 19);
    w[2] = (h.v[2] >> 13) | (h.v[3] << 13);
    w[3] = (h.v[3] >> 19) | (h.v[4] << 6);
    w[4] = h.v[5] | (h.v[6] << 25);
    w[5] = (h.v[6] >> 7) | (h.v[7] << 19);
    w[6] = (h.v[7] >> 13) | (h.v[8] << 12);
    w[7] = (h.v[8] >> 20) | (h.v[9] << 6);
    NWV_SEQ();
}

// FieldElement::from_bytes semantics: bit 255 ignored, values >= p kept (they reduce lazily)
NWV_HD fe fe_from_words(const uint32_t w[8]) {
    fe r;
    r.v[0] = w[0] & M26;
    r.v[1] = ((w[0] >> 26) | (w[1] << 6)) & M25;
    r.v[2] = ((w[1] >> 19) | (w[2] << 13)) & M26;
    r.v[3] = ((w[2] >> 13) | (w[3] << 19)) & M25;
    r.v[4] = (w[3] >> 6) & M26;
    r.v[5] = w[4] & M25;
    r.v[6] = ((w[4] >> 25) | (w[5] << 7)) & M26;
    r.v[7] = ((w[5] >> 19) | (w[6] << 13)) & M25;
    r.v[8] = ((w[6] >> 12) | (w[7] << 20)) & M26;
    r.v[9] = (w[7] >> 6) & M25;
    return r;
}

NWV_HD bool fe_is_zero(const fe& a) {
    uint32_t w[8];
    fe_freeze(a, w);
    uint32_t acc = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) acc |= w[i];
    return acc == 0;
}
NWV_HD bool fe_eq(const fe& a, const fe& b) { return fe_is_zero(fe_sub(fe_carry(a), fe_carry(b))); }
NWV_HD uint32_t fe_is_negative(const fe& a) {
    uint32_t w[8];
    fe_freeze(a, w);
    return w[0] & 1;
}
NWV_HD fe fe_select(const fe& a, const fe& b, bool pick_b) {
    fe r;
#pragma unroll
    for (int i = 0; i < 10; i++) r.v[i] = pick_b ? b.v[i] : a.v[i];
    return r;
}

// x^(2^250 - 1) and x^11 (the shared head of inversion and the (p-5)/8 power)
NWV_HD void fe_pow22501(const fe& x, fe& t19, fe& t3) {
    fe t0 = fe_sq(x);
    fe t1 = fe_sqn(t0, 2);
    fe t2 = fe_mul(x, t1);
    t3 = fe_mul(t0, t2);
    fe t4 = fe_sq(t3);
    fe t5 = fe_mul(t2, t4);
    fe t6 = fe_sqn(t5, 5);
    fe t7 = fe_mul(t6, t5);
    fe t8 = fe_sqn(t7, 10);
    fe t9 = fe_mul(t8, t7);
    fe t10 = fe_sqn(t9, 20);
    fe t11 = fe_mul(t10, t9);
    fe t12 = fe_sqn(t11, 10);
    fe t13 = fe_mul(t12, t7);
    fe t14 = fe_sqn(t13, 50);
    fe t15 = fe_mul(t14, t13);
    fe t16 = fe_sqn(t15, 100);
    fe t17 = fe_mul(t16, t15);
    fe t18 = fe_sqn(t17, 50);
    t19 = fe_mul(t18, t13);
}
NWV_HD fe fe_invert(const fe& x) {
    fe t19, t3;
    fe_pow22501(x, t19, t3);
    return fe_mul(fe_sqn(t19, 5), t3);
}
NWV_HD fe fe_pow_p58(const fe& x) {
    fe t19, t3;
    fe_pow22501(x, t19, t3);
    return fe_mul(fe_sqn(t19, 2), x);
}

// curve constants (radix 2^25.5 limbs)
NWV_HD fe fe_d() {
    const uint32_t c[10] = {56195235, 13857412, 51736253, 6949390, 114729,
                            24766616, 60832955, 30306712, 48412415, 21499315};
    fe r; for (int i = 0; i < 10; i++) r.v[i] = c[i]; return r;
}
// 1 / d: 2dxy of an affine Niels record times it is 2xy (msm_point_seed)
NWV_HD fe fe_dinv() {
    const uint32_t c[10] = {30013507, 3972531, 42321084, 12719050, 2979674,
                            28954470, 51415654, 29910370, 18959708, 16925179};
    fe r; for (int i = 0; i < 10; i++) r.v[i] = c[i]; return r;
}
NWV_HD fe fe_d2() {
    const uint32_t c[10] = {45281625, 27714825, 36363642, 13898781, 229458,
                            15978800, 54557047, 27058993, 29715967, 9444199};
    fe r; for (int i = 0; i < 10; i++) r.v[i] = c[i]; return r;
}
NWV_HD fe fe_sqrtm1() {
    const uint32_t c[10] = {34513072, 25610706, 9377949, 3500415, 12389472,
                            33281959, 41962654, 31548777, 326685, 11406482};
    fe r; for (int i = 0; i < 10; i++) r.v[i] = c[i]; return r;
}

// Optimisation fence for a field element: the value is "redefined" here, so nothing computed
// from it can be hoisted above this point (keeps IR-level code motion from stretching live
// ranges across the long exponentiation chains).
NWV_HD void fe_pin(fe& a) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int i = 0; i < 10; i++) asm volatile("" : "+v"(a.v[i]));
#else
    (void)a;
#endif
}

// FieldElement::sqrt_ratio_i (dalek): returns was_nonzero_square; r = nonnegative sqrt(u/v)
//   r = (u v^3) (u v^7)^((p-5)/8); check = v r^2;
//   correct = check == u, flipped = check == -u, flipped_i = check == -u sqrt(-1)
NWV_HD bool fe_sqrt_ratio_i(const fe& u_in, const fe& v_in, fe& r) {
    fe u = u_in, v = v_in;
    fe v3 = fe_mul(fe_sq(v), v);
    fe uv7 = fe_mul(u, fe_mul(fe_sq(v3), v));
    fe uv3 = fe_mul(u, v3);
    fe pw = fe_pow_p58(uv7);
    fe_pin(pw);
    r = fe_mul(uv3, pw);
    fe_pin(v);
    fe check = fe_carry(fe_mul(v, fe_sq(r)));
    fe_pin(u);
    const bool correct = fe_is_zero(fe_sub(check, u));
    const bool flipped = fe_is_zero(fe_add(check, u));
    fe_pin(u);
    const bool flipped_i = fe_is_zero(fe_add(check, fe_mul_const(u, fe_sqrtm1())));
    fe_pin(r);
    fe r_prime = fe_mul_const(r, fe_sqrtm1());
    r = fe_select(r, r_prime, flipped || flipped_i);
    r = fe_select(r, fe_carry(fe_neg(r)), fe_is_negative(r) != 0);
    return correct || flipped;
}

}  // namespace nwv
