// trim_hostemu.cpp -- TEST-ONLY host build (NWV_BOUNDS_CHECK: limb bounds and column sums below
// 2^63 asserted) of the pieces the bucket, squaring and hash trimming touched: the seeded bucket
// accumulator (msm.h msm_point_seed), fe_sq's operand split, the operand roles of ge_p1p1_to_p3 and
// SHA-512 of a prefixed message.  Never part of the product.
#define NWV_HD __host__ __device__ inline
#include <cstring>
#include <vector>

#include "../../narwhal_amd/csrc/msm.h"

using namespace nwv;

namespace {

bool frozen_eq(const fe& a, const fe& b) {
    uint32_t x[8], y[8];
    fe_freeze(a, x);
    fe_freeze(b, y);
    return std::memcmp(x, y, sizeof x) == 0;
}
// the same point: X1 Z2 = X2 Z1 and Y1 Z2 = Y2 Z1, and each T consistent (T Z = X Y)
bool same_point(const ge_p3& a, const ge_p3& b) {
    return frozen_eq(fe_mul(a.X, b.Z), fe_mul(b.X, a.Z)) && frozen_eq(fe_mul(a.Y, b.Z), fe_mul(b.Y, a.Z)) &&
           frozen_eq(fe_mul(a.T, a.Z), fe_mul(a.X, a.Y)) && frozen_eq(fe_mul(b.T, b.Z), fe_mul(b.X, b.Y));
}
fe limbs(const uint32_t* p) { return load_fe(p); }

}  // namespace

extern "C" {

// 1 / d: times d it freezes to 1, and it is fe_invert(d)
int he_trim_dinv_ok() {
    return frozen_eq(fe_mul(fe_dinv(), fe_d()), fe_one()) && frozen_eq(fe_dinv(), fe_invert(fe_d())) ? 1 : 0;
}

// n compressed points.  status[i]: 1 = does not decode (nothing checked), 0 = for both signs the
// seeded accumulator of point i's record is identity + P by ge_madd, and stays equal to it after
// 1, 2 and 15 further records (points i + 1, ... cyclically over the decodable ones, signs
// alternating) are added to both; else 2 + the number of further records at which they differ
// (or 100 when Z is not the constant 2).  seed0: X | Y | Z | T words of point 0's seed (sign +).
void he_trim_seed(uint32_t n, const uint8_t* enc, uint8_t* status, uint32_t* seed0) {
    std::vector<uint32_t> rec((size_t)MSM_PT_WORDS * n);
    std::vector<uint32_t> good;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t w[8];
        std::memcpy(w, enc + 32 * (size_t)i, 32);
        ge_p3 P;
        status[i] = ge_decompress(w, P) ? 0 : 1;
        if (status[i]) continue;
        msm_store_point(rec.data() + (size_t)MSM_PT_WORDS * i, P);
        good.push_back(i);
    }
    const int more[3] = {1, 2, 15};
    for (size_t gi = 0; gi < good.size(); gi++) {
        const uint32_t i = good[gi];
        for (int neg = 0; neg < 2 && status[i] == 0; neg++) {
            const ge_precomp q = msm_load_point(rec.data() + (size_t)MSM_PT_WORDS * i, neg != 0);
            const ge_p3 seed = msm_point_seed(q);
            if (i == 0 && neg == 0) store_p3(seed0, seed);
            const ge_p3 ref = ge_p1p1_to_p3(ge_madd(ge_p3_identity(), q));
            if (!frozen_eq(seed.Z, fe_small(2))) status[i] = 100;
            else if (!same_point(seed, ref)) status[i] = 2;
            for (int m = 0; m < 3 && status[i] == 0; m++) {
                ge_p3 a = seed, b = ref;
                for (int t = 1; t <= more[m]; t++) {
                    const uint32_t j = good[(gi + t) % good.size()];
                    const ge_precomp r = msm_load_point(rec.data() + (size_t)MSM_PT_WORDS * j, ((t + neg) & 1) != 0);
                    a = ge_p1p1_to_p3(ge_madd(a, r));
                    b = ge_p1p1_to_p3(ge_madd(b, r));
                }
                if (!same_point(a, b)) status[i] = (uint8_t)(2 + more[m]);
            }
        }
    }
}

// n elements (ten limbs each): sq = fe_sq(f), mul = fe_mul(f, f), sqn = fe_sqn(f, nsq)
void he_trim_sq(uint32_t n, const uint32_t* a, uint32_t* sq, uint32_t* mul, uint32_t* sqn, int nsq) {
    for (uint32_t t = 0; t < n; t++) {
        const fe f = limbs(a + 10 * (size_t)t);
        store_fe(sq + 10 * (size_t)t, fe_sq(f));
        store_fe(mul + 10 * (size_t)t, fe_mul(f, f));
        store_fe(sqn + 10 * (size_t)t, fe_sqn(f, nsq));
    }
}

// n completed points (X | Y | Z | T, ten limbs each): got = ge_p1p1_to_p3, want = the four products
// X T, Y Z, Z T, X Y in that operand order; got2 / want2 the same for ge_p1p1_to_p2 (30 words)
void he_trim_p1p1(uint32_t n, const uint32_t* in, uint32_t* got, uint32_t* want, uint32_t* got2, uint32_t* want2) {
    for (uint32_t t = 0; t < n; t++) {
        const uint32_t* s = in + 40 * (size_t)t;
        const ge_p1p1 c{limbs(s), limbs(s + 10), limbs(s + 20), limbs(s + 30)};
        store_p3(got + 40 * (size_t)t, ge_p1p1_to_p3(c));
        store_p3(want + 40 * (size_t)t, ge_p3{fe_mul(c.X, c.T), fe_mul(c.Y, c.Z), fe_mul(c.Z, c.T), fe_mul(c.X, c.Y)});
        const ge_p2 p = ge_p1p1_to_p2(c);
        const fe w2[3] = {fe_mul(c.X, c.T), fe_mul(c.Y, c.Z), fe_mul(c.Z, c.T)};
        store_fe(got2 + 30 * (size_t)t, p.X);
        store_fe(got2 + 30 * (size_t)t + 10, p.Y);
        store_fe(got2 + 30 * (size_t)t + 20, p.Z);
        for (int k = 0; k < 3; k++) store_fe(want2 + 30 * (size_t)t + 10 * k, w2[k]);
    }
}

// SHA-512(prefix || msg): 64 prefix bytes, as the challenge hash of a signature has (R || A)
void he_trim_sha512(const uint8_t* prefix, const uint8_t* msg, uint32_t mlen, uint8_t* out) {
    uint32_t pw[16];
    std::memcpy(pw, prefix, 64);
    std::vector<uint8_t> m((size_t)mlen + 160, 0);  // (the block loads read past the message, masked)
    if (mlen) std::memcpy(m.data() + 16, msg, mlen);
    sha512_state s;
    sha512_prefixed_msg<16>(s, pw, m.data() + 16, mlen);
    uint32_t o[16];
    sha512_digest_words(s, o);
    std::memcpy(out, o, 64);
}

}  // extern "C"
