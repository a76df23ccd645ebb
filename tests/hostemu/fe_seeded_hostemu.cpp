// fe_seeded_hostemu.cpp -- TEST-ONLY host build of fe25519.h's multiply and squaring in every
// column-sum form (FE_COLS_*), with the limb-bound and column-sum assertions enabled
// (NWV_BOUNDS_CHECK: every pre-carry column sum, carry-in included, stays below 2^63).  The host
// path runs the same arithmetic in the same column order as the device's pinned multiply-adds.
// Never part of the product.
#define NWV_HD __host__ __device__ inline
#include "../../narwhal_amd/csrc/fe25519.h"

using namespace nwv;

namespace {

template <int FORM>
void run(uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* mul, uint32_t* sq, uint32_t* sqn, int nsq) {
    for (uint32_t t = 0; t < n; t++) {
        fe f, g;
        for (int i = 0; i < 10; i++) f.v[i] = a[10 * t + i], g.v[i] = b[10 * t + i];
        const fe m = fe_mul_form<FORM>(f, g);
        const fe s = fe_sq_form<FORM>(f);
        fe q = f;
        for (int r = 0; r < nsq; r++) q = fe_sq_form<FORM>(q);
        for (int i = 0; i < 10; i++) mul[10 * t + i] = m.v[i], sq[10 * t + i] = s.v[i], sqn[10 * t + i] = q.v[i];
    }
}

}  // namespace

extern "C" {

int he_fe_default_form() { return NWV_FE_FORM; }

// n elements a, b (ten limbs each): mul = a b, sq = a^2, sqn = a^(2^nsq) in column-sum form
// `form`; form < 0: the library's own fe_mul / fe_sq / fe_sqn.  Returns 0, or -1 for an unknown form.
int he_fe_ops(int form, uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* mul, uint32_t* sq,
              uint32_t* sqn, int nsq) {
#define FORM_CASE(F) \
    case F: run<F>(n, a, b, mul, sq, sqn, nsq); return 0
    switch (form) {
        FORM_CASE(FE_COLS_PLAIN);
        FORM_CASE(FE_COLS_SERIAL);
        FORM_CASE(FE_COLS_TWO);
        FORM_CASE(FE_COLS_HALVES);
        FORM_CASE(FE_COLS_THREE);
        FORM_CASE(FE_COLS_SERIAL | FE_COLS_BYCOL);
        FORM_CASE(FE_COLS_TWO | FE_COLS_BYCOL);
        FORM_CASE(FE_COLS_HALVES | FE_COLS_BYCOL);
        FORM_CASE(FE_COLS_THREE | FE_COLS_BYCOL);
        default: break;
    }
    if (form >= 0) return -1;
    for (uint32_t t = 0; t < n; t++) {
        fe f, g;
        for (int i = 0; i < 10; i++) f.v[i] = a[10 * t + i], g.v[i] = b[10 * t + i];
        const fe m = fe_mul(f, g), s = fe_sq(f), q = fe_sqn(f, nsq);
        for (int i = 0; i < 10; i++) mul[10 * t + i] = m.v[i], sq[10 * t + i] = s.v[i], sqn[10 * t + i] = q.v[i];
    }
    return 0;
}

}  // extern "C"
