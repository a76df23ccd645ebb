// bls_wave_vectors_hostemu.cpp -- the wave interpreter's lane arithmetic (bls_wave.h: comb_sums,
// carry_par / carry_seq, fp_mul, quick_reduce) on the host with its limb bounds evaluated
// (-DBLS_BOUNDS_CHECK), one program at a time on a given slot image
// (tests/test_bls_wave_vectors_hostemu.py; the device runs the same images through
// tools/bls_wave_vectors).
#include <cstring>
#include <vector>

#define BLS_GROUP_HOST_EMU 1  // the host form of bls_wave.h
#ifndef BLS_BOUNDS_CHECK
#error "build with -DBLS_BOUNDS_CHECK"
#endif
#include "../../narwhal_amd/csrc/bls_wave.h"

using namespace bls;
using namespace bls::wave;

namespace {
constexpr uint32_t CANARY = 0xc0ffee11u;
constexpr int GUARD = 4 * SW;  // words on either side of a bank

// the records of program (off, n, nl0) lie inside T_DATA and address slots below `nslots` only
bool prog_ok(uint32_t off, int n, int nl0, int nslots) {
    const size_t len = sizeof(T_DATA) / sizeof(T_DATA[0]);
    if (n < 1 || n > 64 || off % 8) return false;
    size_t at = off;
    int nl = nl0;
    for (int s = 0; s < n; s++) {
        if (nl < 1 || nl > 64 || at + (size_t)nl * REC > len) return false;
        int nl_next = 0;
        for (int l = 0; l < nl; l++) {
            const uint16_t* r = T_DATA + at + (size_t)l * REC;
            if (r[REC - 4] != nl || r[0] >= nslots || r[2] > 16 || r[3] > 16) return false;
            for (int t = 4; t < 4 + 4 * TMAX; t++)
                if ((r[t] & 0xfff) >= nslots) return false;
            if (l && r[REC - 1] != nl_next) return false;
            nl_next = r[REC - 1];
        }
        at += (size_t)nl * REC;
        nl = nl_next;
    }
    return true;
}
}  // namespace

extern "C" {

int bwv_nslots() { return NSLOTS; }
int bwv_nslots_pc() { return NSLOTS_PC; }
int bwv_reg_f() { return REG_F; }

// the program `reps` times over on image (NSLOTS x 14 words, in place) by the host's Wave::run,
// lane_value<8> with the P << k table below slot 0: 0, or -1 for a program outside the tables
int bwv_run8(uint32_t off, int n, int nl0, int reps, uint32_t* image) {
    if (!prog_ok(off, n, nl0, NSLOTS) || reps < 1 || reps > 8) return -1;
    std::vector<uint32_t> buf(WM_WORDS);
    memcpy(buf.data(), &T_KP[0][0], 4 * KP_WORDS);
    memcpy(buf.data() + KP_WORDS, image, 4 * SW * NSLOTS);
    const Wave w{buf.data() + KP_WORDS};
    w.run(Prog{off, (uint16_t)n, (uint16_t)nl0}, reps);
    memcpy(image, buf.data() + KP_WORDS, 4 * SW * NSLOTS);
    return 0;
}

// the same with lane_value<4> (the packed pairing kernel's form: at most four term reads at once,
// then the rest) on a bank of NSLOTS_PC slots (image: NSLOTS_PC x 14 words) with the P << k table
// in an allocation of its own; the words around the bank must come back untouched (-2 if not)
int bwv_run4(uint32_t off, int n, int nl0, int reps, uint32_t* image) {
    if (!prog_ok(off, n, nl0, NSLOTS_PC) || reps < 1 || reps > 8) return -1;
    constexpr int BANK = SW * NSLOTS_PC;
    std::vector<uint32_t> kpt(&T_KP[0][0], &T_KP[0][0] + KP_WORDS);
    std::vector<uint32_t> buf(BANK + 2 * GUARD, CANARY);
    uint32_t* wm = buf.data() + GUARD;
    memcpy(wm, image, 4 * BANK);
    for (int rep = 0; rep < reps; rep++) {
        const uint16_t* base = T_DATA + off;
        int nl = nl0;
        for (int s = 0; s < n; s++) {
            fp out[64];
            uint32_t dst[64];
            int nl_next = 0;
            for (int l = 0; l < nl; l++) {  // every lane's reads, then the writes
                const Rec r = load_rec(base + (uint32_t)l * REC);
                const Hdr h = rec_hdr(r);
                nl_next = h.nl_next;
                dst[l] = rec_u16(r, 0);
                out[l] = lane_value<4>(wm, kpt.data(), h, r);
            }
            for (int l = 0; l < nl; l++)
                for (int j = 0; j < NL; j++) wm[SW * dst[l] + j] = out[l].l[j];
            base += (uint32_t)nl * REC;
            nl = nl_next;
        }
    }
    memcpy(image, wm, 4 * BANK);
    for (int t = 0; t < GUARD; t++)
        if (buf[t] != CANARY || buf[GUARD + BANK + t] != CANARY) return -2;
    return 0;
}

// out: assertions fired, carry_par fallbacks, negative top limb sums; then the counters restart
void bwv_stats(uint64_t* out) {
    BoundsStats& s = bounds_stats();
    out[0] = s.fired;
    out[1] = s.par_fallback;
    out[2] = s.top_negative;
    s = BoundsStats{0, 0, 0, s.first};
}
// the first assertion that fired since the library was loaded ("" if none)
const char* bwv_first_fired() {
    const char* f = bounds_stats().first;
    return f ? f : "";
}

// Wave::f_is_one on an F of 12 x 14 words
int bwv_f_is_one(const uint32_t* f) {
    std::vector<uint32_t> buf(WM_WORDS, 0u);
    const Wave w{buf.data() + KP_WORDS};
    memcpy(w.wm + SW * REG_F, f, 4 * SW * 12);
    return w.f_is_one() ? 1 : 0;
}

}  // extern "C"
