// Host build of the hash role of a BLS call that uses the message ring
// (narwhal_amd/csrc/bls_verify.h: w_hash_ring_item, the item function of k_blsw_pre_r, with
// w_hash_to_g1 and w_g1_clear_raw under it) -- TEST INFRASTRUCTURE ONLY:
// tests/test_bls_msg_ring_hostemu.py runs its four modes with the same interpreter and stage
// tables the kernel runs, on the CPU.
#include <vector>

#define BLS_GROUP_HOST_EMU 1
#include "../../narwhal_amd/csrc/bls_verify.h"

using namespace bls;

namespace {

// a wave whose slots start out as `fill` in every word: a result may not depend on what an
// earlier program left behind
wave::Wave fresh_wave(std::vector<uint32_t>& wm, uint32_t fill) {
    wm.assign(wave::WM_WORDS, fill);
    wave::Wave w;
    w.wm = wm.data() + wave::KP_WORDS;
    return w;
}

}  // namespace

extern "C" {

int bmh_rec_words() { return G1H_REC_WORDS; }

// w_hash_to_g1: out <- the record (raw when clear = 0); raw_out (optional) <- the raw record
void bmh_hash(const uint8_t* msg, size_t n, const uint8_t* dst, size_t dl, int clear, uint32_t fill, uint32_t* out,
              uint32_t* raw_out) {
    std::vector<uint32_t> wm;
    w_hash_to_g1(fresh_wave(wm, fill), msg, (uint32_t)n, dst, (uint32_t)dl, out, clear != 0, raw_out);
}

// one hash-role item: src = the ring record of a hit or null, pub = the ring record a miss also
// fills or null
void bmh_ring_item(const uint8_t* msg, size_t n, const uint8_t* dst, size_t dl, const uint32_t* src, uint32_t* pub,
                   int key_side, uint32_t fill, uint32_t* out) {
    std::vector<uint32_t> wm;
    w_hash_ring_item(fresh_wave(wm, fill), msg, (uint32_t)n, dst, (uint32_t)dl, src, pub, key_side != 0, out);
}

// a homogeneous record as x || y (96 bytes big-endian), zeros for the identity
void bmh_affine(const uint32_t* rec, uint8_t* out) {
    if (rec[3 * NL]) {
        for (int i = 0; i < 96; i++) out[i] = 0;
        return;
    }
    const fp zi = fp_inv(ld_fp(rec + 2 * NL));
    plain_to_be(out, fp_from_mont(fp_mul(ld_fp(rec), zi)));
    plain_to_be(out + 48, fp_from_mont(fp_mul(ld_fp(rec + NL), zi)));
}

}  // extern "C"
