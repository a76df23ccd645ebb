// Host build of the dense key-sum stage of large BLS calls (narwhal_amd/csrc/bls_verify.h:
// blsd_total_lane, blsd_lane_ascending, blsd_lane_direct, blsd_lane_absent, blsd_finish,
// jac_add_affine; narwhal_amd/csrc/bls_apk_dense.h: the routing) -- TEST INFRASTRUCTURE ONLY:
// tests/test_bls_apk_dense_hostemu.py runs k_blsd_total's and k_blsd_apk's per-group arithmetic on
// the CPU, lane by lane and level by level as the kernels order it, and compares every item's sum
// (made affine) and status with the per-item kernel's (blsw_apk_item: 64 lanes, jac_add over
// jac_from_affine, a six-level tree) on the same inputs.
#include <vector>

#define BLS_GROUP_HOST_EMU 1
#include "../../narwhal_amd/csrc/bls_verify.h"
#include "../../narwhal_amd/csrc/bls_apk_dense.h"

using namespace bls;

namespace {

// the tree both kernels run over `lanes` partial sums: lane s < h takes lane s + h's
jac<fp2> tree(std::vector<jac<fp2>>& acc) {
    for (size_t h = acc.size() / 2; h >= 1; h /= 2)
        for (size_t s = 0; s < h; s++) acc[s] = jac_add(acc[s], acc[s + h]);
    return acc[0];
}
bool same_point(const jac<fp2>& a, const jac<fp2>& b) {
    if (a.inf || b.inf) return a.inf == b.inf;
    fp2 ax, ay, bx, by;
    g2_to_affine(ax, ay, a);
    g2_to_affine(bx, by, b);
    return f2_eq(ax, bx) && f2_eq(ay, by);
}

}  // namespace

extern "C" {

uint32_t bh_ad_lanes(size_t n_dense, unsigned long forced) { return nwv::apk_dense_lanes(n_dense, forced); }

// the split of a call's items: kind[i] = 1 dense, 0 left to the per-item kernel
void bh_ad_split(size_t n, const uint32_t* kmode, const uint32_t* pk_cnt, int32_t* kind) {
    nwv::ApkDenseSplit s;
    nwv::apk_dense_split(n, kmode, pk_cnt, s);
    for (uint32_t i : s.dense) kind[i] = 1;
    for (uint32_t i : s.rest) kind[i] = 0;
}

// A key table of nk keys (pks, 96 bytes each): key k sits in cache slot nk - 1 - k with status
// kst[k] when cached[k], else it is a key the cache does not hold.  n items, item i = the key
// numbers klist[koff[i] .. + kcnt[i]); every item must be one the dense kernel takes (two keys or
// more, all cached).  lanes = 4, 8 or 16.  Per item: st_dense / st_ref = the dense arithmetic's
// and the per-item kernel's status, same = 1 when the two sums are one point (or both the
// identity), mode = 1 when the sum came from the total.  *flag = k_blsd_total's flag.
// Returns 0, or -1 when a key does not decode or an item is not a dense item.
int bh_ad_items(size_t nk, const uint8_t* pks, const uint8_t* cached, const int32_t* kst, size_t n,
                const uint32_t* koff, const uint32_t* kcnt, const uint32_t* klist, uint32_t lanes, int32_t* st_dense,
                int32_t* st_ref, int32_t* same, int32_t* mode, int32_t* flag) {
    const uint32_t cap = (uint32_t)nk;
    std::vector<uint32_t> hrc(G2_REC_WORDS * nk, 0), ktab(nk);
    std::vector<int32_t> sc(nk, ST_OK);
    for (size_t k = 0; k < nk; k++) {
        uint32_t krec[G2_REC_WORDS];
        if (key_decode(pks + 96 * k, krec) != ST_OK) return -1;
        if (!cached[k]) {
            ktab[k] = cap + (uint32_t)k;
            continue;
        }
        const uint32_t slot = (uint32_t)(nk - 1 - k);
        ktab[k] = slot;
        sc[slot] = kst[k];
        fp2 ax, ay;
        ld_g2(krec, ax, ay);
        g2_to_affine(ax, ay, jac_mul64(jac_from_affine(ax, ay), BLS_H_EFF));
        st_g2(hrc.data() + G2_REC_WORDS * slot, ax, ay, false);
    }
    const DenseKeys t{hrc.data(), sc.data(), ktab.data(), (uint32_t)nk, cap};
    // k_blsd_total: 64 lanes' shares, the six-level tree, the flag
    bool all_ok = true;
    std::vector<jac<fp2>> part(64);
    for (uint32_t l = 0; l < 64; l++) {
        bool ok;
        part[l] = blsd_total_lane(t, l, 64, ok);
        all_ok = all_ok && ok;
    }
    jac<fp2> total = tree(part);
    if (!all_ok) total = blsd_identity();
    *flag = all_ok ? 1 : 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t cnt = kcnt[i];
        const uint32_t* idx = klist + koff[i];
        if (cnt < 2) return -1;
        for (uint32_t j = 0; j < cnt; j++)
            if (idx[j] >= nk || ktab[idx[j]] >= cap) return -1;
        // k_blsd_apk's group
        bool asc = true;
        for (uint32_t s = 0; s < lanes; s++) asc = asc && blsd_lane_ascending(idx, cnt, s, lanes);
        const bool comp = asc && all_ok && cnt > t.n_keys / 2;
        uint32_t first_bad = 0xffffffffu;
        std::vector<jac<fp2>> g(lanes);
        for (uint32_t s = 0; s < lanes; s++) {
            uint32_t fb = 0xffffffffu;
            g[s] = comp ? blsd_lane_absent(t, idx, cnt, s, lanes) : blsd_lane_direct(t, idx, cnt, s, lanes, fb);
            first_bad = fb < first_bad ? fb : first_bad;
        }
        jac<fp2> acc = tree(g);
        st_dense[i] = blsd_finish(t, idx, acc, comp, total, first_bad);
        mode[i] = comp ? 1 : 0;
        // blsw_apk_item on the keys' [h_eff] pk records
        uint32_t rbad = 0xffffffffu;
        std::vector<jac<fp2>> r(64);
        for (uint32_t l = 0; l < 64; l++) {
            r[l] = blsd_identity();
            for (uint32_t j = l; j < cnt; j += 64) {
                const uint32_t slot = ktab[idx[j]];
                if (sc[slot] != ST_OK) {
                    rbad = j < rbad ? j : rbad;
                    break;
                }
                fp2 x, y;
                ld_g2(hrc.data() + G2_REC_WORDS * slot, x, y);
                r[l] = jac_add(r[l], jac_from_affine(x, y));
            }
        }
        jac<fp2> ref = tree(r);
        int32_t rs = ST_OK;
        if (rbad != 0xffffffffu) rs = sc[ktab[idx[rbad]]];
        else if (ref.inf) rs = ST_PK_INFINITY;
        if (rs != ST_OK) ref = blsd_identity();
        st_ref[i] = rs;
        same[i] = same_point(acc, ref) ? 1 : 0;
    }
    return 0;
}

}  // extern "C"
