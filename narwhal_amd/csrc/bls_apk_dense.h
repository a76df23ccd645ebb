// bls_apk_dense.h -- the host side of the dense key-sum stage of large BLS calls
// (nwv_bls_set_apk_dense_min): which items the dense kernel takes, which stay with
// the per-item kernel, and how many lanes an item gets.  No HIP: nwv_bls.hip runs it before the
// key-sum launches, tests/hostemu/bls_apk_dense_hostemu.cpp exposes it to the tests.
//
// The dense kernel (k_blsd_apk) packs 64 / L items into a wave, L lanes an item.  It takes the
// items whose keys all sit in the serving device's key cache (kmode[i] = 1) and whose list names
// at least two keys; one-key items, empty lists and items naming an uncached key keep the per-item
// code (blsw_apk_item through an item list), so AGGR_MISMATCH, the one-key copy and the order of
// the first bad key stay in one place.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace nwv {

// lanes per item: the largest L of 4, 8, 16 that still fills 65,536 lanes (the chip's 1,024 SIMDs
// with one wave each) over n_dense items, else 4; `forced` (NWV_BLS_APK_LANES) wins when it is one
// of the three
inline uint32_t apk_dense_lanes(size_t n_dense, unsigned long forced = 0) {
    if (forced == 4 || forced == 8 || forced == 16) return (uint32_t)forced;
    for (uint32_t l = 16; l > 4; l /= 2)
        if (n_dense * l >= 65536) return l;
    return 4;
}

struct ApkDenseSplit {
    std::vector<uint32_t> dense, rest;  // the call's items, ascending in each list
};
// kmode may be null (no key-side items: everything stays with the per-item kernel)
inline void apk_dense_split(size_t n, const uint32_t* kmode, const uint32_t* pk_cnt, ApkDenseSplit& s) {
    s.dense.clear();
    s.rest.clear();
    for (size_t i = 0; i < n; i++) (kmode && kmode[i] && pk_cnt[i] >= 2 ? s.dense : s.rest).push_back((uint32_t)i);
}

}  // namespace nwv
