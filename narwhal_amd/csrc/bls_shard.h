// bls_shard.h -- BLS12-381 calls over a multi-device context (host code, SURVEY §8 e).
//
// The reference verifies certificates independently (validate_certificates,
// primary/src/block_synchronizer/responses.rs:115-129; the Core's queued headers and votes), so a
// nwv_bls_verify_many call splits its items by index into contiguous ranges, one per device, and
// every range's statuses land at their own indices: no cross-device exchange, exactly as the
// Ed25519 calls shard (nwv_host.hip for_shards).  Small calls stay on one device, the least loaded
// one (place.h): each item's pairing check is latency-bound on one wave, so spreading 100 items
// over 8 devices buys nothing and costs a host thread per device.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

#include "shard.h"

namespace nwv {

// [lo, hi) item ranges over at most ndev devices, near-equal, each of at least min_per items (so a
// call of n < 2 min_per items is one range); place.h maps the ranges to devices
inline std::vector<std::pair<size_t, size_t>> bls_shard_ranges(size_t n, size_t ndev, size_t min_per) {
    std::vector<std::pair<size_t, size_t>> r;
    if (n == 0) return r;
    if (min_per == 0) min_per = 1;
    size_t k = n / min_per;
    if (k > ndev) k = ndev;
    if (k == 0) k = 1;
    for (size_t j = 0; j < k; j++) r.push_back({n * j / k, n * (j + 1) / k});
    return r;
}

// for_ranges (shard.h) under the name the BLS code and its host stub use
template <class Fn>
int bls_for_ranges(const std::vector<std::pair<size_t, size_t>>& ranges, Fn fn) {
    return for_ranges(ranges, std::move(fn));
}

}  // namespace nwv
