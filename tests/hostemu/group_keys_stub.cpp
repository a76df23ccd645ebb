// The key grouping of the trait surface (narwhal_amd/csrc/group_keys.h) behind a C interface, with
// no HIP: tests/test_group_keys_host.py drives it, and tools/trait_grouped.py times it.
#include <chrono>
#include <cstdint>
#include <cstring>

#include "../../narwhal_amd/csrc/group_keys.h"

extern "C" {

void* gk_new(void) { return new nwv::KeyGrouper; }
void gk_free(void* g) { delete static_cast<nwv::KeyGrouper*>(g); }

// Group n keys.  Returns the number of distinct keys, or -1 if there were more than max_distinct
// (0: no limit).  idx_out (n words) and keys_out (32 bytes per distinct key; room for n) may be null.
int64_t gk_group(void* g, const uint8_t* keys, uint64_t n, uint64_t max_distinct, uint32_t* idx_out,
                 uint8_t* keys_out) {
    nwv::KeyGrouper& kg = *static_cast<nwv::KeyGrouper*>(g);
    if (!kg.group(keys, (size_t)n, max_distinct ? (size_t)max_distinct : SIZE_MAX)) return -1;
    if (idx_out && n) std::memcpy(idx_out, kg.key_idx(), 4 * (size_t)n);
    if (keys_out && kg.n_distinct()) std::memcpy(keys_out, kg.distinct(), 32 * kg.n_distinct());
    return (int64_t)kg.n_distinct();
}

// the same on a grouper that lives in the calling thread, as the engine's does
int64_t gk_group_tls(const uint8_t* keys, uint64_t n, uint32_t* idx_out, uint8_t* keys_out, uint64_t caps_out[2]) {
    thread_local nwv::KeyGrouper kg;
    const int64_t m = gk_group(&kg, keys, n, 0, idx_out, keys_out);
    if (caps_out) {
        caps_out[0] = kg.table_capacity();
        caps_out[1] = kg.out_capacity();
    }
    return m;
}

// out[0] table entries, [1] bytes of output capacity
void gk_caps(void* g, uint64_t out[2]) {
    const nwv::KeyGrouper& kg = *static_cast<nwv::KeyGrouper*>(g);
    out[0] = kg.table_capacity();
    out[1] = kg.out_capacity();
}

// `reps` groupings of the same keys, one after another: nanoseconds per grouping
double gk_time_ns(void* g, const uint8_t* keys, uint64_t n, uint64_t max_distinct, uint64_t reps) {
    nwv::KeyGrouper& kg = *static_cast<nwv::KeyGrouper*>(g);
    const size_t lim = max_distinct ? (size_t)max_distinct : SIZE_MAX;
    kg.group(keys, (size_t)n, lim);
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t sink = 0;
    for (uint64_t r = 0; r < reps; r++) sink += kg.group(keys, (size_t)n, lim) ? kg.n_distinct() : 0;
    const auto t1 = std::chrono::steady_clock::now();
    static volatile uint64_t keep;
    keep = sink;
    return std::chrono::duration<double, std::nano>(t1 - t0).count() / (double)(reps ? reps : 1);
}

}  // extern "C"
