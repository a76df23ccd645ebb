// The key-transposed batch check's host pass (narwhal_amd/csrc/bls_key_batch.h) behind a C
// interface, with no HIP: tests/test_bls_key_batch_host.py compares the plan (groups, key entries,
// the key-major lists) and the per-item launch ranges with a plain Python transposition.
#include <cstdint>
#include <cstring>

#include "../../narwhal_amd/csrc/bls_key_batch.h"

extern "C" {

void* bkb_plan(uint64_t n, const uint8_t* ok, const uint8_t* elig, const uint32_t* pk_off, const uint32_t* pk_cnt,
               const uint32_t* slot_idx, uint32_t slot_cap, uint32_t group, uint32_t ratio) {
    auto* p = new nwv::KeyBatchPlan;
    nwv::key_batch_plan((size_t)n, ok, elig, pk_off, pk_cnt, slot_idx, slot_cap, group, ratio, *p);
    return p;
}
void bkb_free(void* p) { delete static_cast<nwv::KeyBatchPlan*>(p); }
// out: run, n_ok, n_eligible, groups, entries, millers, then the lengths of items, gfirst, goff,
// eslot, egrp, coff, cidx, outside
void bkb_sizes(void* h, uint64_t out[14]) {
    const auto& p = *static_cast<nwv::KeyBatchPlan*>(h);
    const uint64_t v[14] = {p.run ? 1u : 0u, p.n_ok, p.n_eligible, p.groups(), p.entries(), p.millers(),
                            p.items.size(), p.gfirst.size(), p.goff.size(), p.eslot.size(), p.egrp.size(),
                            p.coff.size(), p.cidx.size(), p.outside.size()};
    std::memcpy(out, v, sizeof v);
}
// which: 0 items, 1 gfirst, 2 goff, 3 eslot, 4 egrp, 5 coff, 6 cidx, 7 outside
void bkb_get(void* h, int which, uint32_t* out) {
    const auto& p = *static_cast<nwv::KeyBatchPlan*>(h);
    const std::vector<uint32_t>* v[8] = {&p.items, &p.gfirst, &p.goff, &p.eslot, &p.egrp, &p.coff, &p.cidx, &p.outside};
    if (which < 0 || which > 7 || v[which]->empty()) return;
    std::memcpy(out, v[which]->data(), 4 * v[which]->size());
}
// the ranges of recheck_ranges as lo, hi pairs into out (room for 2 n words); returns their number
uint64_t bkb_ranges(uint64_t n, const uint8_t* need, uint64_t gap, uint64_t* out) {
    const auto r = nwv::recheck_ranges((size_t)n, need, (size_t)gap);
    for (size_t k = 0; k < r.size(); k++) {
        out[2 * k] = r[k].first;
        out[2 * k + 1] = r[k].second;
    }
    return r.size();
}

}  // extern "C"
