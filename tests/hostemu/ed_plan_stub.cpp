// The Ed25519 path choice (narwhal_amd/csrc/ed_plan.h) behind a C interface, with no HIP:
// tests/test_ed_plan_host.py compares it with a literal table.
#include <cstdint>

#include "../../narwhal_amd/csrc/ed_plan.h"

extern "C" {

// path (0 Tiny, 1 Comb, 2 Msm, 3 Each) | comb_pass << 8; lim: tiny_max, comb_max, pass_max, msm_min
int ep_plan(uint64_t n, uint32_t flags, int keyed_cached, int all_tables, int staged, const uint64_t lim[4]) {
    const nwv::EdLimits l{(size_t)lim[0], (size_t)lim[1], (size_t)lim[2], (size_t)lim[3]};
    const nwv::EdPlan p = nwv::ed_plan((size_t)n, flags, keyed_cached != 0, all_tables != 0, staged != 0, l);
    return (int)p.path | (p.comb_pass ? 256 : 0);
}

int ep_wants_tables(uint64_t n, uint32_t flags, int keyed_cached, int staged, const uint64_t lim[4]) {
    const nwv::EdLimits l{(size_t)lim[0], (size_t)lim[1], (size_t)lim[2], (size_t)lim[3]};
    return nwv::ed_plan_wants_tables((size_t)n, flags, keyed_cached != 0, staged != 0, l) ? 1 : 0;
}

// what a buffer set holds before any staging
int ep_default_plan(void) {
    const nwv::EdPlan p;
    return (int)p.path | (p.comb_pass ? 256 : 0);
}

uint32_t ep_forces_path_mask(void) { return nwv::ED_FORCES_PATH; }

// the flag bits by name, so the test's table does not restate include/nwv.h: 0 NO_TINY,
// 1 MSM_ALWAYS, 2 MSM_NEVER
uint32_t ep_flag(int which) {
    return which == 0 ? NWV_FLAG_NO_TINY : which == 1 ? NWV_FLAG_MSM_ALWAYS : which == 2 ? NWV_FLAG_MSM_NEVER : 0u;
}

}  // extern "C"
