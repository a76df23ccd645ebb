// ed_plan.h -- which path an Ed25519 batch takes on its device (host code, no HIP): a pure function
// of the batch's size, the context's flags, what keyed staging found out about the batch's keys, and
// the limits in force.  Keyed staging calls it once, at its end, and leaves the plan on the buffers;
// batch_on_device switches on it.  Un-keyed and staged batches get the default plan, Msm or Each by
// the flags and msm_min (nwv_staged_run launches a staged batch itself and never consults a plan).
// DESIGN.md 3.8 has the rules as a table.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/nwv.h"

namespace nwv {

enum class EdPath { Tiny, Comb, Msm, Each };
struct EdPlan {
    EdPath path = EdPath::Msm;  // (what flags 0 and msm_min 0 give: a buffer set before any staging)
    bool comb_pass = false;     // the per-signature pass, if one runs, is k_ed_comb_pass over the key combs
};
// the one-launch kernel's capacity; the context's comb_batch_max, 0 when the call splits over
// devices; the device's comb_pass_max; NWV_MSM_MIN_N
struct EdLimits {
    size_t tiny_max = 0, comb_max = 0, pass_max = 0, msm_min = 0;
};
// the context flags that force a path: the comb path, the comb pass and a typed call's one-launch
// form need none of them set
constexpr uint32_t ED_FORCES_PATH = NWV_FLAG_NO_TINY | NWV_FLAG_MSM_ALWAYS | NWV_FLAG_MSM_NEVER;

// Whether the Tiny, Comb or comb-pass rule holds but for all_tables: only then is every signature's
// comb table looked up.  keyed_cached: the keyed batch got key cache slots; staged: the batch is
// staged for nwv_staged_run (no rule is offered, so pass_max counts as 0).
inline bool ed_plan_wants_tables(size_t n, uint32_t flags, bool keyed_cached, bool staged, const EdLimits& lim) {
    if (!keyed_cached || staged || n == 0) return false;
    // (MSM_ALWAYS does not exclude the tiny path: the open ADVICE.md finding, kept as it is)
    if (n <= lim.tiny_max) return !(flags & (NWV_FLAG_NO_TINY | NWV_FLAG_MSM_NEVER));
    return (n <= lim.comb_max || n <= lim.pass_max) && !(flags & ED_FORCES_PATH);
}

// all_tables: every signature's key has a comb table (looked at only when ed_plan_wants_tables)
inline EdPlan ed_plan(size_t n, uint32_t flags, bool keyed_cached, bool all_tables, bool staged, const EdLimits& lim) {
    EdPlan p;
    if (!((flags & NWV_FLAG_MSM_ALWAYS) || (!(flags & NWV_FLAG_MSM_NEVER) && n >= lim.msm_min))) p.path = EdPath::Each;
    if (!all_tables || !ed_plan_wants_tables(n, flags, keyed_cached, staged, lim)) return p;
    if (n <= lim.tiny_max) p.path = EdPath::Tiny;       // 1 <= n <= tiny_max
    else if (n <= lim.comb_max) p.path = EdPath::Comb;  // tiny_max < n <= comb_max
    else p.comb_pass = true;                            // max(tiny_max, comb_max) < n <= pass_max
    return p;
}

}  // namespace nwv
