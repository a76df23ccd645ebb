// bls_key_batch.h -- the host side of the key-transposed batch check of large BLS calls
// (nwv_bls_set_key_batch_min): which items enter the check, how they are grouped,
// and each group's key-major list.  No HIP: nwv_bls.hip runs it between the pre-pairing kernels
// and the check, tests/test_bls_key_batch_host.py drives it through tests/hostemu/bls_key_batch_stub.cpp.
//
// The check regroups the random linear combination of a group's items by key:
//   prod_i e([r_i] H_i, apk_i) e(-sum_i [r_i] sig_i, g2) = prod_k e(T_k, pk_k) e(-S, g2),
//   T_k = sum over the occurrences of key k in the group's key lists of [r_i] H_i,
// so a group costs one Miller loop per distinct key plus one, whatever its number of items.
//
// An item is ELIGIBLE when its pre-pairing statuses are OK, its signature is not the identity and
// every key of its list sits in the serving device's key cache (a slot below the cache's
// capacity).  The eligible items, in the caller's order, are cut into consecutive groups of
// `group` items.  A group whose distinct keys + 1 exceed 1 / ratio of its items gains nothing and
// is dropped (ratio 0: no group is dropped); the kept groups close up, so group g holds
// items[g group, min((g + 1) group, items.size())): only the last eligible group can be short, and
// it stays last among the kept ones.  The plan does not run when fewer than half of the OK items
// are eligible or no group is kept; the call then takes the path it takes with the setting off.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace nwv {

struct KeyBatchPlan {
    bool run = false;
    size_t n_ok = 0, n_eligible = 0;  // items whose pre-pairing statuses are OK; the eligible ones
    std::vector<uint32_t> items;      // the kept groups' items (caller's indices), group after group
    std::vector<uint32_t> gfirst;     // groups + 1: group g is positions [gfirst[g], gfirst[g + 1]) of items
    std::vector<uint32_t> goff;       // groups + 1: group g's key entries are [goff[g], goff[g + 1])
    std::vector<uint32_t> eslot;      // per key entry: the key's cache slot (first-occurrence order in its group)
    std::vector<uint32_t> egrp;       // per key entry: its group
    std::vector<uint32_t> coff;       // key entries + 1: entry m's occurrences are cidx[coff[m], coff[m + 1])
    std::vector<uint32_t> cidx;       // positions in `items`, one per occurrence of the key in an item's list
    std::vector<uint32_t> outside;    // OK items in no kept group, ascending: checked per item
    size_t groups() const { return gfirst.empty() ? 0 : gfirst.size() - 1; }
    size_t entries() const { return eslot.size(); }
    // Miller loops of the check: the key entries and one signature entry a group
    size_t millers() const { return entries() + groups(); }
};

// ok[i]: item i's decode, G1 and key statuses are all OK.  elig[i]: beyond that, the item may
// enter the check (the caller has looked at the signature and at where the keys live); read only
// where ok[i].  slot_idx[pk_off[i] .. + pk_cnt[i]): the cache slots of an eligible item's keys,
// each below slot_cap.
inline void key_batch_plan(size_t n, const uint8_t* ok, const uint8_t* elig, const uint32_t* pk_off,
                           const uint32_t* pk_cnt, const uint32_t* slot_idx, uint32_t slot_cap, uint32_t group,
                           uint32_t ratio, KeyBatchPlan& P) {
    P = KeyBatchPlan();
    if (group < 1) group = 1;
    std::vector<uint32_t> el;
    for (size_t i = 0; i < n; i++) {
        if (!ok[i]) continue;
        P.n_ok++;
        if (elig[i] && pk_cnt[i] > 0) el.push_back((uint32_t)i);
    }
    P.n_eligible = el.size();
    auto all_outside = [&]() {
        P.outside.clear();
        for (size_t i = 0; i < n; i++)
            if (ok[i]) P.outside.push_back((uint32_t)i);
    };
    if (el.empty() || 2 * P.n_eligible < P.n_ok) {
        all_outside();
        return;
    }
    // local[s]: key entry of slot s in the group being built (stamped by group, so no clearing)
    std::vector<uint32_t> local(slot_cap, 0), stamp(slot_cap, 0xffffffffu), cnt, fill;
    std::vector<uint8_t> kept(n, 0);
    P.gfirst.push_back(0);
    P.goff.push_back(0);
    P.coff.push_back(0);
    uint32_t g_try = 0;
    for (size_t lo = 0; lo < el.size(); lo += group, g_try++) {
        const size_t hi = lo + group < el.size() ? lo + group : el.size();
        const uint32_t e0 = (uint32_t)P.eslot.size();
        cnt.clear();
        for (size_t e = lo; e < hi; e++) {
            const uint32_t i = el[e];
            for (uint32_t j = 0; j < pk_cnt[i]; j++) {
                const uint32_t s = slot_idx[pk_off[i] + j];
                if (stamp[s] != g_try) {
                    stamp[s] = g_try;
                    local[s] = (uint32_t)cnt.size();
                    cnt.push_back(0);
                    P.eslot.push_back(s);
                }
                cnt[local[s]]++;
            }
        }
        const size_t keys = cnt.size(), size = hi - lo;
        if (ratio && (keys + 1) * (size_t)ratio > size) {  // dropped: its items go per item
            P.eslot.resize(e0);
            continue;
        }
        const uint32_t g = (uint32_t)P.groups(), p0 = (uint32_t)P.items.size();
        uint32_t at = P.coff.back();
        fill.assign(keys, 0);
        for (size_t k = 0; k < keys; k++) {
            fill[k] = at;
            at += cnt[k];
            P.coff.push_back(at);
            P.egrp.push_back(g);
        }
        P.cidx.resize(at);
        for (size_t e = lo; e < hi; e++) {
            const uint32_t i = el[e], pos = p0 + (uint32_t)(e - lo);
            for (uint32_t j = 0; j < pk_cnt[i]; j++) P.cidx[fill[local[slot_idx[pk_off[i] + j]]]++] = pos;
            P.items.push_back(i);
            kept[i] = 1;
        }
        P.gfirst.push_back((uint32_t)P.items.size());
        P.goff.push_back((uint32_t)P.eslot.size());
    }
    if (P.groups() == 0) {
        P = KeyBatchPlan{false, P.n_ok, P.n_eligible};
        all_outside();
        return;
    }
    for (size_t i = 0; i < n; i++)
        if (ok[i] && !kept[i]) P.outside.push_back((uint32_t)i);
    P.run = true;
}

// The per-item launches behind this check and behind the wave batch check: need[i] != 0 marks an
// item that must run the per-item kernel (an OK item outside the groups, an item of a rejected
// group; the wave batch check marks every item of a rejected group).  A launch over a few items
// costs one item's whole chain, so marked items less than `gap` items apart share one launch with
// whatever lies between them.  Returns the half-open ranges, ascending.
inline std::vector<std::pair<size_t, size_t>> recheck_ranges(size_t n, const uint8_t* need, size_t gap) {
    std::vector<std::pair<size_t, size_t>> r;
    for (size_t i = 0; i < n; i++) {
        if (!need[i]) continue;
        if (!r.empty() && i - r.back().second < gap) r.back().second = i + 1;
        else r.push_back({i, i + 1});
    }
    return r;
}
// the function's name while it served this check alone (host stubs built against that name still compile)
inline std::vector<std::pair<size_t, size_t>> key_batch_ranges(size_t n, const uint8_t* need, size_t gap) {
    return recheck_ranges(n, need, gap);
}

}  // namespace nwv
