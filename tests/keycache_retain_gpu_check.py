"""Child process of tests/test_gpu_keycache_retain.py: nwv_keycache_retain (the epoch change of the
Ed25519 key cache: nwv_host.hip, keycache_alloc.h) with inputs from tests/keycache_cases.py and the
check / check3 of tests/keycache_gpu_check.py (a case through nwv_ed25519_verify_batch_keyed with
and without verdict bits, on the default, NWV_FLAG_NO_TINY and NWV_FLAG_NO_KEYCACHE contexts, with
the nwv_diag_counters_ex delta of each call).  The library reads NWV_COMB_KEYS and
NWV_DEVICE_REPLICAS once per process, so the parent starts one child per value.

  --parts tables     tables come back, a reused slot / table holds the new key (NWV_COMB_KEYS=4)
          overlap    a committee that shares three members with the one before
          fp         the fingerprint of the registered list after a retain; NWV_FLAG_NO_KEYCACHE
          staged     staged keyed batches pin their slots (also under NWV_STAGE_CHAIN=0)
          threads    keyed calls beside retain / register
          full       the full slot table recovers (NWV_COMB_KEYS=8)
          replicas   every device object (NWV_DEVICE_REPLICAS=3)

Prints one JSON line."""
import argparse
import json
import os
import random
import sys
import threading
import time
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import keycache_cases as kc  # noqa: E402
import oracle_ffi as of  # noqa: E402
from keycache_gpu_check import S, check, check3, close_forms, fast, open_forms  # noqa: E402

OUT = ("slots_retired", "combs_retired", "pinned_kept", "used")


def out4(d):
    return [d[k] for k in OUT]


def retain_all(engs, keys):
    """the call on the three contexts: [default's out, no_tiny's, no_keycache's]"""
    return [out4(engs[f].keycache_retain(keys)) for f in ("default", "no_tiny", "no_keycache")]


def register_all(engs, keys):
    for e in engs.values():
        e.keycache_register(keys)


def stats2(engs):
    return [engs[f].keycache_stats() for f in ("default", "no_tiny")]


def batches(checks, engs, com, path, name, seed, sizes=(8, 100)):
    """an honest and a forged batch of each size by the committee, on the three contexts; path:
    "fast" (tiny / comb by size) or "msm" """
    for n in sizes:
        v = kc.valid(com, n, seed + n)
        p = fast(n) if path == "fast" else path
        check3(checks, engs, v, p, f"{name}_{n}_valid")
        check3(checks, engs, kc.forged(v, seed + 50 + n, wrong=2), p, f"{name}_{n}_forged")


def crossed(B, A, n, seed, pairs):
    """n honest signatures by B, then position p named under B_j and signed by A_k for the p-th
    (j, k) of pairs: the signature a cache that still held A_k's record or table in B_j's place
    would accept"""
    keys, kidx, sigs, msgs, _ = kc.valid(B, n, seed)
    kidx, sigs = list(kidx), list(sigs)
    for p, (j, k) in enumerate(pairs):
        kidx[p], sigs[p] = j, of.sign(A[0][k], msgs[p])
    return keys, kidx, sigs, list(msgs), kc.verdicts(keys, kidx, sigs, msgs)


# ---- tables: NWV_COMB_KEYS=4 --------------------------------------------------------------------
def part_tables():
    A, B = kc.committee(4, 1100), kc.committee(4, 1101)
    engs = open_forms()
    r = {"comb_keys": os.environ.get("NWV_COMB_KEYS")}
    checks = r["checks"] = []
    register_all(engs, A[1])
    r["stats_A"] = stats2(engs)
    register_all(engs, B[1])
    r["stats_AB"] = stats2(engs)
    batches(checks, engs, B, "msm", "B_before", 1110)  # no table left for B: today's behaviour
    r["retain_B"] = retain_all(engs, B[1])
    r["stats_retained"] = stats2(engs)
    register_all(engs, B[1])
    r["stats_B"] = stats2(engs)
    batches(checks, engs, B, "fast", "B_after", 1120)
    # every (B_j, A_k): a signature by A_k named under B_j, whichever slot or table B_j took over
    pairs = [(j, k) for j in range(4) for k in range(4)]
    for h in (0, 1):
        c = crossed(B, A, 8, 1130 + h, pairs[8 * h:8 * h + 8])
        assert [i for i, w in enumerate(c[4]) if not w] == list(range(8))
        # (eight rejections out of eight: the parent reads these apart from the mixed batches)
        r.setdefault("crossed8", []).extend(check(engs[f], c, "tiny" if f == "default" else "msm", f"crossed8_{h}", f)
                                            for f in ("default", "no_tiny", "no_keycache"))
    c = crossed(B, A, 100, 1150, pairs)
    assert [i for i, w in enumerate(c[4]) if not w] == list(range(16))
    check3(checks, engs, c, "comb", "crossed_100_forged")
    r["stats_before_A_again"] = stats2(engs)
    # A's own batches: fresh slots (the ones it had), no tables, the cached MSM
    batches(checks, engs, A, "msm", "A_again", 1160)
    r["stats_end"] = stats2(engs)
    r["stats_no_keycache"] = engs["no_keycache"].keycache_stats()
    close_forms(engs)
    return r


# ---- overlap ------------------------------------------------------------------------------------
def part_overlap():
    A, Bx = kc.committee(10, 1200), kc.committee(7, 1201)
    B = (A[0][7:] + Bx[0], A[1][7:] + Bx[1])  # shares three members with A
    shared = (A[0][7:], A[1][7:])
    engs = open_forms()
    r = {}
    checks = r["checks"] = []
    register_all(engs, A[1])
    r["stats_A"] = stats2(engs)
    r["retain_B"] = retain_all(engs, B[1])
    r["stats_retained"] = stats2(engs)
    batches(checks, engs, shared, "fast", "shared_before", 1210)  # kept: records and tables, not refilled
    r["stats_before_register"] = stats2(engs)
    register_all(engs, B[1])
    r["stats_B"] = stats2(engs)
    batches(checks, engs, shared, "fast", "shared_after", 1220)
    batches(checks, engs, B, "fast", "B", 1230)
    r["retain_B_again"] = retain_all(engs, B[1] + B[1][:2])  # nothing to retire; duplicates allowed
    close_forms(engs)
    return r


# ---- fp: the registered list's fingerprint, and NWV_FLAG_NO_KEYCACHE ----------------------------
def part_fp():
    A = kc.committee(10, 1300)
    engs = open_forms()
    r = {}
    checks = r["checks"] = []
    r["retain_before_anything"] = retain_all(engs, [])
    register_all(engs, A[1])
    r["stats_A"] = stats2(engs)
    stray = kc.committee(3, 1301)[1]
    r["retain_A_and_strangers"] = retain_all(engs, A[1] + stray)  # names that are not cached: ignored
    r["stats_kept"] = stats2(engs)
    r["retain_none"] = retain_all(engs, [])
    r["stats_retained"] = stats2(engs)
    register_all(engs, A[1])  # the same list again: must do the work
    r["stats_A_again"] = stats2(engs)
    batches(checks, engs, A, "fast", "A_again", 1310)
    nk = engs["no_keycache"]
    r["no_keycache"] = {"retain_list": out4(nk.keycache_retain(A[1])), "retain_none": out4(nk.keycache_retain([])),
                        "stats": nk.keycache_stats()}
    close_forms(engs)
    return r


# ---- staged -------------------------------------------------------------------------------------
def part_staged():
    import narwhal_amd
    from narwhal_amd import _lib
    e = narwhal_amd.Engine(device=0)
    A, N = kc.committee(10, 1400), kc.committee(10, 1402)
    e.keycache_register(A[1])
    v = kc.valid(A, 100, 1401, signers=range(6))  # six of A's keys are staged, four are not
    cases = {"valid": v, "forged": kc.forge_one(v, 37)}
    r = {"stage_chain": os.environ.get("NWV_STAGE_CHAIN"), "stats_before": e.keycache_stats(),
         "distinct_staged": len(set(v[1]))}
    staged = {}
    for nm, (keys, kidx, sigs, msgs, _) in cases.items():
        arena, offs, lens = _lib.pack_messages(msgs)
        staged[nm] = e.stage_keyed(np.frombuffer(b"".join(keys), dtype=np.uint8), np.asarray(kidx, dtype=np.uint32),
                                   np.frombuffer(b"".join(sigs), dtype=np.uint8), arena, offs, lens)
    got = {nm: [] for nm in cases}

    def run_all():
        for nm, st in staged.items():
            st.run(mode=1, seed=S)
            allv, bits = st.fetch()
            got[nm].append([bool(allv), [bool(b) for b in bits] == cases[nm][4]])

    run_all()
    r["retain_none"] = out4(e.keycache_retain([]))
    r["stats_retained"] = e.keycache_stats()
    e.keycache_register(N[1])  # takes the four freed slots and tables first, then new ones
    r["stats_N"] = e.keycache_stats()
    run_all()
    run_all()
    r["runs"] = got  # per run: [batch verdict, bits == oracle's]
    r["want_all"] = {nm: all(c[4]) for nm, c in cases.items()}
    r["rejected"] = {nm: c[4].count(False) for nm, c in cases.items()}
    r["tally"] = {nm: list(st.run_tally()) for nm, st in staged.items()}
    w = kc.valid(N, 100, 1404)
    r["checks"] = [check(e, w, "comb", "new_keys_valid"), check(e, kc.forged(w, 1405, wrong=2), "comb", "new_keys_forged"),
                   check(e, v, "comb", "A_pinned_unstaged_valid")]  # the six pinned keys kept their tables
    staged["valid"].free()
    r["retain_one_freed"] = out4(e.keycache_retain(N[1]))  # the other batch still pins the six
    staged["forged"].free()
    r["retain_both_freed"] = out4(e.keycache_retain(N[1]))
    r["retain_none_at_end"] = out4(e.keycache_retain([]))
    r["stats_end"] = e.keycache_stats()
    e.close()
    return r


# ---- threads ------------------------------------------------------------------------------------
def part_threads():
    import narwhal_amd
    e = narwhal_amd.Engine(device=0)
    A, B = kc.committee(10, 1500), kc.committee(10, 1501)
    U = kc.joined(A, B)
    e.keycache_register(A[1])
    jobs = [kc.forged(kc.valid(U, n, 1510 + n), 1520 + n, wrong=2) for n in (8, 100)]
    out = [[], []]

    def work(t):
        keys, kidx, sigs, msgs, _ = jobs[t]
        for _ in range(20):
            out[t].append(e.verify_batch_keyed(keys, kidx, sigs, msgs))

    for keys, kidx, sigs, msgs, _ in jobs:  # (lanes and workspaces exist before the overlap starts)
        e.verify_batch_keyed(keys, kidx, sigs, msgs)
    th = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(2)]
    for x in th:
        x.start()
    done_at, outs = [], []
    for _ in range(10):
        for com in (A, B):
            outs.append(out4(e.keycache_retain(com[1])))
            e.keycache_register(com[1])
        done_at.append(len(out[0]) + len(out[1]))
    for x in th:
        x.join(timeout=60)
    r = {"alive": [x.is_alive() for x in th], "calls": [len(o) for o in out], "main_rounds": len(done_at),
         "bits_eq": [all(bits == jobs[t][4] for _, bits in out[t]) for t in range(2)],
         "ok_eq": [all(ok == all(jobs[t][4]) for ok, _ in out[t]) for t in range(2)],
         "rejected": [j[4].count(False) for j in jobs],
         "both_committees_named": [len(set(j[1]) & set(range(10))) > 0 and len(set(j[1]) & set(range(10, 20))) > 0
                                   for j in jobs],
         "sets_differ": len({tuple(i for i, w in enumerate(j[4]) if not w) for j in jobs}) == 2,
         "pinned_kept": sorted({o[2] for o in outs}),
         "calls_done_after_each_round": done_at}  # (how far the two overlapped; not asserted)
    if not any(r["alive"]):
        # the cache is coherent afterwards: only B and what the last calls cached themselves
        r["retain_B_at_end"] = out4(e.keycache_retain(B[1]))
        r["stats_end"] = e.keycache_stats()
        v = kc.valid(B, 100, 1530)
        r["checks"] = [check(e, v, "comb", "B_at_end_valid"), check(e, kc.forged(v, 1531, wrong=2), "comb", "B_at_end_forged")]
        e.close()
    return r


# ---- full: NWV_COMB_KEYS=8 ----------------------------------------------------------------------
def part_full():
    import narwhal_amd
    e = narwhal_amd.Engine(device=0)
    C, F = kc.committee(8, 1600), kc.committee(2, 1603)
    r = {"comb_keys": os.environ.get("NWV_COMB_KEYS")}
    checks = r["checks"] = []
    t0 = time.time()
    e.keycache_register(C[1])
    cap = e.keycache_stats()["cap"]
    rnd = random.Random(1601)
    r["filler_calls"] = 0
    for _ in range(8):  # (four calls fill the table; bounded either way)
        room = cap - e.keycache_stats()["used"]
        if room <= 0:
            break
        e.keycache_register([rnd.randbytes(32) for _ in range(min(20000, room))])
        r["filler_calls"] += 1
    r["fill_seconds"] = round(time.time() - t0, 2)
    r["stats_full"] = e.keycache_stats()
    fresh = kc.valid(F, 40, 1610)
    assert set(fresh[1]) == {0, 1}
    checks.append(check(e, fresh, "msm", "fresh_when_full_valid"))
    checks.append(check(e, kc.forged(fresh, 1611, wrong=2), "msm", "fresh_when_full_forged"))
    r["stats_after_fresh_when_full"] = e.keycache_stats()
    t1 = time.time()
    r["retain_C"] = out4(e.keycache_retain(C[1]))
    r["retain_seconds"] = round(time.time() - t1, 3)
    r["stats_retained"] = e.keycache_stats()
    checks.append(check(e, fresh, "msm", "fresh_after_retain_valid"))
    checks.append(check(e, kc.forged(fresh, 1611, wrong=2), "msm", "fresh_after_retain_forged"))
    r["stats_after_fresh"] = e.keycache_stats()
    for n in (8, 100):
        v = kc.valid(C, n, 1620 + n)
        checks.append(check(e, v, fast(n), f"C_{n}_valid"))
        checks.append(check(e, kc.forged(v, 1630 + n, wrong=2), fast(n), f"C_{n}_forged"))
    e.close()
    return r


# ---- replicas: NWV_DEVICE_REPLICAS=3 ------------------------------------------------------------
def part_replicas():
    import narwhal_amd
    e = narwhal_amd.Engine(device=0)
    A = kc.committee(10, 1700)
    e.keycache_register(A[1])
    r = {"replicas": os.environ.get("NWV_DEVICE_REPLICAS"), "devices": e.device_count,
         "stats_A": [e.keycache_stats(i) for i in range(e.device_count)]}
    r["retain"] = out4(e.keycache_retain(A[1][:4]))
    r["stats_retained"] = [e.keycache_stats(i) for i in range(e.device_count)]
    kept = (A[0][:4], A[1][:4])
    checks = r["checks"] = []
    for n in (8, 100):
        v = kc.valid(kept, n, 1710 + n)
        checks.append(check(e, v, fast(n), f"kept_{n}_valid"))
        checks.append(check(e, kc.forged(v, 1720 + n, wrong=2), fast(n), f"kept_{n}_forged"))
    r["retain_none"] = out4(e.keycache_retain([]))
    r["stats_end"] = [e.keycache_stats(i) for i in range(e.device_count)]
    e.close()
    return r


PARTS = {"tables": part_tables, "overlap": part_overlap, "fp": part_fp, "staged": part_staged,
         "threads": part_threads, "full": part_full, "replicas": part_replicas}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", required=True)
    a = ap.parse_args()
    out = {}
    for part in a.parts.split(","):
        t0 = time.time()
        try:
            out[part] = PARTS[part]()
        except Exception:  # the parent reports it against the part's own tests
            out[part] = {"error": traceback.format_exc()[-3000:]}
        out[part]["seconds"] = round(time.time() - t0, 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
