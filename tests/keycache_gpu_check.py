"""Child process of tests/test_gpu_keycache.py: the committee key cache and the per-key comb tables
(nwv_host.hip KeyCache, keycache_slots, nwv_keycache_register, ed_stage_keyed's path choice) at
their capacity, epoch and alias edges, with inputs from tests/keycache_cases.py.  The library reads
NWV_COMB_KEYS once per process, so the parent starts one child per value.

A "check" is one case through nwv_ed25519_verify_batch_keyed twice, with verdict bits and without:
bits == the oracle's, both batch verdicts == all(oracle's), and the nwv_diag_counters_ex delta of
each call (the parent asserts the path from it).  Cases that name an engine form run on three
contexts: default, NWV_FLAG_NO_TINY (cached batch MSM) and NWV_FLAG_NO_KEYCACHE (uncached).

  --parts a   comb-table capacity (run under NWV_COMB_KEYS=4, and again under NWV_COMB_KEYS=0)
          b   epoch change, re-registration, duplicate keys
          c   wrong signer, swapped key bytes, one-byte variants of a key
          d   the full slot table (run under NWV_COMB_KEYS=8)
          e   staged keyed batches across later registrations (also under NWV_STAGE_CHAIN=0)
          f   registration beside verification on one context
          g   k_ed_comb above 64 verdict words, workspace growth, the default limit

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

S = bytes(range(1, 33))
FORMS = ("default", "no_tiny", "no_keycache")
G_SIZES = [300, 4097, 65, 4160, 129]


def _delta(a, b):
    return {k: b[k] - a[k] for k in b}


def open_forms():
    import narwhal_amd
    from narwhal_amd import _lib
    flags = {"default": 0, "no_tiny": _lib.NWV_FLAG_NO_TINY, "no_keycache": _lib.NWV_FLAG_NO_KEYCACHE}
    return {f: narwhal_amd.Engine(device=0, flags=flags[f]) for f in FORMS}


def close_forms(engs):
    for e in engs.values():
        e.close()


def check(eng, case, path, name, form="default"):
    keys, kidx, sigs, msgs, want = case
    r = {"name": name, "form": form, "path": path, "n": len(sigs), "rejected": want.count(False)}
    c0 = eng.diag_counters_ex()
    ok, bits = eng.verify_batch_keyed(keys, kidx, sigs, msgs)
    c1 = eng.diag_counters_ex()
    ok2, none = eng.verify_batch_keyed(keys, kidx, sigs, msgs, want_bits=False)
    c2 = eng.diag_counters_ex()
    r["bits_eq"] = bits == want
    if bits != want:
        r["differ_at"] = [i for i in range(len(want)) if bits[i] != want[i]][:8]
    r["ok_bits"] = ok == all(want)
    r["ok_nobits"] = ok2 == all(want) and none is None
    r["runs_bits"], r["runs_nobits"] = _delta(c0, c1), _delta(c1, c2)
    return r


def check3(checks, engs, case, path, name):
    """the case on the three engine forms: `path` on the default one, the MSM on the other two"""
    for f in FORMS:
        checks.append(check(engs[f], case, path if f == "default" else "msm", name, f))


def fast(n):
    return "tiny" if n <= 64 else "comb"


def single(eng, key, seed, name):
    """nwv_ed25519_pubkey_verify of an honest and of a forged signature by `key`"""
    from narwhal_amd import _lib
    msg = b"single " + name.encode()
    sig = of.sign(seed, msg)
    bad = sig[:40] + bytes([sig[40] ^ 1]) + sig[41:]
    c0 = eng.diag_counters_ex()
    rc = [eng.lib.nwv_ed25519_pubkey_verify(eng._h, key, msg, len(msg), s) for s in (sig, bad)]
    want = [_lib.NWV_OK if of.verify(key, s, msg) else _lib.NWV_ERR_SIGNATURE for s in (sig, bad)]
    return {"name": name, "rc": rc, "want": want, "runs": _delta(c0, eng.diag_counters_ex()),
            "want_is_ok_then_reject": want == [_lib.NWV_OK, _lib.NWV_ERR_SIGNATURE]}


def oracle_bits(keys, kidx, sigs, msgs):
    try:
        threads = len(os.sched_getaffinity(0))
    except AttributeError:
        threads = os.cpu_count() or 1
    pk, sig, msg, offs, lens = of.pack([(keys[k], s, m) for k, s, m in zip(kidx, sigs, msgs)])
    words = of.verify_each_mt(pk, sig, msg, offs, lens, max(1, min(16, threads)))
    return [bool(b) for b in np.unpackbits(words.view(np.uint8), bitorder="little")[:len(sigs)]]


def gpu_signed(eng, com, n, seed):
    """n signatures by the committee, made by the GPU signer; verdicts by the oracle"""
    seeds, keys = com
    rnd = random.Random(seed)
    kidx = [rnd.randrange(len(keys)) for _ in range(n)]
    msgs = [rnd.randbytes(rnd.choice(kc.MSG_LENS)) for _ in range(n)]
    _, sg = eng.sign_many([seeds[k] for k in kidx], msgs)
    sigs = [sg[64 * i:64 * i + 64].tobytes() for i in range(n)]
    return list(keys), kidx, sigs, msgs, oracle_bits(keys, kidx, sigs, msgs)


# ---- a: comb-table capacity ---------------------------------------------------------------------
def part_a():
    """six keys registered in one call under NWV_COMB_KEYS=4 (or 0): keys 0..3 get the tables"""
    com = kc.committee(6, 100)
    engs = open_forms()
    e = engs["default"]
    for eng in engs.values():
        eng.keycache_register(com[1])
    r = {"comb_keys": os.environ.get("NWV_COMB_KEYS"), "stats": e.keycache_stats(),
         "stats_no_tiny": engs["no_tiny"].keycache_stats(), "stats_no_keycache": engs["no_keycache"].keycache_stats()}
    tables = r["stats"]["comb_used"] > 0
    checks = r["checks"] = []
    for n in (8, 100):
        pure = kc.valid(com, n, 110 + n, signers=range(4))
        check3(checks, engs, pure, fast(n) if tables else "msm", f"pure_{n}_valid")
        f = kc.forged(pure, 120 + n)
        hp = kc.honest_positions(f, 3)
        # wrong signers among the keys with a table: the batch stays on its path
        fw = kc.wrong_signer(f, hp[:2], to=[(f[1][i] + 1) % 4 for i in hp[:2]])
        check3(checks, engs, fw, fast(n) if tables else "msm", f"pure_{n}_forged")
        for x in (4, 5):
            # one honest signature by a key without a table (two in the forged set, one of them
            # then named under a key with a table, and one by a key with a table named under the
            # other table-less key)
            check3(checks, engs, kc.signed_by(pure, com, hp[0], x), "msm", f"mixed{x}_{n}_valid")
            m = kc.signed_by(kc.signed_by(f, com, hp[0], x), com, hp[2], x)
            m = kc.wrong_signer(m, [hp[0], hp[1]], to=[1, 9 - x])
            assert x in m[1] and [i for i in hp if not m[4][i]] == hp[:2]
            check3(checks, engs, m, "msm", f"mixed{x}_{n}_forged")
    e.keycache_register(com[1])
    r["stats_same_list_again"] = e.keycache_stats()
    e.keycache_register(com[1][4:])
    r["stats_k4_k5_alone"] = e.keycache_stats()
    stray = kc.committee(1, 199)
    r["single"] = [single(e, com[1][0], com[0][0], "key0"), single(e, com[1][5], com[0][5], "key5"),
                   single(e, stray[1][0], stray[0][0], "unregistered")]
    r["stats_end"] = e.keycache_stats()
    close_forms(engs)
    return r


# ---- b: epoch change and duplicates -------------------------------------------------------------
def part_b():
    A, Bx, X = kc.committee(10, 200), kc.committee(7, 201), kc.committee(1, 202)
    B = (A[0][7:] + Bx[0], A[1][7:] + Bx[1])  # shares three members with A
    U = kc.joined(A, Bx)
    coms = {"A": A, "B": B, "U": U}
    cases = {}
    for nm, com in coms.items():
        for n in (8, 100):
            v = kc.valid(com, n, 210 + n + len(nm) + ord(nm))
            cases[nm, n] = (v, kc.forged(v, 220 + n, wrong=2))
    engs = open_forms()
    e = engs["default"]
    r = {"steps": []}
    checks = r["checks"] = []
    registered = set()
    for k, nm in enumerate(("A", "B", "A", "A")):
        for eng in engs.values():
            eng.keycache_register(coms[nm][1])
        registered |= set(coms[nm][1])
        step = {"registered": nm, "stats": e.keycache_stats(), "stats_no_tiny": engs["no_tiny"].keycache_stats()}
        for (cn, n), (v, f) in cases.items():
            path = fast(n) if set(coms[cn][1]) <= registered else "msm"
            check3(checks, engs, v, path, f"step{k}_{cn}_{n}_valid")
            check3(checks, engs, f, path, f"step{k}_{cn}_{n}_forged")
        step["stats_after_batches"] = e.keycache_stats()
        r["steps"].append(step)
    # one key's bytes twice in a registered list: one slot, one table
    before = e.keycache_stats()
    for eng in engs.values():
        eng.keycache_register([A[1][0], X[1][0], A[1][1], X[1][0]])
    r["dup_register"] = {"before": before, "after": e.keycache_stats()}
    AX = kc.joined((A[0][:1], A[1][:1]), X)
    v = kc.valid(AX, 8, 230)
    check3(checks, engs, v, "tiny", "dup_registered_key_valid")
    check3(checks, engs, kc.forged(v, 231, wrong=2), "tiny", "dup_registered_key_forged")
    # the same bytes at two indices of a keyed call's key list
    for n in (8, 100):
        d = kc.duplicate_key_list(cases["A", n][0])
        check3(checks, engs, d, fast(n), f"dup_list_{n}_valid")
        for idx in (d[0].index(d[0][-1]), len(d[0]) - 1):
            check3(checks, engs, kc.forge_one(d, d[1].index(idx)), fast(n), f"dup_list_{n}_forged_under_{idx}")
    # and with keys the call caches itself: the repeated bytes take one slot
    F = kc.committee(5, 240)
    r["dup_fresh"] = []
    seen = set()
    for n in (8, 100):
        d = kc.duplicate_key_list(kc.valid(F, n, 241 + n))
        before = e.keycache_stats()
        named = {d[0][k] for k in d[1]}
        checks.append(check(e, d, "msm", f"dup_list_fresh_{n}_valid"))
        checks.append(check(e, kc.forge_one(d, d[1].index(5)), "msm", f"dup_list_fresh_{n}_forged"))
        r["dup_fresh"].append({"before": before, "after": e.keycache_stats(), "indices_named": len(set(d[1])),
                               "new_distinct_keys": len(named - seen)})
        seen |= named
    close_forms(engs)
    return r


# ---- c: wrong signer and aliasing ---------------------------------------------------------------
def part_c():
    com = kc.committee(10, 300)
    engs = open_forms()
    for eng in engs.values():
        eng.keycache_register(com[1])
    r = {"stats": engs["default"].keycache_stats()}
    checks = r["checks"] = []
    for n in (8, 64, 65, 300):
        v = kc.valid(com, n, 310 + n)
        w = kc.wrong_signer(v, [0, n // 2, n - 1])
        a = v[1][0]
        s = kc.swapped_key_bytes(v, a, next(k for k in v[1] if k != a))
        for nm, case in (("valid", v), ("wrong_signer", w), ("swapped", s)):
            if n in (8, 300):
                check3(checks, engs, case, fast(n), f"{nm}_{n}")
            else:
                checks.append(check(engs["default"], case, fast(n), f"{nm}_{n}"))
    close_forms(engs)
    engs = open_forms()
    for pad in (0, 32):
        v = kc.one_byte_variants(320, pad)
        if pad == 0:
            for eng in engs.values():
                eng.keycache_register(v[0])
            r["variants_stats"] = engs["default"].keycache_stats()
        check3(checks, engs, v, fast(len(v[2])), f"one_byte_variants_{len(v[2])}")
    close_forms(engs)
    return r


# ---- d: the full slot table ---------------------------------------------------------------------
def part_d():
    import narwhal_amd
    e = narwhal_amd.Engine(device=0)
    C, T, F = kc.committee(8, 400), kc.committee(4, 402), kc.committee(8, 403)
    r = {"comb_keys": os.environ.get("NWV_COMB_KEYS")}
    checks = r["checks"] = []
    t0 = time.time()
    e.keycache_register(C[1])
    r["stats_C"] = st = e.keycache_stats()
    cap = st["cap"]
    rnd = random.Random(401)
    r["filler_calls"] = 0
    for _ in range(8):  # (four calls fill 65,521 slots; bounded either way)
        room = cap - 6 - e.keycache_stats()["used"]
        if room <= 0:
            break
        e.keycache_register([rnd.randbytes(32) for _ in range(min(20000, room))])
        r["filler_calls"] += 1
    r["stats_filled"] = e.keycache_stats()
    e.keycache_register(T[1])
    r["stats_T"] = e.keycache_stats()
    r["fill_seconds"] = round(time.time() - t0, 2)
    # T: cached MSM form at the top slot indices (no tables left for them)
    v = kc.valid(T, 40, 410)
    checks.append(check(e, v, "msm", "T_valid"))
    checks.append(check(e, kc.forged(v, 411, wrong=2), "msm", "T_forged"))
    r["stats_after_T"] = e.keycache_stats()

    def named(case, want_named):
        assert set(case[1]) >= set(want_named), "the case must name every fresh key"
        return case

    # C and three fresh keys: two slots are left, so nothing is published
    v = named(kc.valid(kc.joined(C, (F[0][:3], F[1][:3])), 40, 420), (8, 9, 10))
    before = e.keycache_stats()
    checks.append(check(e, v, "msm", "C_plus_three_fresh_valid"))
    checks.append(check(e, kc.forged(v, 421, wrong=2), "msm", "C_plus_three_fresh_forged"))
    r["three_fresh"] = {"before": before, "after": e.keycache_stats()}
    # C and two fresh keys: the table is full
    v = named(kc.valid(kc.joined(C, (F[0][3:5], F[1][3:5])), 40, 430), (8, 9))
    checks.append(check(e, v, "msm", "C_plus_two_fresh_valid"))
    checks.append(check(e, kc.forged(v, 431, wrong=2), "msm", "C_plus_two_fresh_forged"))
    r["stats_full"] = full = e.keycache_stats()
    v = named(kc.valid(kc.joined(C, (F[0][5:6], F[1][5:6])), 40, 440), (8,))
    checks.append(check(e, v, "msm", "full_one_more_fresh_valid"))
    checks.append(check(e, kc.forged(v, 441, wrong=2), "msm", "full_one_more_fresh_forged"))
    r["stats_after_one_more"] = e.keycache_stats()
    e.keycache_register(F[1][6:8])  # raises unless NWV_OK
    r["stats_after_register_when_full"] = e.keycache_stats()
    for n in (8, 100):
        v = kc.valid(C, n, 450 + n)
        checks.append(check(e, v, fast(n), f"full_C_{n}_valid"))
        checks.append(check(e, kc.forged(v, 460 + n, wrong=2), fast(n), f"full_C_{n}_forged"))
    # the two fresh keys that got the last slots, and T again, now that the table is full
    v = kc.valid(kc.joined(T, (F[0][3:5], F[1][3:5])), 40, 470)
    checks.append(check(e, v, "msm", "full_T_and_last_slots_valid"))
    checks.append(check(e, kc.forged(v, 471, wrong=2), "msm", "full_T_and_last_slots_forged"))
    r["single"] = [single(e, F[1][5], F[0][5], "fresh"), single(e, T[1][0], T[0][0], "T0"),
                   single(e, C[1][0], C[0][0], "C0"), single(e, F[1][4], F[0][4], "last_slot")]
    r["stats_end"] = e.keycache_stats()
    r["stats_end_equals_full"] = r["stats_end"] == full
    r["seconds"] = round(time.time() - t0, 2)
    e.close()
    return r


# ---- e: staged keyed batches across later registrations -----------------------------------------
def part_e():
    import narwhal_amd
    from narwhal_amd import _lib
    e = narwhal_amd.Engine(device=0)
    A, N = kc.committee(10, 500), kc.committee(20, 502)
    e.keycache_register(A[1])
    v = kc.valid(A, 300, 501)
    cases = {"valid": v, "forged": kc.forge_one(v, 137)}
    r = {"stage_chain": os.environ.get("NWV_STAGE_CHAIN"), "stats_before": e.keycache_stats()}
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
    rnd = random.Random(503)
    # (the signing keys first: the list is longer than the comb tables left, which go in list order)
    e.keycache_register(N[1] + [rnd.randbytes(32) for _ in range(4980)])
    r["stats_after"] = e.keycache_stats()
    run_all()
    run_all()
    r["runs"] = got  # per run: [batch verdict, bits == oracle's]
    r["want_all"] = {nm: all(c[4]) for nm, c in cases.items()}
    r["rejected"] = {nm: c[4].count(False) for nm, c in cases.items()}
    r["tally"] = {nm: list(st.run_tally()) for nm, st in staged.items()}
    for st in staged.values():
        st.free()
    # the keys registered meanwhile serve: a batch by the 20 new signing keys takes the comb
    w = kc.valid(N, 100, 504)
    r["checks"] = [check(e, w, "comb", "new_keys_valid"),
                   check(e, kc.forged(w, 505, wrong=2), "comb", "new_keys_forged"),
                   check(e, v, "comb", "A_unstaged_valid")]
    e.close()
    return r


# ---- f: registration beside verification --------------------------------------------------------
def part_f():
    import narwhal_amd
    e = narwhal_amd.Engine(device=0)
    A = kc.committee(10, 600)
    e.keycache_register(A[1])
    jobs = [kc.forged(kc.valid(A, n, 601 + n), 610 + n, wrong=2) for n in (8, 100)]
    more = [kc.committee(50, 620 + k)[1] for k in range(10)]
    out = [[], []]

    def work(t):
        keys, kidx, sigs, msgs, _ = jobs[t]
        for _ in range(20):
            out[t].append(e.verify_batch_keyed(keys, kidx, sigs, msgs))

    for keys, kidx, sigs, msgs, _ in jobs:  # (lanes and workspaces exist before the clock of the overlap starts)
        e.verify_batch_keyed(keys, kidx, sigs, msgs)
    c0 = e.diag_counters_ex()
    th = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(2)]
    for x in th:
        x.start()
    done_at = []
    for keys in more:
        e.keycache_register(keys)
        done_at.append(len(out[0]) + len(out[1]))
    for x in th:
        x.join(timeout=60)
    r = {"alive": [x.is_alive() for x in th], "calls": [len(o) for o in out],
         "bits_eq": [all(bits == jobs[t][4] for _, bits in out[t]) for t in range(2)],
         "ok_eq": [all(ok == all(jobs[t][4]) for ok, _ in out[t]) for t in range(2)],
         "rejected": [j[4].count(False) for j in jobs],
         "sets_differ": len({tuple(i for i, w in enumerate(j[4]) if not w) for j in jobs}) == 2,
         "calls_done_after_each_registration": done_at}  # (how far the two overlapped; not asserted)
    if not any(r["alive"]):
        r["runs"] = _delta(c0, e.diag_counters_ex())
        r["stats"] = e.keycache_stats()
        e.close()
    return r


# ---- g: k_ed_comb above 64 verdict words --------------------------------------------------------
def part_g():
    import narwhal_amd
    e = narwhal_amd.Engine(device=0)
    com = kc.committee(10, 700)
    e.keycache_register(com[1])
    e.set_comb_batch_max(8192)
    r = {"comb_batch_max": e.comb_batch_max}
    checks = r["checks"] = []
    for n in G_SIZES:  # (in this order: the workspace grows at 4,097 and serves 65 afterwards)
        v = gpu_signed(e, com, n, 710 + n)
        checks.append(check(e, v, "comb", f"g_{n}_valid"))
        f = kc.forged(v, 720 + n, extra=(4095, 4096))
        assert n <= 4096 or (not f[4][4095] and not f[4][4096])
        checks.append(check(e, f, "comb", f"g_{n}_forged"))
        # the last signature alone (at 4,097 the only one of word 64): a word the last wave does
        # not collect would accept the batch
        checks.append(check(e, kc.forge_one(v, n - 1), "comb", f"g_{n}_last_forged"))
    e.close()
    # the default limit, on a fresh context
    e = narwhal_amd.Engine(device=0)
    r["default_comb_batch_max"] = e.comb_batch_max
    r["shard_min_env"] = os.environ.get("NWV_SHARD_MIN")
    e.keycache_register(com[1])
    v = gpu_signed(e, com, 2049, 730)
    for n, path in ((2048, "comb"), (2049, "msm")):
        w = tuple(x[:n] for x in v)
        checks.append(check(e, w, path, f"default_limit_{n}_valid"))
        checks.append(check(e, kc.forge_one(w, n - 1), path, f"default_limit_{n}_forged"))
    e.close()
    return r


PARTS = {"a": part_a, "b": part_b, "c": part_c, "d": part_d, "e": part_e, "f": part_f, "g": part_g}


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
