"""The committee key cache and the per-key comb tables at their capacity, epoch and alias edges
(nwv_host.hip KeyCache, keycache_slots, nwv_keycache_register, ed_stage_keyed; consumed by
k_keycache_fill, k_key_comb_fill, k_ed_tiny, k_ed_comb and the cached form of k_msm_prep).
include/nwv.h promises "A full cache leaves further keys uncached; verdicts never depend on the
cache": every case here must give the oracle's verdict bits on the default context, on
NWV_FLAG_NO_TINY (cached batch MSM) and on NWV_FLAG_NO_KEYCACHE (uncached), with and without
verdict bits, and nwv_keycache_stats / nwv_diag_counters_ex must show that the branch aimed at ran:
the comb-table `break`, the full-slot-table return, the fingerprint fast path, the `dup` branch,
the multi-pass verdict-word loop of k_ed_comb.  A slot or a table shared by two keys would accept
a signature made by X and presented as Y: the wrong-signer, swapped-bytes and one-byte-variant
cases (tests/keycache_cases.py) are rejected exactly where the oracle rejects them.

The work runs in child processes (tests/keycache_gpu_check.py, one JSON line each), one at a
time: the library reads NWV_COMB_KEYS once per process."""
import json
import os
import subprocess
import sys

import pytest

import keycache_gpu_check as kg
from test_gpu_zcoeff import KNOBS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FORMS = ("default", "no_tiny", "no_keycache")
ZERO = {"tiny": 0, "msm": 0, "each": 0, "comb": 0}
CAP = 1 << 16


def _child(parts, **env):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS + ("NWV_COMB_KEYS",)}
    e.update(env)
    p = subprocess.run([sys.executable, os.path.join(HERE, "keycache_gpu_check.py"), "--parts", parts], env=e,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print("keycache_gpu_check --parts", parts, env, {k: v["seconds"] for k, v in out.items()})
    return out


def _part(out, key):
    r = out[key]
    assert "error" not in r, r["error"]
    return r


def _ran(runs, path):
    """one call's counter delta: exactly one launch of the path; an MSM call may add the
    per-signature pass that names a rejected batch's bad signatures, and nothing else"""
    if path == "msm":
        assert runs["msm"] == 1 and runs["tiny"] == 0 and runs["comb"] == 0 and runs["each"] in (0, 1), runs
    else:
        assert runs == dict(ZERO, **{path: 1}), runs


def _verdicts(c):
    assert c["bits_eq"], c  # want_bits=True: bits == oracle's
    assert c["ok_bits"] and c["ok_nobits"], c  # both batch verdicts == all(oracle's)
    _ran(c["runs_bits"], c["path"])
    _ran(c["runs_nobits"], c["path"])
    if c["rejected"] == 0 or c["path"] != "msm":
        assert c["runs_bits"]["each"] == 0 and c["runs_nobits"]["each"] == 0, c


def _checks(r, expect):
    """every check of the part is right, and the part ran exactly the checks `expect`:
    {(name, form): (path, n)}; forged ones reject something, valid ones nothing"""
    got = {(c["name"], c["form"]): (c["path"], c["n"]) for c in r["checks"]}
    assert len(got) == len(r["checks"])
    assert got == expect
    for c in r["checks"]:
        _verdicts(c)
        assert (c["rejected"] == 0) == (c["name"].endswith("valid") or c["name"].startswith("valid_")), c
        assert c["rejected"] < c["n"]


def _three(name, path, n):
    return {(name, f): (path if f == "default" else "msm", n) for f in FORMS}


def _fast(n):
    return "tiny" if n <= 64 else "comb"


def _stats(used, comb_used, comb_cap=1024, cap=CAP):
    return {"used": used, "cap": cap, "comb_used": comb_used, "comb_cap": comb_cap}


# ---- a: comb-table capacity ---------------------------------------------------------------------
def _expect_a(tables):
    exp = {}
    for n in (8, 100):
        for kind in ("valid", "forged"):
            exp.update(_three(f"pure_{n}_{kind}", _fast(n) if tables else "msm", n))
            for x in (4, 5):
                exp.update(_three(f"mixed{x}_{n}_{kind}", "msm", n))
    return exp


def _singles(r, names, tiny):
    assert [s["name"] for s in r["single"]] == names
    for s in r["single"]:
        assert s["rc"] == s["want"] and s["want_is_ok_then_reject"], s
        if s["name"] in tiny:
            assert s["runs"] == dict(ZERO, tiny=2), s
        else:
            assert s["runs"]["tiny"] == 0 and s["runs"]["comb"] == 0 and s["runs"]["msm"] == 2, s


def test_comb_table_capacity():
    """NWV_COMB_KEYS=4, six keys registered in one call: keys 0..3 get the tables (the `break` at
    "full: later keys take the MSM path"), batches naming only them take tiny / comb, one signature
    by key 4 or 5 sends the call to the MSM, and a wrong signer between a key with a table and one
    without is rejected either way round"""
    r = _part(_child("a", NWV_COMB_KEYS="4"), "a")
    assert r["comb_keys"] == "4"
    assert r["stats"] == r["stats_no_tiny"] == _stats(7, 4, 4)
    assert r["stats_no_keycache"] == _stats(0, 0, 0, cap=0)
    _checks(r, _expect_a(True))
    assert r["stats_same_list_again"] == r["stats_k4_k5_alone"] == r["stats_end"] == r["stats"]
    _singles(r, ["key0", "key5", "unregistered"], tiny={"key0"})


def test_comb_tables_off():
    """NWV_COMB_KEYS=0: registration still fills the slots, no table exists, every keyed call is an MSM"""
    r = _part(_child("a", NWV_COMB_KEYS="0"), "a")
    assert r["comb_keys"] == "0"
    assert r["stats"] == r["stats_no_tiny"] == _stats(7, 0, 0)
    _checks(r, _expect_a(False))
    assert r["stats_same_list_again"] == r["stats_k4_k5_alone"] == r["stats_end"] == r["stats"]
    _singles(r, ["key0", "key5", "unregistered"], tiny=set())


# ---- b, c, e, f, g: the default environment -----------------------------------------------------
@pytest.fixture(scope="module")
def main_out():
    return _child("b,c,e,f,g")


def test_epoch_change_and_duplicates(main_out):
    """register A, B (three members shared), A, A: slots and tables are append-only and found
    again; a batch over keys not yet registered takes the MSM, over registered ones tiny / comb; the
    same bytes twice in a registered list or at two indices of a call's key list take one slot"""
    r = _part(main_out, "b")
    assert [s["registered"] for s in r["steps"]] == ["A", "B", "A", "A"]
    assert [s["stats"] for s in r["steps"]] == [_stats(11, 10), _stats(18, 17), _stats(18, 17), _stats(18, 17)]
    assert [s["stats_no_tiny"] for s in r["steps"]] == [s["stats"] for s in r["steps"]]
    # (the step-0 batches over B cached its seven new keys themselves: slots, no tables)
    assert [s["stats_after_batches"] for s in r["steps"]] == [_stats(18, 10)] + [_stats(18, 17)] * 3
    exp = {}
    for k in range(4):
        for cn in "ABU":
            for n in (8, 100):
                for kind in ("valid", "forged"):
                    exp.update(_three(f"step{k}_{cn}_{n}_{kind}", _fast(n) if k or cn == "A" else "msm", n))
    exp.update(_three("dup_registered_key_valid", "tiny", 8))
    exp.update(_three("dup_registered_key_forged", "tiny", 8))
    names = {c["name"] for c in r["checks"]}
    for n in (8, 100):
        exp.update(_three(f"dup_list_{n}_valid", _fast(n), n))
        under = sorted(x for x in names if x.startswith(f"dup_list_{n}_forged_under_"))
        assert len(under) == 2 and under[0].endswith("_under_10") != under[1].endswith("_under_10")
        for x in under:
            exp.update(_three(x, _fast(n), n))
        exp[f"dup_list_fresh_{n}_valid", "default"] = exp[f"dup_list_fresh_{n}_forged", "default"] = ("msm", n)
    _checks(r, exp)
    assert r["dup_register"] == {"before": _stats(18, 17), "after": _stats(19, 18)}
    # five fresh keys under six indices: one slot per distinct key, no table
    d8, d100 = r["dup_fresh"]
    assert d8["before"] == _stats(19, 18) and d8["indices_named"] == d8["new_distinct_keys"] + 1
    assert d8["after"] == d100["before"] == _stats(19 + d8["new_distinct_keys"], 18)
    assert d100["indices_named"] == 6 and d100["after"] == _stats(24, 18)


def test_wrong_signer_and_aliasing(main_out):
    """a signature named under another key of the list, two exchanged key-list entries, and a key
    registered beside its 33 one-bit neighbours: bits == oracle's on every form"""
    r = _part(main_out, "c")
    assert r["stats"] == _stats(11, 10)
    assert r["variants_stats"] == _stats(35, 34)
    exp = {}
    for n in (8, 64, 65, 300):
        for nm in ("valid", "wrong_signer", "swapped"):
            if n in (8, 300):
                exp.update(_three(f"{nm}_{n}", _fast(n), n))
            else:
                exp[f"{nm}_{n}", "default"] = (_fast(n), n)
    exp.update(_three("one_byte_variants_38", "tiny", 38))
    exp.update(_three("one_byte_variants_70", "comb", 70))
    _checks(r, exp)
    by = {(c["name"], c["form"]): c for c in r["checks"]}
    for f in FORMS:
        assert by["one_byte_variants_38", f]["rejected"] == by["one_byte_variants_70", f]["rejected"] == 33
        assert by["wrong_signer_300", f]["rejected"] == 3


def _staged(r, chain):
    assert r["stage_chain"] == chain
    assert r["stats_before"] == _stats(11, 10)
    assert r["stats_after"] == _stats(11 + 5000, 1024)  # (the tables left went to the list's first keys)
    assert r["want_all"] == {"valid": True, "forged": False} and r["rejected"] == {"valid": 0, "forged": 1}
    # the run before the registration and the two replays after it: [batch verdict, bits == oracle's]
    assert r["runs"] == {"valid": [[True, True]] * 3, "forged": [[False, True]] * 3}
    assert r["tally"] == {"valid": [3, 0], "forged": [0, 3]}
    _checks(r, {("new_keys_valid", "default"): ("comb", 100), ("new_keys_forged", "default"): ("comb", 100),
                ("A_unstaged_valid", "default"): ("comb", 300)})


def test_staged_keyed_batch_across_registrations(main_out):
    """"a slot in use by an in-flight or captured batch is never rewritten": two staged 300-signature
    keyed batches run once, 5,000 keys are registered, and the replays give the same verdicts"""
    _staged(_part(main_out, "e"), None)


def test_staged_keyed_batch_across_registrations_graph_replay():
    _staged(_part(_child("e", NWV_STAGE_CHAIN="0"), "e"), "0")


def test_registration_beside_verification(main_out):
    """two threads, 20 calls each (8 and 100 signatures, different forged sets), while the main
    thread registers ten committees of 50 keys on the same context"""
    r = _part(main_out, "f")
    assert r["alive"] == [False, False]
    assert r["calls"] == [20, 20]
    assert r["sets_differ"] and min(r["rejected"]) > 0
    assert r["bits_eq"] == [True, True] and r["ok_eq"] == [True, True]
    assert r["stats"] == _stats(1 + 10 + 500, 510)
    assert r["runs"] == dict(ZERO, tiny=20, comb=20)


def test_comb_above_64_verdict_words_and_default_limit(main_out):
    """k_ed_comb's last wave collects ceil(n / 64) verdict words 64 at a time: 4,097 and 4,160
    signatures need a second pass (words 64 and 65, signatures 4,095 / 4,096 forged); the calls
    before and after them are smaller, so the workspace grows once and then serves fewer words.
    Each size also runs with its last signature alone forged: at 4,097 that is the only signature
    of word 64, so a word left uncollected would accept the batch (the forged set above is rejected
    for its other indices whatever word 64 says).  A fresh context sends 2,048 registered-key signatures to the comb kernel and 2,049 to the MSM."""
    r = _part(main_out, "g")
    assert kg.G_SIZES == [300, 4097, 65, 4160, 129]
    assert r["comb_batch_max"] == 8192
    assert r["shard_min_env"] is None and r["default_comb_batch_max"] == 2048
    exp = {}
    kinds = ("valid", "forged", "last_forged")
    for n in kg.G_SIZES:
        for k in kinds:
            exp[f"g_{n}_{k}", "default"] = ("comb", n)
    for n, path in ((2048, "comb"), (2049, "msm")):
        exp[f"default_limit_{n}_valid", "default"] = exp[f"default_limit_{n}_forged", "default"] = (path, n)
    _checks(r, exp)
    assert [c["name"] for c in r["checks"]][:15] == [f"g_{n}_{k}" for n in kg.G_SIZES for k in kinds]
    by = {c["name"]: c for c in r["checks"]}
    assert all(by[f"g_{n}_last_forged"]["rejected"] == 1 for n in kg.G_SIZES)


# ---- d: the full slot table ---------------------------------------------------------------------
def test_full_slot_table():
    """NWV_COMB_KEYS=8: committee C takes slots 1..8 and every table, filler keys fill the table to
    six below its capacity, four signing keys T take the next four slots.  A call that needs three
    new slots publishes nothing, one that needs two fills the table, and from then on fresh keys
    run uncached while C keeps tiny / comb and T the cached MSM at the top slot indices.

    Measured on the MI355X: the part takes 0.27 s in the child, 0.08 s of it to fill the 65,533
    slots, and the test 0.7 s with the child's start -- what one child of test_gpu_zcoeff takes
    (0.5 s a forms child, 1.4 s the main one), so the fill stays in the same child as the checks."""
    r = _part(_child("d", NWV_COMB_KEYS="8"), "d")
    assert r["comb_keys"] == "8"
    assert r["stats_C"] == _stats(9, 8, 8)
    assert r["filler_calls"] == 4  # 20,000 + 20,000 + 20,000 + 5,521: several 4,096-key chunks a call
    assert r["stats_filled"] == _stats(CAP - 6, 8, 8)
    assert r["stats_T"] == r["stats_after_T"] == _stats(CAP - 2, 8, 8)
    assert r["three_fresh"]["before"] == r["three_fresh"]["after"] == _stats(CAP - 2, 8, 8)
    assert r["stats_full"] == _stats(CAP, 8, 8)
    assert r["stats_after_one_more"] == r["stats_after_register_when_full"] == r["stats_end"] == r["stats_full"]
    exp = {}
    for nm in ("T", "C_plus_three_fresh", "C_plus_two_fresh", "full_one_more_fresh", "full_T_and_last_slots"):
        exp[f"{nm}_valid", "default"] = exp[f"{nm}_forged", "default"] = ("msm", 40)
    for n in (8, 100):
        exp[f"full_C_{n}_valid", "default"] = exp[f"full_C_{n}_forged", "default"] = (_fast(n), n)
    _checks(r, exp)
    _singles(r, ["fresh", "T0", "C0", "last_slot"], tiny={"C0"})
