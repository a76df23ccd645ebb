"""nwv_keycache_retain: the Ed25519 key cache at an epoch change (nwv_host.hip KeyCache over
keycache_alloc.h).  A retired key's slot and comb table serve later keys, and reusing an index is a
verification-key swap if anything still reads the old one: every case here must give the oracle's
verdict bits on the default context, on NWV_FLAG_NO_TINY (cached batch MSM) and on
NWV_FLAG_NO_KEYCACHE (uncached), with and without verdict bits, and nwv_keycache_stats /
nwv_diag_counters_ex must show the path aimed at -- the tables that came back, the reused slots,
the pins of staged batches, the fingerprint reset.  Batches are 8 signatures (k_ed_tiny) and 100
(k_ed_comb), committees 4 to 10 keys; the one full-table fill is test_gpu_keycache's.

The work runs in child processes (tests/keycache_retain_gpu_check.py, one JSON line each), one at a
time: the library reads NWV_COMB_KEYS and NWV_DEVICE_REPLICAS once per process."""
import json
import os
import subprocess
import sys

import pytest

from test_gpu_keycache import CAP, FORMS, _checks, _fast, _part, _stats, _three, _verdicts
from test_gpu_zcoeff import KNOBS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NOTHING = [0, 0, 0, 0]


def _child(parts, **env):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS + ("NWV_COMB_KEYS",)}
    e.update(env)
    p = subprocess.run([sys.executable, os.path.join(HERE, "keycache_retain_gpu_check.py"), "--parts", parts], env=e,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print("keycache_retain_gpu_check --parts", parts, env, {k: v["seconds"] for k, v in out.items()})
    return out


def _batches(name, path, sizes=(8, 100)):
    exp = {}
    for n in sizes:
        for kind in ("valid", "forged"):
            exp.update(_three(f"{name}_{n}_{kind}", _fast(n) if path == "fast" else path, n))
    return exp


def _default_only(exp):
    return {k: v for k, v in exp.items() if k[1] == "default"}


# ---- 1, 2: tables come back; a reused slot or table holds the new key ---------------------------
@pytest.fixture(scope="module")
def tables_out():
    return _part(_child("tables", NWV_COMB_KEYS="4"), "tables")


def test_tables_come_back(tables_out):
    """NWV_COMB_KEYS=4: A takes the four tables, B gets slots only and runs on the MSM (today's
    behaviour); retain(B) retires A's four slots and four tables, and registering B again gives B
    the tables: its batches take tiny / comb"""
    r = tables_out
    assert r["comb_keys"] == "4"
    assert r["stats_A"] == [_stats(5, 4, 4)] * 2
    assert r["stats_AB"] == [_stats(9, 4, 4)] * 2
    assert r["retain_B"] == [[4, 4, 0, 5], [4, 4, 0, 5], NOTHING]
    assert r["stats_retained"] == [_stats(5, 0, 4)] * 2
    assert r["stats_B"] == [_stats(5, 4, 4)] * 2  # five live slots and none new, A's tables reused
    exp = _batches("B_before", "msm")
    exp.update(_batches("B_after", "fast"))
    exp.update(_three("crossed_100_forged", "comb", 100))
    exp.update(_batches("A_again", "msm"))
    _checks(r, exp)


def test_a_reused_slot_or_table_holds_the_new_key(tables_out):
    """after the retain every table of B was one of A's, and A's old slots are free: a signature by
    A_k named under B_j, for all sixteen (j, k), is rejected at exactly the oracle's indices on
    the tiny, comb and cached-MSM paths; A's own batches then verify on the MSM path, in fresh
    slots and without tables"""
    r = tables_out
    assert [(c["name"], c["form"]) for c in r["crossed8"]] == [(f"crossed8_{h}", f) for h in (0, 1) for f in FORMS]
    for c in r["crossed8"]:
        assert c["n"] == 8 and c["rejected"] == 8 and c["path"] == ("tiny" if c["form"] == "default" else "msm")
        _verdicts(c)
    by = {(c["name"], c["form"]): c for c in r["checks"]}
    for f in FORMS:
        assert by["crossed_100_forged", f]["rejected"] == 16
    assert r["stats_before_A_again"] == [_stats(5, 4, 4)] * 2
    assert r["stats_end"] == [_stats(9, 4, 4)] * 2
    assert r["stats_no_keycache"] == _stats(0, 0, 0, cap=0)


# ---- 3, 4, 5, 6, 9: the default environment -----------------------------------------------------
@pytest.fixture(scope="module")
def main_out():
    return _child("overlap,fp,staged,threads")


def test_overlapping_committees_keep_the_shared_members(main_out):
    """A is 10 keys, B shares three and adds seven: retain(B) retires seven slots and seven tables,
    the three shared keys keep tiny / comb before and after B is registered"""
    r = _part(main_out, "overlap")
    assert r["stats_A"] == [_stats(11, 10)] * 2
    assert r["retain_B"] == [[7, 7, 0, 4], [7, 7, 0, 4], NOTHING]
    assert r["stats_retained"] == r["stats_before_register"] == [_stats(4, 3)] * 2
    assert r["stats_B"] == [_stats(11, 10)] * 2
    assert r["retain_B_again"] == [[0, 0, 0, 11], [0, 0, 0, 11], NOTHING]
    exp = _batches("shared_before", "fast")
    exp.update(_batches("shared_after", "fast"))
    exp.update(_batches("B", "fast"))
    _checks(r, exp)


def test_the_fingerprint_is_reset(main_out):
    """register A, retain nothing-kept, register A: the second registration does the work
    (comb_used is back at len(A), A's batches take tiny / comb); names that are not cached are
    ignored, and a retain before the cache exists reports nothing"""
    r = _part(main_out, "fp")
    assert r["retain_before_anything"] == [NOTHING] * 3
    assert r["stats_A"] == r["stats_kept"] == [_stats(11, 10)] * 2
    assert r["retain_A_and_strangers"] == [[0, 0, 0, 11], [0, 0, 0, 11], NOTHING]
    assert r["retain_none"] == [[10, 10, 0, 1], [10, 10, 0, 1], NOTHING]
    assert r["stats_retained"] == [_stats(1, 0)] * 2
    assert r["stats_A_again"] == [_stats(11, 10)] * 2
    _checks(r, _batches("A_again", "fast"))


def test_no_keycache_context(main_out):
    """NWV_FLAG_NO_KEYCACHE: retain returns NWV_OK with out all zero"""
    r = _part(main_out, "fp")["no_keycache"]
    assert r == {"retain_list": NOTHING, "retain_none": NOTHING, "stats": _stats(0, 0, 0, cap=0)}


def _staged(r, chain):
    assert r["stage_chain"] == chain
    assert r["stats_before"] == _stats(11, 10) and r["distinct_staged"] == 6
    # the six staged keys are kept only because they are pinned, with their tables
    assert r["retain_none"] == [4, 4, 6, 7]
    assert r["stats_retained"] == _stats(7, 6)
    assert r["stats_N"] == _stats(17, 16)
    assert r["want_all"] == {"valid": True, "forged": False} and r["rejected"] == {"valid": 0, "forged": 1}
    # the run before the retain and the two replays after it: [batch verdict, bits == oracle's]
    assert r["runs"] == {"valid": [[True, True]] * 3, "forged": [[False, True]] * 3}
    assert r["tally"] == {"valid": [3, 0], "forged": [0, 3]}
    _checks(r, {("new_keys_valid", "default"): ("comb", 100), ("new_keys_forged", "default"): ("comb", 100),
                ("A_pinned_unstaged_valid", "default"): ("comb", 100)})
    assert r["retain_one_freed"] == [0, 0, 6, 17]  # the other batch still pins them
    assert r["retain_both_freed"] == [6, 6, 0, 11]
    assert r["retain_none_at_end"] == [10, 10, 0, 1]
    assert r["stats_end"] == _stats(1, 0)


def test_staged_keyed_batch_pins_its_slots(main_out):
    """two staged 100-signature keyed batches over six of A's keys run once; retain(empty) keeps
    exactly their six slots, a fresh committee takes the freed slots and tables, and the replays
    give the same verdict, bits and run tally; freed batches let the next retain retire the keys"""
    _staged(_part(main_out, "staged"), None)


def test_staged_keyed_batch_pins_its_slots_graph_replay():
    _staged(_part(_child("staged", NWV_STAGE_CHAIN="0"), "staged"), "0")


def test_keyed_calls_beside_retain_and_register(main_out):
    """two threads, 20 keyed calls each (8 and 100 signatures, different forged sets, keys of both
    committees), while the main thread runs retain(A), register(A), retain(B), register(B) ten
    times: bits == oracle's on every call (the path varies legitimately), everything finishes"""
    r = _part(main_out, "threads")
    assert r["alive"] == [False, False]
    assert r["calls"] == [20, 20] and r["main_rounds"] == 10
    assert r["both_committees_named"] == [True, True]
    assert r["sets_differ"] and min(r["rejected"]) > 0
    assert r["bits_eq"] == [True, True] and r["ok_eq"] == [True, True]
    assert r["pinned_kept"] == [0]
    assert r["retain_B_at_end"][1:] == [0, 0, 11] and r["stats_end"] == _stats(11, 10)
    _checks(r, {("B_at_end_valid", "default"): ("comb", 100), ("B_at_end_forged", "default"): ("comb", 100)})


# ---- 7: the full slot table recovers ------------------------------------------------------------
def test_full_table_recovers():
    """NWV_COMB_KEYS=8: C takes slots 1..8 and every table, filler keys fill the slot table (the
    fill of test_full_slot_table, 0.27 s there).  A call that names two fresh keys runs uncached;
    retain(C) leaves (9, 8); the same call now takes two slots, and C still takes tiny / comb"""
    r = _part(_child("full", NWV_COMB_KEYS="8"), "full")
    print("fill %.2f s, retain of %d keys %.3f s" % (r["fill_seconds"], CAP - 9, r["retain_seconds"]))
    assert r["comb_keys"] == "8" and r["filler_calls"] == 4
    assert r["stats_full"] == r["stats_after_fresh_when_full"] == _stats(CAP, 8, 8)
    assert r["retain_C"] == [CAP - 9, 0, 0, 9]
    assert r["stats_retained"] == _stats(9, 8, 8)
    assert r["stats_after_fresh"] == _stats(11, 8, 8)
    exp = {}
    for nm in ("fresh_when_full", "fresh_after_retain"):
        exp[f"{nm}_valid", "default"] = exp[f"{nm}_forged", "default"] = ("msm", 40)
    exp.update(_default_only(_batches("C", "fast")))
    _checks(r, exp)


# ---- 8: every device object ---------------------------------------------------------------------
def test_every_device_object_is_retained():
    """NWV_DEVICE_REPLICAS=3: the stats of the three device objects agree after a retain, and out is
    three times the one-device values"""
    r = _part(_child("replicas", NWV_DEVICE_REPLICAS="3"), "replicas")
    assert r["replicas"] == "3" and r["devices"] == 3
    assert r["stats_A"] == [_stats(11, 10)] * 3
    assert r["retain"] == [3 * x for x in (6, 6, 0, 5)]
    assert r["stats_retained"] == [_stats(5, 4)] * 3
    _checks(r, _default_only(_batches("kept", "fast")))
    assert r["retain_none"] == [3 * x for x in (4, 4, 0, 1)]
    assert r["stats_end"] == [_stats(1, 0)] * 3
