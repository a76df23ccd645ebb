"""The BLS aggregate-key ring on the GPU (nwv_bls_set_apk_ring): a device keeps, per recurring
signer set, the affine sum of the signers' [h_eff] pk records and its Miller-loop line table, so a
certificate by a set seen before verifies as a one-key item by a registered key.  The scenarios run
in child processes (tests/bls_apk_ring_gpu_check.py): one child runs every scenario that needs only
a context of its own, each on a fresh engine; NWV_BLS_DEVICE_REPLICAS=2 has a child to itself.
Statuses are always compared with the oracle's; what the ring did in a call is read from
nwv_bls_last_apk as (hits, missed, noted, published) and nwv_bls_apk_ring_stats as (held, busy,
pinned).  Every case is a handful of one-item calls over a 4-key committee, but for one 67-of-100
set."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, VERIFY_FAIL, PK_INFINITY = 0, 5, 6
WAVE = 3                                    # nwv_bls_last_path of a small wave call
NOTED, FILLED, HIT, UNUSED = [0, 1, 1, 0], [0, 1, 0, 1], [1, 0, 0, 0], [0, 0, 0, 0]
SCENARIOS = ["default_off", "noted_filled_hit", "held_set", "gate", "identity", "eviction", "epoch", "real_size",
             "with_msg_ring", "types", "threads", "ignored:batch", "ignored:per_item", "ignored:no_keycache",
             "ignored:unregistered", "ignored:n1025", "many_keys"]


def _child(names, **env):
    e = dict(os.environ, NWV_BLS_DEVICE_REPLICAS="1")
    for k in ("NWV_BLS_WAVE_MAX", "NWV_DEVICE_REPLICAS"):
        e.pop(k, None)
    e.update(env)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bls_apk_ring_gpu_check.py")] + list(names),
                       env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def runs():
    return _child(SCENARIOS)


def _of(runs, name):
    assert name in runs, "the child stopped before this scenario: %s" % {k: v for k, v in runs.items() if "error" in v}
    assert "error" not in runs[name], runs[name]["error"]
    return runs[name]


def _same(run):
    assert run["got"] == run["want"], run
    return run["apk"]


def _warmed(three):
    """a set brought to a hit: noted, filled, hit, OK each time, on the small wave path"""
    assert [_same(x) for x in three] == [NOTED, FILLED, HIT], three
    assert all(x["got"] == [OK] and x["path"] == WAVE for x in three)


def test_off_by_default(runs):
    out = _of(runs, "default_off")
    assert out["size_fresh"] == 0 and out["size_after"] == 0
    for x in out["runs"]:
        assert _same(x) == UNUSED and x["got"] == [OK] and x["stats"] == [0, 0, 0]
    assert out["size_on"] == 8 and out["resize_refused"] and out["too_large_refused"]
    _warmed(out["on"])
    assert out["size_off_again"] == 0
    assert _same(out["off_again"]) == UNUSED and out["off_again"]["got"] == [OK]
    assert _same(out["on_again"]) == HIT, "a later 0 switches the ring off without freeing it"


def test_noted_filled_hit(runs):
    out = _of(runs, "noted_filled_hit")
    _warmed(out["runs"])
    assert [x["stats"] for x in out["runs"]] == [[0, 0, 0], [1, 0, 0], [1, 0, 0]]


def test_on_a_held_set(runs):
    out = _of(runs, "held_set")
    _warmed(out["warm"])
    assert _same(out["forged"]) == HIT and out["forged"]["got"] == [VERIFY_FAIL]
    assert _same(out["wrong_message"]) == HIT and out["wrong_message"]["got"] == [VERIFY_FAIL]
    # one key fewer and one key more are other sets: never served from the held one
    assert _same(out["key_dropped"]) == NOTED and out["key_dropped"]["got"] == [VERIFY_FAIL]
    assert _same(out["key_dropped_valid"])[0] == 0 and out["key_dropped_valid"]["got"] == [OK]
    assert _same(out["key_added"]) == NOTED and out["key_added"]["got"] == [VERIFY_FAIL]
    assert _same(out["key_added_valid"])[0] == 0 and out["key_added_valid"]["got"] == [OK]
    assert _same(out["permuted"]) == HIT and out["permuted"]["got"] == [OK]
    # [a, b] is held by now ([0, 1] was filled above and warmed again): [a, a, b] is another set
    assert _same(out["warm_ab"][-1]) == HIT
    assert _same(out["aab_with_ab_aggregate"])[0] == 0 and out["aab_with_ab_aggregate"]["got"] == [VERIFY_FAIL]
    assert _same(out["aab_valid"])[0] == 0 and out["aab_valid"]["got"] == [OK]
    assert _same(out["ab_with_aab_aggregate"]) == HIT and out["ab_with_aab_aggregate"]["got"] == [VERIFY_FAIL]
    assert _same(out["ab_valid"]) == HIT and out["ab_valid"]["got"] == [OK]


def test_the_gate(runs):
    """a valid set with a forged aggregate, five times: noted, then reserved, filled and released
    every time; nothing is ever held"""
    out = _of(runs, "gate")
    assert [_same(x) for x in out["runs"]] == [NOTED] + [[0, 1, 0, 0]] * 4
    for x in out["runs"]:
        assert x["got"] == [VERIFY_FAIL] and x["stats"] == [0, 0, 0]
    assert _same(out["then_valid"]) == FILLED and out["then_valid"]["stats"] == [1, 0, 0]


def test_an_identity_sum(runs):
    out = _of(runs, "identity")
    assert [_same(x) for x in out["runs"]] == [NOTED] + [[0, 1, 0, 0]] * 3
    for x in out["runs"]:
        assert x["got"] == [PK_INFINITY] and x["stats"] == [0, 0, 0]


def test_eviction(runs):
    out = _of(runs, "eviction")
    for k in "ABC":
        _warmed(out["warm"][k])
        assert all(x["stats"][0] <= 2 and x["stats"][1:] == [0, 0] for x in out["warm"][k])
    after = out["after"]
    assert _same(after["C"]) == HIT and _same(after["B"]) == HIT, "the newest two hit"
    # the oldest was pushed out (filled again at once if the 8-entry filter still has its hash,
    # noted again if another set's took the entry)
    assert _same(after["A"]) in (FILLED, NOTED)
    for k in "ABC":
        assert after[k]["got"] == [OK] and after[k]["stats"] == [2, 0, 0]


def test_epoch(runs):
    out = _of(runs, "epoch")
    _warmed(out["warm"])
    assert out["stats_after_reset"] == [0, 0, 0]
    # {k3, k2, k1} now has the index list {k0, k1, k2} had: a stale entry would swap the keys
    assert _same(out["k3k2k1"]) == NOTED and out["k3k2k1"]["got"] == [OK]
    assert _same(out["k0k1k2"]) == NOTED and out["k0k1k2"]["got"] == [OK]
    assert _same(out["swapped"])[0] == 0 and out["swapped"]["got"] == [VERIFY_FAIL]


def test_the_real_size(runs):
    out = _of(runs, "real_size")
    _warmed(out["warm"])
    assert _same(out["valid"]) == HIT and out["valid"]["got"] == [OK]
    assert _same(out["forged"]) == HIT and out["forged"]["got"] == [VERIFY_FAIL]


def test_with_the_message_ring_on_too(runs):
    out = _of(runs, "with_msg_ring")
    _warmed(out["runs"])
    assert out["runs"][2]["msgs"]["hits_copied"] == 1, "the third call hits on both rings"
    assert _same(out["forged"]) == HIT and out["forged"]["got"] == [VERIFY_FAIL]
    assert out["forged"]["msgs"]["hits_copied"] == 1


def test_the_types_layer(runs):
    out = _of(runs, "types")
    assert out["q"] == 3 and sorted(map(tuple, out["signed"])) == [(0, 1, 2)] * 3 + [(1, 2, 3)] * 3
    hc, vc, cc = out["want"]
    assert hc == [0] * 4 and vc == [0] * 6 and [c != 0 for c in cc] == [False] * 4 + [True, False]
    for call in out["calls"]:
        assert call["got"] == out["want"], call
        assert call["validate"] == [False, [4]], "the invalid set exactly"
        assert call["apk"][0] + call["apk"][1] == 6 == call["validate_apk"][0] + call["validate_apk"][1]
    assert out["calls"][2]["apk"] == [6, 0, 0, 0] and out["calls"][2]["validate_apk"] == [6, 0, 0, 0]
    assert out["stats"] == [2, 0, 0]


def test_four_threads_on_a_ring_of_two(runs):
    out = _of(runs, "threads")
    assert out["errors"] == [] and out["bad"] == [], out
    assert out["calls"] == [20] * 4
    assert out["statuses_seen"] == [OK, VERIFY_FAIL]
    held, busy, pinned = out["stats"]
    assert busy == 0 and pinned == 0 and held <= 2


def test_two_device_objects():
    out = _child(["replicas"], NWV_BLS_DEVICE_REPLICAS="2", NWV_DEVICE_REPLICAS="2")
    out = out["replicas"]
    assert "error" not in out, out.get("error")
    assert out["devices"] == 2 and out["staged_ok"]
    assert all(sorted(p) == [0, 1] for p in out["placed"]), out["placed"]
    seen = {0: [], 1: []}
    for p, x in zip(out["placed"], out["runs"]):
        assert x["got"] == [OK]
        seen[p.index(1)].append(_same(x))
    assert len(seen[0]) >= 3 and len(seen[1]) >= 3, "both device objects served calls: %s" % out["placed"]
    for d in (0, 1):    # each device's ring fills on its own sightings, whichever calls it was sent
        assert seen[d] == ([NOTED, FILLED] + [HIT] * len(seen[d]))[:len(seen[d])], (d, seen[d])


def test_more_uncached_keys_than_the_cache_has_slots(runs):
    """66,005 keys in one call's table: scratch indices beyond 2 x 65,536 are scratch entries, not
    ring slots"""
    out = _of(runs, "many_keys")
    _warmed(out["warm"])
    assert out["n_keys"] > 65536 + 4
    assert _same(out["run"]) == [2, 0, 0, 0]
    assert out["run"]["got"][0] == OK and out["run"]["got"][1] == OK and out["run"]["got"][3] == VERIFY_FAIL
    assert out["run"]["got"][2] not in (OK, VERIFY_FAIL), "an undecodable key's own status"


@pytest.mark.parametrize("what", ["batch", "per_item", "no_keycache", "unregistered"])
def test_paths_that_ignore_the_ring(runs, what):
    out = _of(runs, "ignored:" + what)
    assert out["size"] == 8
    for x in out["runs"]:
        assert _same(x) == UNUSED and x["got"] == [OK] and x["stats"] == [0, 0, 0]
    if what in ("batch", "per_item"):
        assert all(x["path"] != WAVE for x in out["runs"])


def test_a_call_of_1025_items_ignores_the_ring(runs):
    out = _of(runs, "ignored:n1025")
    assert out["size"] == 8
    for x in out["runs"]:
        assert x["got"] == x["want"] == [OK, VERIFY_FAIL]
        assert x["apk"] == UNUSED and x["stats"] == [0, 0, 0]
