"""The BLS message ring on the GPU (nwv_bls_set_msg_ring, nwv_bls_hash_ahead,
nwv_bls_verify_many_ahead): a device keeps the raw hashed point of every message a small call
verified over, so a message that recurs is not hashed again, and a message known ahead of its
signature is hashed before the call that needs it.  Every configuration runs in a fresh child
(tests/bls_msg_ring_gpu_check.py).  Statuses are always compared with the oracle's; what the ring
did in a call is read from nwv_bls_last_msgs (copied hits, chain hits, computed, published, ahead
published).  Every case is a handful of items."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, VERIFY_FAIL = 0, 5
ZERO = {"hits_copied": 0, "hits_chained": 0, "computed": 0, "published": 0, "ahead_published": 0}


def cnt(**kw):
    return dict(ZERO, **kw)


def _child(scenario, arg="", **env):
    e = dict(os.environ, NWV_BLS_DEVICE_REPLICAS="1")
    for k in ("NWV_BLS_WAVE_MAX", "NWV_DEVICE_REPLICAS"):
        e.pop(k, None)
    e.update(env)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bls_msg_ring_gpu_check.py"), scenario, arg],
                       env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _same(run):
    assert run["got"] == run["want"], run
    return run["msgs"]


def test_off_by_default():
    out = _child("default_off")
    assert out["size_fresh"] == 0 and out["size_after"] == 0
    assert _same(out["verify"]) == ZERO and out["verify"]["got"] == [OK]
    assert _same(out["after_hash_ahead"]) == ZERO, "hash_ahead with the ring off changes nothing"
    assert out["stats"] == [0, 0, 0]
    assert out["size_on"] == 16 and out["resize_refused"] and out["too_large_refused"]
    assert _same(out["on"][0]) == cnt(computed=1, published=1) and _same(out["on"][1]) == cnt(hits_copied=1)
    assert out["size_off_again"] == 0 and _same(out["off_again"]) == ZERO


def test_hit_and_miss_at_one_item():
    out = _child("hit_miss")
    assert _same(out["first"]) == cnt(computed=1, published=1) and out["first"]["got"] == [OK]
    assert _same(out["second"]) == cnt(hits_copied=1) and out["second"]["got"] == [OK]
    assert _same(out["forged_over_cached"]) == cnt(hits_copied=1)
    assert out["forged_over_cached"]["got"] == [VERIFY_FAIL]
    assert _same(out["other_key"]) == cnt(hits_copied=1) and out["other_key"]["got"] == [OK]
    # the same message under another DST is another key: a miss, then a hit of its own
    assert _same(out["other_dst_valid"]) == cnt(computed=1, published=1) and out["other_dst_valid"]["got"] == [OK]
    assert _same(out["other_dst_again"]) == cnt(hits_copied=1) and out["other_dst_again"]["got"] == [VERIFY_FAIL]
    for run in out["long_message"]:   # 65 bytes: hashed, never kept
        assert _same(run) == cnt(computed=1) and run["got"] == [OK]


def test_both_hash_forms():
    out = _child("forms")
    assert _same(out["registered_first"]) == cnt(computed=1, published=1)
    assert _same(out["then_unregistered"]) == cnt(hits_chained=1)
    assert _same(out["unregistered_first"]) == cnt(computed=1, published=1)
    assert _same(out["then_registered"]) == cnt(hits_copied=1)
    assert _same(out["aggregate_67_of_100"]) == cnt(hits_copied=1)
    assert _same(out["aggregate_with_stranger"]) == cnt(hits_chained=1)
    for k in ("registered_first", "then_unregistered", "unregistered_first", "then_registered",
              "aggregate_67_of_100", "aggregate_with_stranger"):
        assert out[k]["got"] == [OK], k
    assert _same(out["aggregate_forged"]) == cnt(computed=1, published=1)
    assert out["aggregate_forged"]["got"] == [VERIFY_FAIL]


def test_two_items_one_cached_one_not():
    out = _child("two_items")
    assert _same(out["warm"]) == cnt(computed=1, published=1)
    assert _same(out["one_cached_one_not"]) == cnt(hits_copied=1, computed=1, published=1)
    assert _same(out["both_cached_mixed_forms"]) == cnt(hits_copied=1, hits_chained=1)
    assert out["one_cached_one_not"]["got"] == [OK, OK] == out["both_cached_mixed_forms"]["got"]


def test_duplicates_within_a_call():
    """five items over one message: each computes on its own, only the first gets a slot"""
    out = _child("duplicates")
    assert _same(out["cold"]) == cnt(computed=5, published=1)
    assert _same(out["repeated"]) == cnt(hits_copied=4, hits_chained=1)
    assert out["cold"]["got"] == [OK, OK, VERIFY_FAIL, OK, OK] == out["repeated"]["got"]
    assert out["stats"] == [1, 0, 0]


def test_the_failure_table_twice():
    """bad encodings, a signature outside G1, the identity signature, an empty key list, a key
    outside G2, the identity key and an identity key sum beside valid items: the oracle's statuses
    both times, and the second run hashes nothing"""
    out = _child("failures")
    n = out["n"]
    assert out["n_bad"] == 11 and n == 23
    first, second = _same(out["first"]), _same(out["second"])
    assert sum(1 for w in out["first"]["want"] if w) == 11
    assert first == cnt(computed=n, published=out["n_messages"])
    assert second["computed"] == 0 and second["published"] == 0
    assert second["hits_copied"] + second["hits_chained"] == n
    assert second["hits_copied"] > 0 and second["hits_chained"] > 0
    assert out["stats"] == [out["n_messages"], 0, 0]


@pytest.mark.parametrize("cap", [4, 1])
def test_eviction_keeps_the_newest(cap):
    """hash_ahead of 6 distinct messages into a ring of 4 (and of 1), then 6 one-item verifies:
    exactly the last cap messages hit, and all 6 are OK.  The verifies run newest first (5, 4, ..
    0).  In the order 0 .. 5 no message could hit whatever the ring kept: message 0 misses, and a
    miss reserves the FIFO's oldest slot for its own message, which is message 6 - cap's, the first
    one the test expects to find (tests/test_bls_msg_ring_host.py test_fifo_keeps_the_newest pins
    that order on the host)."""
    out = _child("eviction", str(cap))
    assert out["size"] == cap
    for k in range(6):
        run = out["runs"][str(k)]
        msgs = _same(run)
        assert run["got"] == [OK]
        if k >= 6 - cap:
            assert msgs == cnt(hits_copied=1), (k, msgs)     # exactly the last cap messages are there
        else:
            assert msgs == cnt(computed=1, published=1), (k, msgs)
    assert out["stats"] == [cap, 0, 0]


def test_the_gate():
    """ahead messages gated on a valid and on a forged item, an ungated one, one over the length
    limit, one the call itself verifies over and a duplicate"""
    out = _child("gate")
    assert out["checks_ok"] and out["plain"]["got"] == [OK, VERIFY_FAIL] == out["with_ahead"]["got"]
    assert out["plain"]["msgs"] == cnt(computed=2, published=2)
    assert out["with_ahead"]["msgs"] == cnt(hits_copied=2, ahead_published=2)
    found = out["found"]
    assert found[0] == cnt(hits_copied=1), "gated on the valid item: kept"
    assert found[1] == cnt(computed=1, published=1), "gated on the forged item: not kept"
    assert found[2] == cnt(hits_copied=1), "no gate: kept"
    assert out["bad_gate_refused"]


def test_the_types_layer_hashes_certificate_digests_ahead():
    on, off = _child("types", "on"), _child("types", "off")
    assert on["ring"] == 64 and off["ring"] == 0
    for out in (on, off):
        for call in ("call1", "call2"):
            assert out[call]["got"] == out[call]["want"], (call, out[call])
    assert on["call1"]["got"] == off["call1"]["got"] and on["call2"]["got"] == off["call2"]["got"]
    hc = on["call1"]["got"][0]
    assert hc[0] == 0 and hc[1] != 0 and hc[2] == 0, "the forged header alone is rejected"
    assert on["call2"]["got"][1] == [0] * 6 and on["call2"]["got"][2] == [0] * 3
    # call 1: three header ids hashed and kept, two certificate digests hashed ahead (not the forged header's)
    assert on["call1"]["msgs"] == cnt(computed=3, published=3, ahead_published=2)
    # call 2: the three header signatures inside the certificates hit (ids kept by call 1); the
    # two votes and the aggregate of each valid header hit; those of the forged header miss
    assert on["call2"]["msgs"] == cnt(hits_copied=9, computed=3, published=1)
    assert off["call1"]["msgs"] == ZERO and off["call2"]["msgs"] == ZERO
    assert on["stats"] == [6, 0, 0] and off["stats"] == [0, 0, 0]


def test_six_threads_on_a_ring_of_eight():
    out = _child("concurrency")
    assert out["errors"] == [] and out["bad"] == [], out
    assert out["calls"] == [20] * 6
    assert out["statuses_seen"] == [OK, VERIFY_FAIL]
    held, busy, pinned = out["stats"]
    assert busy == 0 and pinned == 0 and 1 <= held <= 8


def test_hash_ahead_fills_every_device_object():
    out = _child("replicas", NWV_BLS_DEVICE_REPLICAS="3", NWV_DEVICE_REPLICAS="3")
    assert out["devices"] == 3 and out["staged_ok"]
    assert out["placed"] == [[1, 0, 0], [0, 1, 0], [0, 0, 1]], out["placed"]
    for run in out["runs"]:
        assert _same(run) == cnt(hits_copied=1) and run["got"] == [OK]


@pytest.mark.parametrize("arg,env,path", [("", {"NWV_BLS_WAVE_MAX": "4"}, "wave"),
                                          ("batch", {}, "batch_rejected_then_per_item"),
                                          ("per_item", {}, "per_item")])
def test_paths_that_ignore_the_ring(arg, env, path):
    out = _child("ignored", arg, **env)
    assert out["size"] == 64 and out["path"] == path
    for run in (out["first"], out["second"], out["with_ahead"]):
        assert _same(run) == ZERO
        assert run["got"] == [OK, OK, OK, OK, VERIFY_FAIL, OK]
