"""The key-transposed batch check of large BLS calls (nwv_bls_set_key_batch_min: the random linear
combination regrouped by registered key, distinct keys + 1 Miller loops and one final
exponentiation per group of NWV_BLS_KEY_GROUP eligible items, the per-item check for the groups
that reject and for the items that stay out) against bls_ffi.fast_aggregate_verify.  Every
configuration runs in a fresh child (tests/bls_key_batch_gpu_check.py): the environment is read
once per process.  With NWV_BLS_WAVE_MAX=0 every call is a large wave call, and with
NWV_BLS_KEY_GROUP_RATIO=0 groups of six items over a 4-key committee are formed although they gain
nothing, so a handful of items reach every edge: a partial last group, groups of unequal key
counts, a product tree of one level."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERIFY_FAIL = 5
LAYOUTS = ["onekey", "certs", "mixed"]
ACCEPTED, REJECTED = "key_batch_accepted", "key_batch_rejected_then_per_item"


def _child(scenario, layout="mixed", **env):
    e = dict(os.environ, NWV_BLS_WAVE_MAX="0", NWV_BLS_KEY_GROUP="6", NWV_BLS_KEY_GROUP_RATIO="0",
             NWV_BLS_DEVICE_REPLICAS="1")
    e.update(env)
    for k in [k for k, v in e.items() if v is None]:
        del e[k]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bls_key_batch_gpu_check.py"), scenario, layout],
                       env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_all_valid_sizes(layout):
    """n = 1, 6, 7, 13, 23 valid items at group size 6: all 0, ceil(n / 6) groups that all accept,
    distinct keys + 1 Miller loops a group, nothing re-checked"""
    out = _child("sizes", layout)
    assert out["min_fresh"] == 0
    for n in (1, 6, 7, 13, 23):
        run = out["runs"][str(n)]
        assert run["want"] == [0] * n
        assert run["got"] == run["want"], (n, run)
        assert run["path"] == ACCEPTED, (n, run)
        assert run["kb"] == [(n + 5) // 6, 0, 0, run["millers"], n], (n, run)
        assert run["batch"] == [0, 0, 0]


def test_groups_that_gain_nothing_take_the_setting_off_path():
    """without the ratio override six items over three or four keys form no group: the call runs as
    with the setting at 0, statuses and path"""
    out = _child("no_override", NWV_BLS_KEY_GROUP_RATIO=None)
    assert out["on"]["want"][9] == VERIFY_FAIL and sum(1 for w in out["on"]["want"] if w) == 1
    assert out["on"]["got"] == out["on"]["want"] == out["off"]["got"]
    assert out["on"]["path"] == out["off"]["path"] == "wave"
    assert out["on"]["kb"] == out["off"]["kb"] == [0] * 5


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_forgery_rechecks_one_group(layout):
    out = _child("forgery", layout)
    assert out["want"][14] == VERIFY_FAIL and sum(1 for w in out["want"] if w) == 1
    assert out["got"] == out["want"], out
    assert out["path"] == REJECTED
    assert out["kb"][:3] == [5, 1, 6] and out["kb"][4] == 30


@pytest.mark.parametrize("layout", LAYOUTS)
def test_cancelling_forgeries_in_one_group(layout):
    """sig_a + D and sig_b - D in one group: S_g is what it is with the honest signatures, so only
    the per-item weights make the group reject"""
    out = _child("cancel", layout)
    a, b = out["a"], out["b"]
    assert out["same_sum"] and a // 6 == b // 6
    assert out["want"][a] == VERIFY_FAIL and out["want"][b] == VERIFY_FAIL
    assert out["got"] == out["want"], out
    assert [i for i, g in enumerate(out["got"]) if g] == [a, b]
    assert out["path"] == REJECTED and out["kb"][:3] == [3, 1, 6]


def test_swapped_signers_on_one_message():
    """item A carries key 1's signature and names key 2, item B the reverse, one message, one
    group: T_1 and T_2 swap what they should hold, the product without coefficients is 1"""
    out = _child("swap", "onekey")
    assert out["unweighted"] == 0
    assert [i for i, w in enumerate(out["want"]) if w] == [7, 9]
    assert out["got"] == out["want"], out
    assert out["path"] == REJECTED and out["kb"][:3] == [3, 1, 6]


def test_multiplicity_and_sharing():
    """a key named twice by one item, one key on several messages, one message under several keys"""
    out = _child("multi")
    assert out["want"] == [0] * 10
    assert out["got"] == out["want"], out
    assert out["path"] == ACCEPTED and out["kb"] == [2, 0, 0, out["millers"], 10]


def test_items_that_stay_out():
    """a bad encoding, a signature outside G1, the identity signature, an empty key list, an
    identity key sum of two registered keys, items naming an unregistered valid key and an
    unregistered key outside G2, beside valid items: the oracle's statuses, no group rejects, and
    key 3 -- named by such items only -- gets no Miller entry"""
    out = _child("outside")
    assert sum(1 for w in out["want"] if w == 0) == out["n_valid"] == 16
    assert out["got"] == out["want"], out
    assert out["path"] == ACCEPTED
    assert out["kb"][0] == 3 and out["kb"][1] == 0 and out["kb"][3] == out["millers"] == 11 and out["kb"][4] == 14
    w = out["with_wrong_key"]
    assert w["want"][-1] == VERIFY_FAIL and w["got"] == w["want"], w
    assert w["path"] == REJECTED and w["kb"][0] == 3 and w["kb"][1] == 1 and w["kb"][3] == 12 and w["kb"][4] == 15


def test_sharded_one_forgery_per_shard():
    out = _child("sharded", NWV_BLS_DEVICE_REPLICAS="3", NWV_BLS_SHARD_MIN="8")
    assert [i for i, w in enumerate(out["want"]) if w] == [3, 14, 27]
    assert out["got"] == out["want"], out


def test_off_by_default():
    """a fresh context has the setting at 0 and a 1,100-item call takes the per-item wave path;
    with the setting on the same call takes the key-transposed check (one group, the committee's
    four keys + 1 Miller loops) and gives the same statuses; back at 0 the wave path returns"""
    out = _child("default_off", NWV_BLS_WAVE_MAX=None, NWV_BLS_KEY_GROUP=None, NWV_BLS_KEY_GROUP_RATIO=None)
    assert out["min_fresh"] == 0 and out["min_set"] == 1 and out["min_after_zero"] == 0
    assert out["want"] == [0] * 1100
    assert out["off"] == {"got": out["want"], "path": "wave", "kb": [0] * 5}
    assert out["on"] == {"got": out["want"], "path": ACCEPTED, "kb": [1, 0, 0, 5, 1100]}
    assert out["off_again"] == out["off"]


def test_goes_before_the_wave_batch_check():
    out = _child("precedence")
    assert out["good"]["got"] == out["good"]["want"] == [0] * 13
    assert out["good"]["path"] == ACCEPTED and out["good"]["batch"] == [0, 0, 0]
    assert out["forged"]["got"] == out["forged"]["want"] and out["forged"]["want"][8] == VERIFY_FAIL
    assert out["forged"]["path"] == REJECTED and out["forged"]["batch"] == [0, 0, 0]


def test_through_validate_certificates():
    """seven certificates of a 4-node committee, one with another certificate's aggregate: the
    invalid set is the oracle's, and the call went through the key-transposed check"""
    out = _child("types")
    assert out["q"] == 3 and out["want_invalid"] == [4]
    assert not out["ok"] and out["invalid"] == out["want_invalid"]
    assert out["path"] in (ACCEPTED, REJECTED) and out["kb"][0] >= 1
