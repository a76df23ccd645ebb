"""The wave engine's batch check of large BLS calls (nwv_bls_set_wave_batch_min: one Miller loop per
item, one final exponentiation per group of NWV_BLS_BATCH_GROUP items, the per-item check only for
the groups that reject) against bls_ffi.fast_aggregate_verify.  Every configuration runs in a
fresh child (tests/bls_wave_batch_gpu_check.py): the environment is read once per process.  With
NWV_BLS_WAVE_MAX=0 every call is a large wave call, so groups of five and a handful of items reach
every edge: a partial last group, a partial last Miller wave, group boundaries inside a wave."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERIFY_FAIL = 5
LAYOUTS = ["registered", "unregistered", "mixed"]


def _child(scenario, layout="registered", pack="3", **env):
    e = dict(os.environ, NWV_BLS_WAVE_MAX="0", NWV_BLS_BATCH_GROUP="5", NWV_BLS_PACK=pack,
             NWV_BLS_DEVICE_REPLICAS="1")
    e.update(env)
    for k in [k for k, v in e.items() if v is None]:
        del e[k]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bls_wave_batch_gpu_check.py"), scenario, layout],
                       env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("pack", ["1", "3"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_all_valid_sizes(layout, pack):
    """n = 1, 5, 6, 16, 23 valid items at group size 5: all 0, every group accepts, ceil(n / 5)
    groups, nothing re-checked -- with the committee's precomputed key lines, computed lines, and
    both kinds in one wave"""
    out = _child("sizes", layout, pack)
    assert out["min_fresh"] == 0
    for n in (1, 5, 6, 16, 23):
        run = out["runs"][str(n)]
        assert run["want"] == [0] * n
        assert run["got"] == run["want"], (n, run)
        assert run["path"] == "wave_batch_accepted", (n, run)
        assert run["batch"] == [(n + 4) // 5, 0, 0], (n, run)


@pytest.mark.parametrize("layout,pack", [(x, "3") for x in LAYOUTS] + [("mixed", "1")])
def test_one_forgery_rechecks_one_group(layout, pack):
    out = _child("forgery", layout, pack)
    assert out["want"][12] == VERIFY_FAIL and sum(1 for w in out["want"] if w) == 1
    assert out["got"] == out["want"], out
    assert out["path"] == "wave_batch_rejected_then_per_item"
    assert out["batch"] == [5, 1, 5]


def test_two_rejected_groups_share_one_recheck_range():
    """forgeries in items 2 and 17 reject groups 0 and 3: one re-check launch over items 0..19, the
    accepted groups 1 and 2 included; in items 2 and 21 they reject group 0 and the partial last
    group, and the launch ends at the call's 23 items, not at the group's 25"""
    out = _child("two_rejected", "registered", "3")["runs"]
    for name, bad, batch in (("apart", [2, 17], [5, 2, 20]), ("to_the_end", [2, 21], [5, 2, 23])):
        run = out[name]
        assert [i for i, w in enumerate(run["want"]) if w] == bad
        assert all(run["want"][i] == VERIFY_FAIL for i in bad)
        assert run["got"] == run["want"], (name, run)
        assert run["path"] == "wave_batch_rejected_then_per_item", (name, run)
        assert run["batch"] == batch, (name, run)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_cancelling_forgeries_in_one_group(layout):
    """sig_a + D and sig_b - D in one group: the product of the two items' equations without
    coefficients is 1, so only the weights make the group reject"""
    out = _child("cancel", layout)
    a, b = out["a"], out["b"]
    assert out["same_sum"] and a // 5 == b // 5
    assert out["want"][a] == VERIFY_FAIL and out["want"][b] == VERIFY_FAIL
    assert out["got"] == out["want"], out
    assert [i for i, g in enumerate(out["got"]) if g] == [a, b]
    assert out["path"] == "wave_batch_rejected_then_per_item"
    assert out["batch"] == [4, 1, 5]


@pytest.mark.parametrize("layout,pack", [(x, "3") for x in LAYOUTS] + [("mixed", "1")])
def test_pre_pairing_failures_stay_out_of_the_batch(layout, pack):
    """bad encodings, a signature outside G1, the identity signature, an empty key list, a key
    outside G2, the identity key and an identity key sum beside valid items, one group made of
    such items only: the oracle's statuses, and no group rejects"""
    out = _child("pre", layout, pack)
    assert out["n_bad"] == 11 and sum(1 for w in out["want"] if w) == 11
    assert all(w != 0 for w in out["group1_want"])
    assert out["got"] == out["want"], out
    assert out["path"] == "wave_batch_accepted"
    assert out["batch"] == [5, 0, 0]


def test_sharded_one_forgery_per_shard():
    out = _child("sharded", "registered", NWV_BLS_DEVICE_REPLICAS="3", NWV_BLS_SHARD_MIN="8")
    assert [i for i, w in enumerate(out["want"]) if w] == [3, 14, 27]
    assert out["got"] == out["want"], out


def test_off_by_default():
    """a fresh context has the setting at 0 and a 1,100-item call takes the per-item wave path;
    with the setting on the same call takes the batch check and gives the same statuses"""
    out = _child("default_off", NWV_BLS_WAVE_MAX=None, NWV_BLS_BATCH_GROUP=None, NWV_BLS_PACK=None)
    assert out["min_fresh"] == 0 and out["min_after_zero"] == 0 and out["min_set"] == 1
    assert out["want"] == [0] * 1100
    assert out["off"]["got"] == out["want"] and out["off"]["path"] == "wave" and out["off"]["batch"] == [0, 0, 0]
    assert out["on"]["got"] == out["want"] and out["on"]["path"] == "wave_batch_accepted"
    assert out["on"]["batch"][0] >= 1 and out["on"]["batch"][1:] == [0, 0]
