"""The dense key-sum stage of large BLS calls (nwv_bls_set_apk_dense_min: k_blsd_total, k_blsd_apk
with 4, 8 or 16 lanes an item, k_blsw_apk_list for the items that keep the per-item code) against
bls_ffi.fast_aggregate_verify and against the same call with the setting at 0.  Every
configuration runs in a fresh child (tests/bls_apk_dense_gpu_check.py): the environment is read
once per process.  With NWV_BLS_WAVE_MAX=0 every call is a large wave call, so a handful of items
reach every edge: a wave's last group empty, full or spilling into the next wave, lists shorter
than, equal to and longer than the lanes, sums taken directly and from the key table's total."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, AGGR_MISMATCH, VERIFY_FAIL, PK_INFINITY = 0, 4, 5, 6
KB_ACCEPTED, KB_REJECTED = "key_batch_accepted", "key_batch_rejected_then_per_item"


def _child(scenario, *args, **env):
    e = dict(os.environ, NWV_BLS_WAVE_MAX="0", NWV_BLS_DEVICE_REPLICAS="1", NWV_BLS_KEY_GROUP="6",
             NWV_BLS_KEY_GROUP_RATIO="0", NWV_BLS_BATCH_GROUP="4")
    e.pop("NWV_BLS_APK_LANES", None)
    e.update(env)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bls_apk_dense_gpu_check.py"), scenario, *args],
                       env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _same_as_off_and_oracle(run):
    assert run["on"]["got"] == run["want"], run
    assert run["off"]["got"] == run["want"], run
    assert run["off"]["dense"] == [0, 0, 0, 0], run


@pytest.mark.parametrize("lanes", [4, 8, 16])
def test_lanes_and_item_counts(lanes):
    """1, 64 / L - 1, 64 / L, 64 / L + 1 and 33 items, list lengths 2, 3, L - 1, L, L + 1 and 7,
    committees of 4 and 7 registered keys: all valid, every item in the dense kernel, by complement
    exactly where the list is strictly ascending over more than half of the committee"""
    out = _child("sizes", NWV_BLS_APK_LANES=str(lanes))
    assert out["lanes"] == lanes and len(out["runs"]) == 10
    for run in out["runs"]:
        n = run["n"]
        assert run["want"] == [OK] * n, run
        _same_as_off_and_oracle(run)
        assert run["on"]["dense"] == [n - run["comp"], run["comp"], 0, lanes], run
        assert run["on"]["path"] == run["off"]["path"] == "wave"
    assert any(run["comp"] for run in out["runs"]) and any(run["n"] - run["comp"] for run in out["runs"])


def test_path_choice():
    """3-of-4 and 4-of-4 by complement; 2-of-4, a descending list and a list naming a key twice
    directly; a one-key item and an empty list through the per-item kernel.  Over a table with an
    unregistered key nothing goes by complement, and the item naming that key is per-item too."""
    out = _child("paths")
    a, b = out["registered_table"], out["table_with_unregistered_key"]
    assert a["want"] == [OK] * 6 + [AGGR_MISMATCH]
    _same_as_off_and_oracle(a)
    assert a["on"]["dense"] == [3, 2, 2, 4]
    assert b["want"] == [OK] * 6 + [AGGR_MISMATCH, OK]
    _same_as_off_and_oracle(b)
    assert b["on"]["dense"] == [5, 0, 3, 4]


def test_identity_sums():
    """{a, -a, b} signed by {a, -a}: the complement equals the total -> PK_INFINITY; by {a, b}: OK.
    {a, -a} signed by both: an identity total and an empty complement -> PK_INFINITY.
    {a, -a, b, -b} signed by {a, b, -b}: an identity total -> OK."""
    out = _child("identity")
    for name, want, dense in (("a_na_b", [PK_INFINITY, OK], [0, 2, 0, 4]), ("a_na", [PK_INFINITY], [0, 1, 0, 4]),
                              ("a_na_b_nb", [OK], [0, 1, 0, 4])):
        run = out[name]
        assert run["want"] == want, (name, run)
        _same_as_off_and_oracle(run)
        assert run["on"]["dense"] == dense, (name, run)


@pytest.mark.parametrize("mode", ["per_item", "key_batch", "wave_batch"])
def test_the_pairing_reads_the_dense_record(mode):
    """valid certificates summed by complement are OK on every pairing path; with one signer
    swapped in a certificate's list that certificate alone fails"""
    out = _child("pairing", mode)
    good, bad = out["good"], out["swapped"]
    assert out["swapped_by_complement"]
    assert good["want"] == [OK] * 9
    assert bad["want"] == [OK] * 4 + [VERIFY_FAIL] + [OK] * 4
    for run in (good, bad):
        _same_as_off_and_oracle(run)
        assert run["on"]["dense"] == [0, 9, 0, 4], run
        assert run["on"]["path"] == run["off"]["path"]
    if mode == "per_item":
        assert good["on"]["path"] == bad["on"]["path"] == "wave"
    elif mode == "key_batch":
        assert good["on"]["path"] == KB_ACCEPTED and bad["on"]["path"] == KB_REJECTED
        assert good["on"]["kb"] == good["off"]["kb"] and good["on"]["kb"][0] == 2
    else:
        assert good["on"]["batch"] == good["off"]["batch"] == [3, 0, 0]
        assert bad["on"]["batch"][:2] == [3, 1]


def test_setting_edges():
    """off by default; a call of n - 1 items stays on today's launches and a call of n items takes
    the stage; a call of at most NWV_BLS_WAVE_MAX items never does"""
    out = _child("edges", NWV_BLS_WAVE_MAX="8")
    assert out["min_fresh"] == 0 and out["min_set"] == 12 and out["min_after_zero"] == 0
    for name, n, dense in (("at_12_items_11", 11, [0] * 4), ("at_12_items_12", 12, [0, 12, 0, 4]),
                           ("at_1_items_8", 8, [0] * 4), ("at_1_items_9", 9, [0, 9, 0, 4])):
        run = out[name]
        assert run["want"] == [OK] * n, (name, run)
        _same_as_off_and_oracle(run)
        assert run["on"]["dense"] == dense, (name, run)
        assert run["on"]["path"] == run["off"]["path"] == "wave"


def test_sharded_statuses():
    out = _child("sharded", NWV_BLS_DEVICE_REPLICAS="3", NWV_BLS_SHARD_MIN="8")
    assert [i for i, w in enumerate(out["want"]) if w] == [3, 14, 27]
    assert out["on"]["got"] == out["want"] == out["off"]["got"], out
