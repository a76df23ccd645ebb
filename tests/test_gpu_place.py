"""Placement of calls over a multi-device context on the GPU (narwhal_amd/csrc/place.h inside the
library): an all-devices context over three device objects of either engine on this one GPU
(NWV_DEVICE_REPLICAS=3, NWV_BLS_DEVICE_REPLICAS=3).  A call that does not split goes to the
least-loaded device, the ranges of one that splits rotate, NWV_PLACE=first keeps device 0 / device
k, and whatever the device, every verdict, bad set, status, digest and DagError code equals the
oracle's.  Where a call ran is read from nwv_diag_device_counters.  The child script is
tests/place_gpu_check.py (the variables are read at nwv_init); one child per part."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _run(part, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("NWV_PLACE", "NWV_SHARD_MIN", "NWV_BLS_SHARD_MIN")}
    e.update(NWV_DEVICE_REPLICAS="3", NWV_BLS_DEVICE_REPLICAS="3", **env)
    p = subprocess.run([sys.executable, os.path.join(HERE, "place_gpu_check.py"), "--part", part], env=e,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    return out


def _all_checks(out, at_least):
    failed = sorted(k for k, v in out["checks"].items() if not v)
    assert not failed, failed
    assert len(out["checks"]) >= at_least


def test_a_held_device_pushes_the_next_call_to_the_next_device():
    out = _run("hold")
    _all_checks(out, 60)
    for name in ("certificate", "certificate_bad", "batch128", "keyed_new", "blake2b", "mixed", "serialized"):
        assert out["placed"][name] == [[0, 1, 0], [0, 0, 1], [1, 0, 0]], name
    assert out["placed"]["bls_verify_held"] == [0, 4, 0]
    assert out["placed"]["bls_aggregate_verified"] == [0, 1, 0]
    assert out["placed"]["bls_aggregate_fresh"] == [1, 0, 0]


def test_split_calls_rotate_over_the_devices():
    out = _run("rotate", NWV_SHARD_MIN="64")
    _all_checks(out, 8)
    assert out["ranges"] == [2, 2, 2] and out["items"] == [128, 128, 128]


def test_nwv_place_first_keeps_range_k_on_device_k():
    out = _run("rotate", NWV_SHARD_MIN="64", NWV_PLACE="first")
    _all_checks(out, 8)
    assert out["place"] == "first" and out["ranges"] == [3, 3, 0] and out["items"] == [192, 192, 0]


def test_six_threads_of_every_call_shape_at_once():
    out = _run("threads")
    _all_checks(out, 8)
    assert out["errors"] == [] and out["mismatches"] == []
    assert sum(out["ed25519_distribution"]) + sum(out["bls_distribution"]) == 6 * 12
