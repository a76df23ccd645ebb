"""The latency class on the GPU (nwv_set_latency_max; narwhal_amd/csrc/lane_pool.h inside the
library): off by default, classification at the bounds, the reserved lanes' stream priority, small
calls beside bulk callers on one lane of each kind, beside a key-cache retain, and over device
replicas.  Whatever the lane, every verdict, bad set, status, digest and DagError code equals the
oracle's; which class a call ran in is read from nwv_diag_qos.  The child script is
tests/qos_gpu_check.py (the variables are read at nwv_init); one child per part, each under a time
limit: a part that does not end inside it fails, and is not run again."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
OWN = ("NWV_LANES", "NWV_LATENCY_LANES", "NWV_LATENCY_DIGEST_BYTES", "NWV_LATENCY_PRIORITY", "NWV_DEVICE_REPLICAS",
       "NWV_BLS_DEVICE_REPLICAS", "NWV_PLACE", "NWV_SHARD_MIN", "NWV_B2_SHARD_MIN", "NWV_BLS_SHARD_MIN")


def _run(part, **env):
    e = {k: v for k, v in os.environ.items() if k not in OWN}
    e.update(env)
    p = subprocess.run([sys.executable, os.path.join(HERE, "qos_gpu_check.py"), "--part", part], env=e,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    return out


def _all_checks(out, at_least):
    failed = sorted(k for k, v in out["checks"].items() if not v)
    assert not failed, (failed, out)
    assert len(out["checks"]) >= at_least


def test_off_by_default_no_call_is_latency_class_and_no_reserved_lane_opens():
    out = _run("off")
    _all_checks(out, 13)
    for name in ("ed25519", "bls"):
        q = out[name]
        assert q["latency_calls"] == 0 and q["latency_reserved"] == 0 and q["reserved_open"] == 0, (name, q)


def test_classification_at_the_bounds_and_the_priority_in_force():
    out = _run("edge", NWV_LATENCY_DIGEST_BYTES="4096")
    _all_checks(out, 40)
    for name in ("ed25519", "bls"):
        pr, q = out[f"{name}_priority"], out[name]
        assert pr[0] == pr[1], (name, pr)  # the reserved lane's stream reports the greatest priority
        assert 1 <= q["reserved_open"] <= q["reserved_cap"], (name, q)
    assert out["clamped"] == [16383, 255]


def test_small_ed25519_calls_beside_a_bulk_caller_on_one_lane_of_each_kind():
    out = _run("beside", NWV_LANES="1", NWV_LATENCY_LANES="1")
    _all_checks(out, 6)
    assert out["errors"] == [] and out["mismatches"] == []
    d = out["delta"]
    assert d["latency_calls"] == 3 * 130 and d["latency_reserved"] <= d["latency_calls"] and d["other_calls"] >= 40


def test_bls_single_verifies_beside_a_bulk_caller():
    out = _run("beside_bls", NWV_LATENCY_LANES="1")
    _all_checks(out, 6)
    assert out["errors"] == [] and out["mismatches"] == []
    d = out["delta"]
    assert d["latency_calls"] == 2 * 20 and d["latency_reserved"] <= d["latency_calls"] and d["other_calls"] >= 10


def test_a_retain_and_a_registration_beside_latency_class_certificates():
    out = _run("keycache")
    _all_checks(out, 6)
    assert out["errors"] == [] and out["mismatches"] == []


def test_latency_class_calls_over_three_device_objects():
    out = _run("replicas", NWV_DEVICE_REPLICAS="3", NWV_BLS_DEVICE_REPLICAS="3")
    _all_checks(out, 6)
    assert out["errors"] == [] and out["mismatches"] == []
    per = out["per_device"]
    assert len(per) == 3 and all(p[5] <= p[6] for p in per)
    assert sum(p[0] for p in per) >= 6 * 24
