"""Typed calls in one launch (nwv_set_typed_fused; k_ed_tiny_fused / k_ed_comb_fused):
with the setting on, a header / vote / certificate verification by registered committee keys runs its
digests and its signatures in a single launch; with it off, and for every call that does not
qualify, it takes the launches it took before.  The results must equal the oracle restatement
(oracle/narwhal_types.py) in both modes for every item kind and DagError, for header preimages on
both sides of every 128-byte block edge, for certificates on both sides of the tiny / comb edge and
for forgeries of R, s, s + l and the message; the digests must equal hashlib's; the diagnostics say
which form ran.  The checks run in a fresh child process (tests/typed_fused_gpu_check.py)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = ("NWV_DEVICE_REPLICAS", "NWV_COMB_KEYS", "NWV_NO_HOST_POLL", "NWV_LIB")


def _child(part, **env):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env)
    p = subprocess.run([sys.executable, os.path.join(HERE, "typed_fused_gpu_check.py"), "--part", part],
                       env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def main():
    return _child("main")


@pytest.fixture(scope="module")
def fallback():
    return _child("fallback")


def test_setter_and_default():
    import narwhal_amd
    e = narwhal_amd.Engine(device=0)
    try:
        assert e.typed_fused is False and e.diag_typed_fused() == (0, 0, 0)  # the default is off
        e.set_typed_fused(True)
        assert e.typed_fused is True
        e.set_typed_fused(False)
        assert e.typed_fused is False
    finally:
        e.close()


def test_every_item_kind_matches_oracle_in_both_modes(main):
    assert main["setting"] == [True, False]
    assert main["bad"] == []
    for size in (4, 34, 94):
        assert set(main[f"codes_{size}"]) >= {0, 10, 11, 12, 13, 14, 15}


def test_path_selection_by_counters(main):
    # a C1 certificate (3 + 1 signatures): one fused tiny launch, no per-signature pass, no MSM
    on, off = main["c1_on"], main["c1_off"]
    assert on["result"] == [0] and off["result"] == [0]
    assert on["counters"] == {"tiny": 1, "msm": 0, "each": 0, "comb": 0} and on["fused"] == [1, 0, 0]
    assert off["counters"] == {"tiny": 1, "msm": 0, "each": 0, "comb": 0} and off["fused"] == [0, 0, 0]
    # 64 + 1 signatures: the comb kernel, fused and unfused
    on, off = main["c94_on"], main["c94_off"]
    assert on["result"] == [0] and off["result"] == [0]
    assert on["counters"] == {"tiny": 0, "msm": 0, "each": 0, "comb": 1} and on["fused"] == [0, 1, 0]
    assert off["counters"] == {"tiny": 0, "msm": 0, "each": 0, "comb": 1} and off["fused"] == [0, 0, 0]
    assert main["off_fused_total"] == [0, 0, 0]
    for tag in ("on", "off"):  # the device's own counters count fused launches where they count the others
        d = main[f"device_counters_{tag}"]
        assert d[0] == d[2] and d[1] == d[3]


def test_digest_outputs_equal_hashlib_in_both_modes(main):
    assert main["digest_bad"] == []
    assert main["typed_call_on"] == [1, 0, 0] and main["typed_call_off"] == [0, 0, 0]
    # a signature over a side preimage's digest has a device dependency: the two-launch form
    assert main["side_signed_on"] == [0, 0, 1] and main["side_signed_off"] == [0, 0, 0]


def test_two_threads_on_one_engine(main):
    assert main["threads"] == [True, True]


def test_calls_that_take_the_fallback_form(fallback):
    assert fallback["bad"] == []
    for tag in ("no_tiny", "msm_always"):  # the flags exclude the path: every call counted as a fallback
        f = fallback[tag]
        assert f[0] == 0 and f[1] == 0 and f[2] > 0
    u = fallback["unregistered"]
    assert u["ok"] and u["verdicts"] == [True, True, True] and u["digests"] and u["fused"] == [0, 0, 1]
    r = fallback["round"]
    assert r["signatures"] >= 7000 and r["equal"] and r["rejected"] == [1, 2]
    assert r["fused"] == [0, 0, 1] and r["counters"]["tiny"] == 0 and r["counters"]["comb"] == 0


def test_three_replica_context():
    r = _child("replicas", NWV_DEVICE_REPLICAS="3")
    assert r["devices"] == 3 and r["alive"] == [False] * 3
    assert r["equal"] == [True] * 3
    assert r["fused"][0] > 0 and r["fused"][1] > 0
