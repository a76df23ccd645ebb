"""One lane serves every Ed25519 path in turn (narwhal_amd/csrc/ed_plan.h).  A batch's
path is planned when it is staged and kept on the lane's buffers, so the way this can go wrong is a
plan left over from the lane's previous batch.  With NWV_LANES=1 and the latency class off, one lane
runs a keyed tiny batch, an un-keyed one of the same size, a comb batch, an un-keyed one, a batch
with the comb pass behind its MSM, an un-keyed one, a tiny batch without bits, a grouped trait call,
a typed call in the one-launch form, a comb batch again, and then stages a keyed batch for
nwv_staged_run.  Every batch has one forged signature at its last index: the verdict bits must equal
the oracle's, and the counters must show the path of this batch, not of the one before.  The calls
run in a fresh child process (tests/ed_paths_gpu_check.py)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = ("NWV_DEVICE_REPLICAS", "NWV_COMB_KEYS", "NWV_NO_HOST_POLL", "NWV_LIB", "NWV_LATENCY_LANES", "NWV_MSM_MIN_N")

ZERO = {"tiny": 0, "msm": 0, "each": 0, "comb": 0, "comb_pass": [0, 0], "typed_fused": [0, 0, 0]}
# (call, counter deltas that are not zero)
EXPECT = [
    ("keyed 64", {"tiny": 1}),
    ("un-keyed 64", {"msm": 1, "each": 1}),
    ("keyed 65", {"comb": 1}),
    ("un-keyed 65", {"msm": 1, "each": 1}),
    ("keyed 129", {"msm": 1, "each": 1, "comb_pass": [1, 129]}),
    ("un-keyed 129", {"msm": 1, "each": 1}),
    ("keyed 64, no bits", {"tiny": 1}),
    ("grouped 65", {"comb": 1}),
    ("typed", {"tiny": 1, "typed_fused": [1, 0, 0]}),
    ("keyed 65 again", {"comb": 1}),
]


@pytest.fixture(scope="module")
def run():
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e["NWV_LANES"] = "1"
    p = subprocess.run([sys.executable, os.path.join(HERE, "ed_paths_gpu_check.py")], env=e, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_one_lane_and_the_limits_in_force(run):
    assert run["lanes_env"] == "1"
    assert run["limits"] == [0, 128, 256]  # latency class off, comb_batch_max, comb_pass_max
    assert run["lanes"] == {"ordinary_open": 1, "reserved_open": 0, "latency_calls": 0}
    # every batch: all valid but the forged last signature
    assert run["oracle_shape"] == {"64": [True, False], "65": [True, False], "129": [True, False]}


def test_every_call_equals_the_oracle(run):
    assert [c["call"] for c in run["calls"]] == [name for name, _ in EXPECT]
    assert [c["call"] for c in run["calls"] if not c["equal"]] == []


@pytest.mark.parametrize("k", range(len(EXPECT)), ids=[name.replace(" ", "_").replace(",", "") for name, _ in EXPECT])
def test_counters_show_this_batchs_path(run, k):
    name, moved = EXPECT[k]
    got = run["calls"][k]
    assert got["call"] == name
    assert got["delta"] == dict(ZERO, **moved)


def test_staged_keyed_batch_after_them(run):
    assert run["staged"] == {"equal": True, "tiny": 0, "comb": 0}
