"""The batch MSM's coefficients on the device, pinned with cancelling forgeries (tests/zcoeff.py):
every touched signature is individually invalid, and the batch equation's error term vanishes
exactly when the device's z_i, for every touched i, is the documented PRF value under the caller's
seed.  So the MSM verdict must accept under the construction's seed and reject under any other --
on both sides of every switch of msm_plan / msm_launch, on the keyed, digest, aggregate and staged
calls, on every kernel form an environment knob or a flag selects, and on a call split over three
device objects (per-range seed, local indices).  A truncated or colliding coefficient, a dropped
signature or a stale seed breaks the cancellation (tests/test_zcoeff_host.py shows the method
bites).  The paths without coefficients (one-launch, comb) must reject the same sets.

The work runs in child processes (tests/zcoeff_gpu_check.py, one JSON line each): the library
reads its environment once per process."""
import json
import os
import subprocess
import sys

import pytest

import zcoeff_gpu_check as zg
from narwhal_amd import _lib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = ("NWV_MSM_TAIL_S", "NWV_TAIL_QUAD_MAX_N", "NWV_BUCKET_QUAD_MAX_N", "NWV_MSM_ROW_PREP_MAX", "NWV_NO_HOST_POLL",
         "NWV_MSM_SEG", "NWV_STAGE_CHAIN", "NWV_DEVICE_REPLICAS", "NWV_SHARD_MIN", "NWV_MSM_MIN_N",
         "NWV_KEYCACHE_MAX_KEYS", "NWV_MSM_SORT2_MIN_PTS", "NWV_TAIL_QUAD_TOP_C", "NWV_TAIL_SPIN_LIMIT")


def _child(parts, flags=0, **env):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env)
    p = subprocess.run([sys.executable, os.path.join(HERE, "zcoeff_gpu_check.py"), "--parts", parts, "--flags",
                        str(flags)], env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _case(out, key):
    r = out[key]
    assert "error" not in r, r["error"]
    return r


def _accepts_under_its_seed_only(r, oracle):
    """the three checks of a case"""
    assert r["valid_accepts"], r
    assert r["touched_differ"], r
    if oracle:
        assert r["oracle_rejects_touched"], r  # every touched signature alone is invalid
    else:
        assert "oracle_rejects_touched" not in r
    assert r["seed_accepts_nobits"], r
    assert r["seed_accepts_bits"] and r["no_fallback"], r
    assert r["other_rejects_nobits"], r
    assert r["other_rejects_bits"], r  # rejected, and the bits are the oracle's
    assert r["path_ran"] and r["runs"]["tiny"] == 0 and r["runs"]["comb"] == 0, r["runs"]


@pytest.fixture(scope="module")
def main_out():
    return _child("default,keyed,other")


def test_seg2_boundary_is_the_plans():
    assert zg.seg2_max_n() == zg.SEG2_MAX_N
    assert zg.plan(zg.SEG2_MAX_N, zg.SEG2_MAX_N, env={})["seg"] == 2
    assert zg.plan(zg.SEG2_MAX_N + 1, zg.SEG2_MAX_N + 1, env={})["seg"] == 8


@pytest.mark.parametrize("n", zg.DEFAULT_SIZES)
def test_default_plan_distinct_keys(main_out, n):
    r = _case(main_out, f"default_{n}")
    assert r["n"] == r["touched"] == n
    _accepts_under_its_seed_only(r, oracle=n <= zg.ORACLE_MAX)
    assert r["plan_matches_engine"], r["plan"]
    # the switches this size sits at (a check of the size list against the plan)
    p = r["plan"]
    assert p["seg"] == (2 if n <= zg.SEG2_MAX_N else 8)
    assert p["chunks"] == (1 if n <= 4095 else 2 if n <= 4097 else 3 if n == 8192 else 5)
    assert p["narrow_top"] == (n > 16384)


@pytest.mark.parametrize("fused", ["fused", "nofused"])
@pytest.mark.parametrize("cache,n", zg.KEYED_CASES + [("kc", 64), ("nokc", 64)])
def test_keyed_batches_over_a_committee(main_out, cache, n, fused):
    r = _case(main_out, f"keyed_{cache}_{fused}_{n}")
    assert r["n"] == r["touched"] == n
    _accepts_under_its_seed_only(r, oracle=n <= zg.ORACLE_MAX)


def test_keyed_digests_call(main_out):
    r = _case(main_out, "digests")
    assert r["n"] == 700 and r["digests_equal"]
    _accepts_under_its_seed_only(r, oracle=True)


def test_aggregate_batch_call(main_out):
    r = _case(main_out, "aggregate")
    assert r["valid_accepts"] and r["msm_runs"] == 10
    for name in ("all", "second", "across"):
        assert all(r[name].values()), (name, r[name])


@pytest.mark.parametrize("pair", zg.SPARSE_PAIRS, ids=lambda p: "%d-%d" % p)
def test_sparse_pairs_name_the_culprit(main_out, pair):
    r = _case(main_out, "sparse_%d_%d" % pair)
    assert r["n"] == zg.SPARSE_N and r["touched"] == 2
    _accepts_under_its_seed_only(r, oracle=True)


def _staged(r):
    assert r["valid_accepts"], r
    n = 4096
    # S accepts, S with its last bit flipped rejects every signature, S accepts again, another seed rejects
    assert r["verdicts"] == [[True, n], [False, 0], [True, n], [False, 0]], r
    assert r["tally_after_1"] == [1, 0] and r["tally_after_3"] == [2, 1], r


@pytest.mark.parametrize("kind", ["staged", "staged_keyed"])
def test_staged_batch_replays_with_the_runs_seed(main_out, kind):
    _staged(_case(main_out, kind))


@pytest.mark.parametrize("kind", ["staged", "staged_keyed"])
def test_staged_batch_graph_replay_with_the_runs_seed(kind):
    """NWV_STAGE_CHAIN=0: the second and later runs replay a captured graph, whose kernels read the
    seed from device memory"""
    _staged(_case(_child("staged", NWV_STAGE_CHAIN="0"), kind))


@pytest.mark.parametrize("n", [4, 64, 65, 1000])
def test_paths_without_coefficients_reject(main_out, n):
    """one-launch (n <= 64) and comb paths over a registered committee: every touched bit false
    under any seed, the construction's included"""
    r = _case(main_out, f"nocoeff_{n}")
    assert r["n"] == r["touched"] == n
    assert r["valid_accepts"] and r["touched_differ"] and r["oracle_rejects_touched"], r
    assert r["seed_rejects_nobits"] and r["seed_rejects_bits"], r
    assert r["other_rejects_nobits"] and r["other_rejects_bits"], r
    want = {"tiny": 0, "msm": 0, "each": 0, "comb": 0}
    want["tiny" if n <= 64 else "comb"] = 5
    assert r["runs"] == want


FORMS = {
    "tail_s_64": ({"NWV_MSM_TAIL_S": "64"}, 0),
    "tail_lane_local_narrow_top": ({"NWV_TAIL_QUAD_MAX_N": "0"}, 0),
    "bucket_lanes": ({"NWV_BUCKET_QUAD_MAX_N": "0"}, 0),
    "prep_lanes": ({"NWV_MSM_ROW_PREP_MAX": "0"}, 0),
    "no_host_poll": ({"NWV_NO_HOST_POLL": "1"}, 0),
    "seg_1": ({"NWV_MSM_SEG": "1"}, 0),
    "seg_64": ({"NWV_MSM_SEG": "64"}, 0),
    "sort2": ({}, _lib.NWV_FLAG_MSM_SORT2),
    "split_prep": ({}, _lib.NWV_FLAG_MSM_SPLIT_PREP),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_forms_the_defaults_reach_only_at_large_sizes(form):
    env, flags = FORMS[form]
    out = _child("forms", flags=flags, **env)
    sizes = zg.FORMS_SIZES + ([zg.FORMS_WIDE_N] if form == "tail_s_64" else [])
    for n in sizes:
        r = _case(out, f"forms_{n}")
        assert r["n"] == r["touched"] == n
        _accepts_under_its_seed_only(r, oracle=n <= zg.ORACLE_MAX)
        assert r["plan_matches_engine"], r["plan"]
        p = r["plan"]
        if form == "tail_s_64":
            # (lg C + 1) S_w over the plan's windows: above 256 k_msm_tail_wide runs.  1,025 and
            # 4,097 stay at or below it (64 chunks a window in k_msm_tail, 4,097 at exactly 256)
            assert p["tail_S"] == 64
            assert p["tail_items"] == {1025: 192, 4097: 256, zg.FORMS_WIDE_N: 320}[n]
        elif form == "tail_lane_local_narrow_top":
            assert p["narrow_top"] and p["widths"][0] == max(p["widths"]) and p["widths"][-1] == min(p["widths"])
        elif form in ("seg_1", "seg_64"):
            assert p["seg"] == int(env["NWV_MSM_SEG"])
        if form == "sort2":
            assert p["chunks"] == (1 if n == 1025 else 2)  # the two-level sort runs at 4,097 only


def test_split_over_device_objects():
    """three device objects, ranges of at least 1,024: a set built per range with the range's
    derived seed and local indices is accepted; one built with the caller's seed and global
    indices, or one whose sum vanishes only over all ranges together, is rejected"""
    out = _child("shard", NWV_DEVICE_REPLICAS="3", NWV_SHARD_MIN="1024")
    assert out["devices"] == 3 and out["ranges"] == [[0, 1024], [1024, 2112], [2112, 3137]]
    for kind in ("shard_batch", "shard_keyed"):
        r = _case(out, kind)
        for k in ("valid_accepts", "touched_differ", "local_accepts_nobits", "local_accepts_bits", "no_fallback",
                  "local_other_rejects", "local_last_bit_rejects", "global_rejects_nobits", "global_rejects_bits",
                  "one_sum_over_ranges_rejects"):
            assert r[k], (kind, k, r)
        assert r["msm_runs"] == 3 * 8, r  # every call ran the MSM on each of the three ranges
