"""k_msm_tail's chunk sums by rows and columns and the larger bucket chunks of large batches, on the
device, at the smallest sizes that take the lane bucket kernel (4,160 and 8,229 signatures: above
the 4,096 where the quad bucket kernel ends).  Such small batches run their tail butterflies on
quads by default, so every child runs with NWV_TAIL_QUAD_MAX_N=0 and NWV_TAIL_QUAD_TOP_C=0: every
chunk lane-local, as at 65,536.  Forms:

  NWV_MSM_SEG       the chunk size msm_plan's rule gives the 65,536-signature headline
                    (test_msm_seg_rule.RULE_SEG_HEADLINE), and 1: every bucket of three or more
                    entries spans three or more bucket lanes, so the tail's join adds two or more
                    continuation pieces for almost every bucket;
  NWV_TAIL_RC_MIN_C the default (256-bucket chunks by rows and columns, smaller ones by the
                    butterfly) and 2 (every chunk by rows and columns: 128 and 256 at these sizes,
                    a rectangular and a square view).

Each size and form: the clean batch, one forged signature (rejected, the bad set exact through the
fallback), a cancelling forgery pair under pinned coefficients, and the same over 100 keys in the
key cache -- against the oracle, in child processes (tests/tail_rc_gpu_check.py)."""
import json
import os
import subprocess
import sys

import pytest

import tail_rc_gpu_check as tc
from test_gpu_zcoeff import KNOBS, _accepts_under_its_seed_only, _case
from test_msm_seg_rule import RULE_SEG_HEADLINE

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FORMS = {
    "rule_seg": {"NWV_MSM_SEG": str(RULE_SEG_HEADLINE)},
    "rule_seg_rc_all": {"NWV_MSM_SEG": str(RULE_SEG_HEADLINE), "NWV_TAIL_RC_MIN_C": "2"},
    "seg_1": {"NWV_MSM_SEG": "1"},
    "seg_1_rc_all": {"NWV_MSM_SEG": "1", "NWV_TAIL_RC_MIN_C": "2"},
}
_outs = {}


def _out(form):
    if form not in _outs:
        e = {k: v for k, v in os.environ.items() if k not in KNOBS + ("NWV_TAIL_RC_MIN_C",)}
        e.update(FORMS[form], NWV_TAIL_QUAD_MAX_N="0", NWV_TAIL_QUAD_TOP_C="0")
        p = subprocess.run([sys.executable, os.path.join(HERE, "tail_rc_gpu_check.py")], env=e, capture_output=True,
                           text=True, timeout=240)
        assert p.returncode == 0, p.stderr[-3000:]
        _outs[form] = json.loads(p.stdout.strip().splitlines()[-1])
    return _outs[form]


@pytest.mark.parametrize("n", tc.SIZES)
@pytest.mark.parametrize("kind", ["plain", "keyed"])
@pytest.mark.parametrize("form", list(FORMS))
def test_lane_tail_against_the_oracle(form, kind, n):
    r = _case(_out(form), f"{kind}_{n}")
    # the chunk forms this case reached: 256-bucket chunks in every plan, 128 beside them
    assert 256 in r["chunk_sizes"] and min(r["chunk_sizes"]) >= 64, r["chunk_sizes"]
    if kind == "plain":
        assert r["plan_matches_engine"] and r["plan"]["seg"] == int(FORMS[form]["NWV_MSM_SEG"]), r["plan"]
        assert r["plan"]["chunks"] > 1  # the sort's chunked path: the bucket lanes find their keys by search
        if FORMS[form]["NWV_MSM_SEG"] == "1":
            assert r["plan"]["entries"] > 16 * r["plan"]["buckets"]  # ~17 entries, so ~17 lanes, a bucket
    f = r["forged"]
    assert f["oracle_bad_set"] == [(2 * n) // 3], f
    assert f["rejects_nobits"] and f["rejects_bits"] and f["bits_are_the_oracles"] and f["fallback_ran"], f
    assert f["msm_runs"] == 2, f
    p = r["pair"]
    assert p["n"] == n and p["touched"] == 2
    _accepts_under_its_seed_only(p, oracle=n <= 1100)
