"""The trimmed batch MSM on the device: the lane bucket kernel with its seeded accumulator at
several chunk sizes, and the SHA-512 sums at every padding boundary.

k_msm_bucket (one lane per chunk of T sorted entries) turns a chunk's first record into its running
sum instead of adding it to the identity.  NWV_BUCKET_QUAD_MAX_N=0 sends every batch through that
kernel (small batches otherwise take the quad form) and NWV_MSM_SEG sets T: 1 (the seeded entry
also closes the chunk), 2, 15 (the headline's) and 64 (the largest the plan picks).  Both are read
once per process, so each configuration runs in a fresh child.  Verdicts, and the exact set of
rejected signatures, are compared with the oracle."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# with the 64 bytes of R || A these straddle every padding boundary of one to five blocks
SHA_LENGTHS = (0, 1, 46, 47, 48, 63, 64, 111, 112, 127, 128, 175, 176, 191, 192, 255, 256, 511, 512, 513)

PRELUDE = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, os.environ["NWV_T_HERE"]); sys.path.insert(0, os.path.dirname(os.environ["NWV_T_HERE"]))
import oracle_ffi as of
import narwhal_amd
e = narwhal_amd.Engine(device=0)
out = {}
def signed(n, rng, lens=None):
    seeds = [rng.bytes(32) for _ in range(n)]
    msgs = [rng.bytes(32 if lens is None else lens[i % len(lens)]) for i in range(n)]
    pk, sg = e.sign_many(seeds, msgs)
    return [(pk[32*i:32*i+32].tobytes(), sg[64*i:64*i+64].tobytes(), msgs[i]) for i in range(n)]
"""

BUCKET_CHILD = PRELUDE + r"""
rng = np.random.default_rng(70)
for n in (70, 1024):
    items = signed(n, rng)
    want = [of.verify(*it) for it in items]
    before = e.diag_counters()["msm"]
    ok_nobits, _ = e.verify_batch(items, want_bits=False)
    ok, bits = e.verify_batch(items)
    r = {"oracle_valid": all(want), "valid_nobits": ok_nobits, "valid": ok, "valid_bits": bits == want, "forged": []}
    for i in (0, n // 2, n - 1):
        forged = list(items)
        p, s, m = forged[i]
        forged[i] = (p, s, bytes([m[0] ^ 1]) + m[1:])
        fwant = list(want)
        fwant[i] = of.verify(*forged[i])
        f_nobits, _ = e.verify_batch(forged, want_bits=False)
        f_ok, fb = e.verify_batch(forged)
        r["forged"].append({"oracle_rejects": not fwant[i], "nobits": f_nobits, "ok": f_ok, "exact": fb == fwant})
    r["msm_runs"] = e.diag_counters()["msm"] - before
    out[str(n)] = r
# the golden batches (indices into the vectors, valid and invalid ones mixed) and the ZIP-215
# small-order vectors as one batch
g = of.load_golden("ed25519_vectors.json")
vec = [(bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"])) for v in g["vectors"]]
vwant = [of.verify(*it) for it in vec]
gold = []
for b in g["batches"]:
    items = [vec[i] for i in b["items"]]
    want = [vwant[i] for i in b["items"]]
    ok_nobits, _ = e.verify_batch(items, want_bits=False)
    ok, bits = e.verify_batch(items)
    gold.append([all(want) == b["expect"], ok_nobits == b["expect"], ok == b["expect"], bits == want])
out["golden"] = gold
z = of.load_golden("zip215_small_order.json")
zv = [(bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"])) for v in z["vectors"]]
zwant = [of.verify(*it) for it in zv]
ok_nobits, _ = e.verify_batch(zv, want_bits=False)
ok, bits = e.verify_batch(zv)
out["zip215"] = {"oracle_as_recorded": zwant == [v["expect"] for v in z["vectors"]],
                 "nobits": ok_nobits == all(zwant), "ok": ok == all(zwant), "bits": bits == zwant}
e.close()
print(json.dumps(out))
"""

SHA_CHILD = PRELUDE + r"""
lens = json.loads(os.environ["NWV_T_LENS"])
items = signed(64, np.random.default_rng(512), lens)
assert sorted({len(it[2]) for it in items}) == sorted(lens)
want = [of.verify(*it) for it in items]
ok_nobits, _ = e.verify_batch(items, want_bits=False)
ok, bits = e.verify_batch(items)
out["valid"] = {"oracle_valid": all(want), "nobits": ok_nobits, "ok": ok, "bits": bits == want,
                "each": e.verify_each(items) == want}
# the last byte of every message flipped (the empty message has none and stays valid)
forged = [(p, s, m[:-1] + bytes([m[-1] ^ 0x80]) if m else m) for p, s, m in items]
fwant = [of.verify(*it) for it in forged]
f_nobits, _ = e.verify_batch(forged, want_bits=False)
f_ok, fb = e.verify_batch(forged)
out["forged"] = {"oracle": fwant == [len(it[2]) == 0 for it in items], "nobits": f_nobits, "ok": f_ok,
                 "bits": fb == fwant, "each": e.verify_each(forged) == fwant}
# one forged message at a time
single = []
for i in range(len(lens)):
    if not items[i][2]:
        continue
    one = list(items)
    one[i] = forged[i]
    w = list(want)
    w[i] = fwant[i]
    f_ok, fb = e.verify_batch(one)
    single.append([len(items[i][2]), (not f_ok) and fb == w])
out["single"] = single
e.close()
print(json.dumps(out))
"""


def child(script, **env):
    full = dict(os.environ, NWV_T_HERE=HERE, **env)
    p = subprocess.run([sys.executable, "-c", script], env=full, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("seg", ["1", "2", "15", "64"])
def test_lane_bucket_kernel_with_seeded_accumulator(seg):
    out = child(BUCKET_CHILD, NWV_BUCKET_QUAD_MAX_N="0", NWV_MSM_SEG=seg)
    for n in ("70", "1024"):
        r = out[n]
        assert r["oracle_valid"] and r["valid_nobits"] and r["valid"] and r["valid_bits"], (n, r)
        assert r["msm_runs"] >= 8, (n, r)  # every call went through the batch MSM
        assert len(r["forged"]) == 3
        for f in r["forged"]:
            assert f["oracle_rejects"] and not f["nobits"] and not f["ok"] and f["exact"], (n, r)
    assert len(out["golden"]) == 40 and all(all(g) for g in out["golden"]), out["golden"]
    assert all(out["zip215"].values()), out["zip215"]


def test_sha512_padding_boundaries_on_the_device():
    out = child(SHA_CHILD, NWV_T_LENS=json.dumps(list(SHA_LENGTHS)))
    assert all(out["valid"].values()), out["valid"]
    f = out["forged"]
    assert f["oracle"] and not f["nobits"] and not f["ok"] and f["bits"] and f["each"], f
    assert len(out["single"]) == len(SHA_LENGTHS) - 1 and all(ok for _, ok in out["single"]), out["single"]
