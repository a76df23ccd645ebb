"""k_msm_prep's second trimming on the device: the hash role's reduction by folding, its unreduced
sums of z_i s_i handed to k_msm_tail, the in-order digit recoding, and the lane-local decompression
with u, v and u v^3 parked in LDS.

NWV_FLAG_NO_ROW_PREP sends small batches through the lane-local decompression (they otherwise
decompress on 16-lane rows) and NWV_FLAG_MSM_ALWAYS through the batch MSM at every size.  A batch
is accepted only if every z_i k_i, the sum of z_i s_i, every digit and every point record is right,
so an accepted all-valid batch pins the arithmetic; forged batches must be rejected, with the
oracle's verdict for every signature.  One child process per engine configuration computes every
case once; the tests read its report.

Sizes: 1; 64 and 65 (the wave edge of both roles); 255, 256 and 257 (one hash workgroup, then two:
the partial hand-off); 300.  The signatures of every all-valid batch are the ones with the largest
s out of 2,400 signed (s > l (1 - 1/8): the sums of z_i s_i run as wide as a signer makes them);
s = l - 1 itself cannot be signed for, so it is patched into one signature and must be rejected
as the oracle rejects it."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (1, 64, 65, 255, 256, 257, 300)

PRELUDE = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, os.environ["NWV_T_HERE"]); sys.path.insert(0, os.path.dirname(os.environ["NWV_T_HERE"]))
import oracle_ffi as of
import narwhal_amd
from narwhal_amd import _lib
L = 2**252 + 27742317777372353535851937790883648493
P = 2**255 - 19
D = -121665 * pow(121666, P - 2, P) % P
BASE = _lib.NWV_FLAG_MSM_ALWAYS | _lib.NWV_FLAG_NO_ROW_PREP
out = {}
def signed(e, n, rng, mlen=32):
    seeds = [rng.bytes(32) for _ in range(n)]
    msgs = [rng.bytes(mlen) for _ in range(n)]
    pk, sg = e.sign_many(seeds, msgs)
    return [(pk[32*i:32*i+32].tobytes(), sg[64*i:64*i+64].tobytes(), msgs[i]) for i in range(n)]
def s_of(it):
    return int.from_bytes(it[1][32:], "little")
def run(e, items, want):
    # -> [verdict without bits (the MSM's own), verdict, bits equal the oracle's, MSM runs]
    before = e.diag_counters()["msm"]
    ok_nobits, _ = e.verify_batch(items, want_bits=False)
    ok, bits = e.verify_batch(items)
    return [ok_nobits, ok, bits == want, e.diag_counters()["msm"] - before]
"""

PLAIN_CHILD = PRELUDE + r"""
e = narwhal_amd.Engine(device=0, flags=BASE)
rng = np.random.default_rng(252)
pool = sorted(signed(e, 2400, rng), key=s_of, reverse=True)
out["largest_s_over_l"] = s_of(pool[0]) / L
out["smallest_s_used_over_l"] = s_of(pool[299]) / L
for n in json.loads(os.environ["NWV_T_SIZES"]):
    items = pool[:n]
    want = [of.verify(*it) for it in items]
    r = {"oracle_valid": all(want), "valid": run(e, items, want), "forged": [], "index": []}
    boundary = 256 if n > 256 else 64 if n > 64 else n // 2
    for i in sorted({0, n - 1, boundary}):
        p, s, m = items[i]
        forged = list(items)
        forged[i] = (p, s[:32] + bytes([s[32] ^ 1]) + s[33:], m)  # s + 1 or s - 1
        fwant = list(want)
        fwant[i] = of.verify(*forged[i])
        r["index"].append(i)
        r["forged"].append([not fwant[i]] + run(e, forged, fwant))
    # s = l - 1 by construction
    i = n // 3
    p, s, m = items[i]
    top = list(items)
    top[i] = (p, s[:32] + (L - 1).to_bytes(32, "little"), m)
    twant = list(want)
    twant[i] = of.verify(*top[i])
    r["s_top"] = [not twant[i]] + run(e, top, twant)
    out[str(n)] = r

# 512-byte messages (five SHA-512 blocks), one full hash workgroup
items = signed(e, 256, rng, 512)
want = [of.verify(*it) for it in items]
r = {"oracle_valid": all(want), "valid": run(e, items, want)}
p, s, m = items[255]
forged = items[:255] + [(p, s, m[:511] + bytes([m[511] ^ 0x80]))]
fwant = want[:255] + [of.verify(*forged[255])]
r["forged"] = [not fwant[255]] + run(e, forged, fwant)
out["msg512"] = r

# n = 257, the edge encodings in both decompression roles.  The ZIP-215 small-order vectors are
# all valid (14 encodings as A times 14 as R: x = 0 with the sign bit set, y >= p, every small
# order); with 61 valid golden vectors they make a batch the MSM must accept.
g = of.load_golden("ed25519_vectors.json")
z = of.load_golden("zip215_small_order.json")
tup = lambda v: (bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"]))
zv = [tup(v) for v in z["vectors"]]
gv = [tup(v) for v in g["vectors"]]
gwant = [of.verify(*it) for it in gv]
good = zv + [it for it, w in zip(gv, gwant) if w][:257 - len(zv)]
want = [of.verify(*it) for it in good]
out["edge_valid"] = {"n": len(good), "oracle_valid": all(want), "run": run(e, good, want)}
# every golden vector (valid and invalid mixed) and small-order ones up to 257
mixed = (gv + zv)[:257]
mwant = [of.verify(*it) for it in mixed]
out["edge_mixed"] = {"n": len(mixed), "rejects": mwant.count(False), "run": run(e, mixed, mwant)}
# a non-square (y with (y^2 - 1) / (d y^2 + 1) not a square), x = 0 with the sign bit set and
# y >= p, each as R and as A of one otherwise valid signature of a 257 batch, at a time
def non_square():
    y = 2
    while True:
        u, v = (y * y - 1) % P, (D * y * y + 1) % P
        w = u * pow(v, P - 2, P) % P
        if pow(w, (P - 1) // 2, P) == P - 1:
            return y.to_bytes(32, "little")
        y += 1
encs = {"non_square": non_square(), "neg_zero": (1 | 1 << 255).to_bytes(32, "little"),
        "y_ge_p": (P + 3).to_bytes(32, "little")}
base = pool[:257]
bwant = [True] * 257
enc_runs = {}
for name, enc in encs.items():
    for role, i in (("R", 100), ("A", 256)):
        p, s, m = base[i]
        items = list(base)
        items[i] = (p, enc + s[32:], m) if role == "R" else (enc, s, m)
        w = list(bwant)
        w[i] = of.verify(*items[i])
        enc_runs[name + "_" + role] = [not w[i]] + run(e, items, w)
out["edge_single"] = enc_runs
e.close()
print(json.dumps(out))
"""

KEYED_CHILD = PRELUDE + r"""
# keyed batches share `partial` and the digit rows with the plain form: the one-launch form
# (default), the fused key sums (NWV_FLAG_NO_TINY) and the k_msm_keysum launch
# (NWV_FLAG_NO_FUSED_KEYSUM), key cache on and off
def keyed(items):
    keys = list(dict.fromkeys(it[0] for it in items))
    return keys, [keys.index(it[0]) for it in items]
forms = {"default": 0, "fused": _lib.NWV_FLAG_NO_TINY, "keysum": _lib.NWV_FLAG_NO_TINY | _lib.NWV_FLAG_NO_FUSED_KEYSUM}
for name, f in forms.items():
    for kc in (0, _lib.NWV_FLAG_NO_KEYCACHE):
        e = narwhal_amd.Engine(device=0, flags=BASE | f | kc)
        for n, m in ((4, 4), (4, 2), (64, 64), (64, 5)):
            rng = np.random.default_rng(100 * n + m)
            kseeds = [rng.bytes(32) for _ in range(m)]
            msgs = [rng.bytes(32) for _ in range(n)]
            pk, sg = e.sign_many([kseeds[i % m] for i in range(n)], msgs)
            items = [(pk[32*i:32*i+32].tobytes(), sg[64*i:64*i+64].tobytes(), msgs[i]) for i in range(n)]
            want = [of.verify(*it) for it in items]
            keys, kidx = keyed(items)
            sigs = [it[1] for it in items]
            ok, bits = e.verify_batch_keyed(keys, kidx, sigs, msgs)
            ok_nobits, _ = e.verify_batch_keyed(keys, kidx, sigs, msgs, want_bits=False)
            r = [all(want), ok, ok_nobits, bits == want]
            for bad in (0, n - 1):
                s = sigs[bad]
                sigs2 = list(sigs)
                sigs2[bad] = s[:32] + bytes([s[32] ^ 1]) + s[33:]
                w = list(want)
                w[bad] = of.verify(items[bad][0], sigs2[bad], msgs[bad])
                ok, bits = e.verify_batch_keyed(keys, kidx, sigs2, msgs)
                ok_nobits, _ = e.verify_batch_keyed(keys, kidx, sigs2, msgs, want_bits=False)
                r += [not w[bad], not ok, not ok_nobits, bits == w]
            out["%s_kc%d_%d_%d" % (name, 0 if kc else 1, n, m)] = r
        e.close()
print(json.dumps(out))
"""


def child(script, **env):
    full = dict(os.environ, NWV_T_HERE=HERE, **env)
    p = subprocess.run([sys.executable, "-c", script], env=full, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def plain():
    return child(PLAIN_CHILD, NWV_T_SIZES=json.dumps(list(SIZES)))


@pytest.fixture(scope="module")
def keyed():
    return child(KEYED_CHILD)


def accepted(run, n_calls=2):
    """[MSM verdict, verdict, bits == oracle, MSM runs]: accepted, by the batch MSM"""
    return run[0] and run[1] and run[2] and run[3] >= n_calls


def rejected(run):
    """[oracle rejects the changed signature, MSM verdict, verdict, bits == oracle, MSM runs]"""
    return run[0] and not run[1] and not run[2] and run[3] and run[4] >= 2


def test_pool_reaches_large_s(plain):
    assert plain["largest_s_over_l"] > 1 - 1 / 300 and plain["smallest_s_used_over_l"] > 1 - 1 / 6, plain


@pytest.mark.parametrize("n", SIZES)
def test_lane_local_prep_at_the_edges_of_its_roles(plain, n):
    r = plain[str(n)]
    assert r["oracle_valid"] and accepted(r["valid"]), r
    assert len(r["forged"]) == len(set(r["index"])) >= (1 if n == 1 else 2), r
    for i, f in zip(r["index"], r["forged"]):
        assert rejected(f), (n, i, f)
    assert rejected(r["s_top"]), r


def test_five_block_messages_fill_a_hash_workgroup(plain):
    r = plain["msg512"]
    assert r["oracle_valid"] and accepted(r["valid"]) and rejected(r["forged"]), r


def test_edge_encodings_in_both_decompression_roles(plain):
    v, m = plain["edge_valid"], plain["edge_mixed"]
    assert v["n"] == 257 and v["oracle_valid"] and accepted(v["run"]), v
    assert m["n"] == 257 and m["rejects"] > 50, m
    run = m["run"]
    assert not run[0] and not run[1] and run[2] and run[3] >= 2, m
    assert sorted(plain["edge_single"]) == ["neg_zero_A", "neg_zero_R", "non_square_A", "non_square_R",
                                            "y_ge_p_A", "y_ge_p_R"]
    for name, f in plain["edge_single"].items():
        assert rejected(f), (name, f)


def test_keyed_forms_share_the_partials_and_digit_rows(keyed):
    assert len(keyed) == 3 * 2 * 4
    for name, r in keyed.items():
        assert all(r), (name, r)
