"""The comb pass behind a rejected registered-key batch MSM (narwhal_amd/csrc/comb_kernels.hip
k_ed_comb_pass4 / k_ed_comb_pass16, nwv_set_comb_pass_max): a keyed call above 64 signatures whose
keys all have a comb table goes through the batch MSM, and when the MSM does not accept and the
verdict bits are wanted, the bad set is named from the key combs in one launch.  Its bits must equal
the oracle's ZIP-215 verdicts and those of a context with the limit at 0 (today's per-signature
pass) at sizes on both sides of a verdict word and off every workgroup multiple, on forgeries of
every kind, on every golden / ZIP-215 vector, across an epoch change of the key cache, through the
types layer and the grouped trait call, from two threads at once and on a three-replica context
(child script tests/comb_pass_gpu_check.py); nwv_diag_comb_pass and the counters say which path
ran."""
import json
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

import oracle_ffi as of
from narwhal_amd import _lib
from test_gpu_comb import _batch, _forge_set

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = ("NWV_COMB_KEYS", "NWV_DEVICE_REPLICAS", "NWV_COMB_PASS_L")


@pytest.fixture(scope="module")
def engs():
    import narwhal_amd
    a = narwhal_amd.Engine(device=0)
    a.set_comb_batch_max(0)
    a.set_comb_pass_max(4096)
    z = narwhal_amd.Engine(device=0)
    z.set_comb_batch_max(0)
    z.set_comb_pass_max(0)
    rnd = random.Random(4097)
    seeds = [rnd.randbytes(32) for _ in range(10)]
    keys = [of.pubkey(s) for s in seeds]
    for eng in (a, z):
        eng.keycache_register(keys)
    assert a.comb_pass_max == 4096 and z.comb_pass_max == 0
    yield a, z, seeds, keys
    for eng in (a, z):
        eng.close()


def _delta(eng, fn):
    """run fn -> (its result, the movement of the four path counters, that of diag_comb_pass)"""
    c0, p0 = eng.diag_counters_ex(), eng.diag_comb_pass()
    r = fn()
    c1, p1 = eng.diag_counters_ex(), eng.diag_comb_pass()
    return r, {k: c1[k] - c0[k] for k in c1}, (p1[0] - p0[0], p1[1] - p0[1])


@pytest.mark.parametrize("n", [65, 127, 128, 129, 193, 257, 1000])
def test_sizes_and_forgeries_match_oracle(engs, n):
    a, z, seeds, keys = engs
    kidx, sigs, msgs = _batch(a, seeds, n, n)
    _, want = _forge_set(keys, kidx, sigs, msgs, 7 * n)
    (ok, bits), d, p = _delta(a, lambda: a.verify_batch_keyed(keys, kidx, sigs, msgs))
    assert bits == want
    assert not ok
    assert d == {"tiny": 0, "msm": 1, "each": 1, "comb": 0}
    assert p == (1, n)
    (okz, bz), dz, pz = _delta(z, lambda: z.verify_batch_keyed(keys, kidx, sigs, msgs))
    assert bz == want and not okz
    assert dz == {"tiny": 0, "msm": 1, "each": 1, "comb": 0}
    assert pz == (0, 0) and z.diag_comb_pass() == (0, 0)


def test_valid_batch_and_batch_verdict_only_run_no_pass(engs):
    a, _, seeds, keys = engs
    kidx, sigs, msgs = _batch(a, seeds, 300, 300)
    (ok, bits), d, p = _delta(a, lambda: a.verify_batch_keyed(keys, kidx, sigs, msgs))
    assert ok and all(bits) and len(bits) == 300
    assert d == {"tiny": 0, "msm": 1, "each": 0, "comb": 0} and p == (0, 0)  # the MSM accepted
    _forge_set(keys, kidx, sigs, msgs, 5)
    (ok, none), d, p = _delta(a, lambda: a.verify_batch_keyed(keys, kidx, sigs, msgs, want_bits=False))
    assert not ok and none is None
    assert d == {"tiny": 0, "msm": 1, "each": 0, "comb": 0} and p == (0, 0)


def test_golden_and_zip215_vectors_in_one_call(engs):
    """every committed vector (Appendix-B categories, the 196-case small-order table) as ONE keyed
    call over registered keys, undecodable and small-order keys included"""
    a = engs[0]
    vecs = [(bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"]))
            for v in of.load_golden("ed25519_vectors.json")["vectors"]]
    vecs += [(bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"]))
             for v in of.load_golden("zip215_small_order.json")["vectors"]]
    assert len(vecs) > 300
    keys = sorted({p for p, _, _ in vecs})
    kpos = {k: i for i, k in enumerate(keys)}
    a.keycache_register(keys)
    want = [of.verify(*v) for v in vecs]
    assert set(want) == {True, False}
    (ok, bits), d, p = _delta(a, lambda: a.verify_batch_keyed(keys, [kpos[k] for k, _, _ in vecs],
                                                              [s for _, s, _ in vecs], [x for _, _, x in vecs]))
    assert bits == want and not ok
    assert p == (1, len(vecs)) and d["comb"] == 0 and d["tiny"] == 0


def test_path_selection(engs):
    import narwhal_amd
    a, _, seeds, keys = engs
    n = 100
    kidx, sigs, msgs = _batch(a, seeds, n, 100)
    _, want = _forge_set(keys, kidx, sigs, msgs, 100)

    def run(eng, ks=keys, ki=kidx, sg=sigs, w=want):
        (ok, bits), d, p = _delta(eng, lambda: eng.verify_batch_keyed(ks, ki, sg, msgs))
        assert bits == w and not ok
        assert d == {"tiny": 0, "msm": 1, "each": 1, "comb": 0}
        return p

    assert run(a) == (1, n)
    # one key without a comb table (never registered; the call caches it itself): the whole pass
    # takes today's path
    extra_seed = random.Random(5).randbytes(32)
    extra = of.pubkey(extra_seed)
    sg2 = list(sigs)
    sg2[50] = of.sign(extra_seed, msgs[50])
    ki2 = kidx[:50] + [10] + kidx[51:]
    w2 = [of.verify((keys + [extra])[ki2[i]], sg2[i], msgs[i]) for i in range(n)]
    assert w2[50] and w2[:50] == want[:50] and w2[51:] == want[51:]
    assert run(a, keys + [extra], ki2, sg2, w2) == (0, 0)
    # contexts whose flags force a path never take it, with the limit set
    for flag in (_lib.NWV_FLAG_NO_TINY, _lib.NWV_FLAG_MSM_ALWAYS):
        eng = narwhal_amd.Engine(device=0, flags=flag)
        try:
            eng.keycache_register(keys)
            eng.set_comb_batch_max(0)
            eng.set_comb_pass_max(4096)
            assert eng.comb_pass_max == 4096
            assert run(eng) == (0, 0)
            assert eng.diag_comb_pass() == (0, 0)
        finally:
            eng.close()
    try:
        a.set_comb_pass_max(n - 1)  # n = limit + 1
        assert a.comb_pass_max == n - 1
        assert run(a) == (0, 0)
        a.set_comb_pass_max(n)
        assert run(a) == (1, n)
        a.set_comb_pass_max(0)  # 0 after a non-zero value turns it off
        assert a.comb_pass_max == 0
        assert run(a) == (0, 0)
        # at or above the shard minimum a call splits over devices: clamped below
        a.set_comb_pass_max(10**9)
        assert 4096 < a.comb_pass_max < 10**9
        if "NWV_SHARD_MIN" not in os.environ:
            assert a.comb_pass_max == 16383
        assert run(a) == (1, n)
    finally:
        a.set_comb_pass_max(4096)
    assert a.comb_pass_max == 4096
    # 64 signatures stay on the one-launch path
    (ok, bits), d, p = _delta(a, lambda: a.verify_batch_keyed(keys, kidx[:64], sigs[:64], msgs[:64]))
    assert bits == want[:64] and not ok
    assert d == {"tiny": 1, "msm": 0, "each": 0, "comb": 0} and p == (0, 0)


def test_types_layer_mixed_call_of_a_large_committee():
    """three certificates of a 100-node committee (67 votes and the header's signature each) and
    their headers in ONE verify_mixed call, one vote forged: the codes are the oracle
    restatement's, and the bad set came from one comb pass"""
    import narwhal_amd
    import types_util as tu
    from types_util import nt
    from narwhal_amd import types as T
    e = narwhal_amd.Engine(device=0)
    try:
        e.set_comb_batch_max(0)
        e.set_comb_pass_max(4096)
        rnd = random.Random(29)
        fx = nt.CommitteeFixture(100, of.pubkey, of.sign, seed=29)
        c = tu.committee(fx.committee)
        q = fx.committee.quorum_threshold()
        assert q == 67
        parents = [rnd.randbytes(32) for _ in range(q)]
        heads, certs = [], []
        for au in range(3):
            h = fx.header(author_idx=au, parents=parents, payload=[(rnd.randbytes(32), au)])
            heads.append(h)
            certs.append(tu.oracle_certificate(fx, h, [i for i in range(100) if i != au][:q]))
        (gh, gv, gc), d, p = _delta(e, lambda: T.verify_mixed(e, c, [tu.header(h) for h in heads], (),
                                                              [tu.certificate(x) for x in certs]))
        assert gh == [0, 0, 0] and gv == [] and gc == [0, 0, 0]
        assert p == (0, 0) and d["msm"] == 1 and d["each"] == 0
        s = certs[1]["sigs"][40]
        certs[1] = dict(certs[1], sigs=certs[1]["sigs"][:40] + [s[:5] + bytes([s[5] ^ 2]) + s[6:]] +
                        certs[1]["sigs"][41:])
        (gh, gv, gc), d, p = _delta(e, lambda: T.verify_mixed(e, c, [tu.header(h) for h in heads], (),
                                                              [tu.certificate(x) for x in certs]))
        assert gh == [nt.header_verify(fx.committee, h, of.verify) for h in heads] == [0, 0, 0]
        assert gc == [nt.certificate_verify(fx.committee, x, of.verify) for x in certs]
        assert gc[0] == gc[2] == 0 and gc[1] != 0
        assert p[0] == 1 and p[1] >= 3 * 68
        assert d == {"tiny": 0, "msm": 1, "each": 1, "comb": 0}
    finally:
        e.close()


def test_grouped_trait_call(engs):
    """nwv_ed25519_verify_batch_grouped with bits asked for and every key cached"""
    a, z, seeds, keys = engs
    n = 200
    kidx, sigs, msgs = _batch(a, seeds, n, 200)
    _, want = _forge_set(keys, kidx, sigs, msgs, 200)
    pk, sig, arena, offs, lens = _lib.soa([(keys[kidx[i]], sigs[i], msgs[i]) for i in range(n)])
    g0 = a.diag_grouped()
    (ok, bits), d, p = _delta(a, lambda: a.verify_batch_grouped_arrays(pk, sig, arena, offs, lens))
    assert list(bits) == want and not ok
    assert a.diag_grouped()["cached"] == g0["cached"] + 1
    assert d == {"tiny": 0, "msm": 1, "each": 1, "comb": 0} and p == (1, n)
    (okz, bz), _, pz = _delta(z, lambda: z.verify_batch_grouped_arrays(pk, sig, arena, offs, lens))
    assert list(bz) == want and not okz and pz == (0, 0)


def test_two_threads_one_engine(engs):
    """two threads, five calls each of 300 signatures with different forged sets, on one engine:
    each call has its lane's verdict words, so every call's bits are its own"""
    a, _, seeds, keys = engs
    jobs = []
    for t in range(2):
        kidx, sigs, msgs = _batch(a, seeds, 300, 310 + t)
        _, want = _forge_set(keys, kidx, sigs, msgs, 41 + t)
        jobs.append((kidx, sigs, msgs, want))
    assert jobs[0][3] != jobs[1][3]
    out = [[], []]

    def work(t):
        kidx, sigs, msgs, _ = jobs[t]
        for _ in range(5):
            out[t].append(a.verify_batch_keyed(keys, kidx, sigs, msgs))

    p0 = a.diag_comb_pass()
    th = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=60)
    assert not any(x.is_alive() for x in th)
    for t in range(2):
        assert len(out[t]) == 5
        for ok, bits in out[t]:
            assert bits == jobs[t][3] and not ok
    assert a.diag_comb_pass() == (p0[0] + 10, p0[1] + 3000)


def _child(part, **env):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env)
    p = subprocess.run([sys.executable, os.path.join(HERE, "comb_pass_gpu_check.py"), "--part", part], env=e,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    return out


def test_epoch_change_reuses_tables():
    """NWV_COMB_KEYS=8 (read once per process: a child): eight keys take every table, four are
    retired, four new keys take the freed tables.  A forged batch over live keys takes the pass; one
    that names a retired key does not; a signature by retired key k named under new key j, for all
    sixteen (j, k), is rejected"""
    r = _child("epoch", NWV_COMB_KEYS="8")
    assert r["comb_keys"] == "8"
    assert r["stats_K"] == [9, 8] and r["retired"] == [4, 4] and r["stats_retained"] == [5, 4]
    assert r["stats_N"] == [9, 8]  # every table in use again: the new keys' are the freed ones
    assert r["live"] == {"equal": True, "ok": False, "rejected": r["live"]["rejected"], "pass": [1, 100]}
    assert r["live"]["rejected"] > 4
    assert r["retired_named"]["equal"] and not r["retired_named"]["ok"] and r["retired_named"]["pass"] == [0, 0]
    assert r["retired_named"]["rejected"] > 4
    assert r["crossed"]["equal"] and not r["crossed"]["ok"] and r["crossed"]["pass"] == [1, 100]
    assert r["crossed"]["crossed_rejected"] == 16 and r["crossed"]["rejected"] == 16


def test_three_replicas():
    """NWV_DEVICE_REPLICAS=3 (read at nwv_init: a child process): one forged 300-signature call from
    each of three overlapping threads gives the oracle's bits from whichever device object serves it"""
    r = _child("replicas", NWV_DEVICE_REPLICAS="3")
    assert r["devices"] == 3
    assert r["alive"] == [False] * 3
    assert r["equal"] == [True] * 3 and r["ok"] == [False] * 3
    assert r["sets_differ"] and min(r["rejected"]) > 4
    assert r["pass"] == [3, 900]
    assert sum(r["each_by_device"]) == 3
