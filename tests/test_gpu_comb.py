"""The comb path for registered-key batches above 64 signatures (narwhal_amd/csrc/comb_kernels.hip
k_ed_comb): a keyed call of 64 < n <= comb_batch_max signatures whose keys all have a comb table
(nwv_keycache_register) is checked signature by signature in one launch.  Its verdict bits must
equal the oracle's ZIP-215 verdicts and those of the batch MSM path (NWV_FLAG_NO_TINY) at sizes on
both sides of a verdict-word boundary and off every workgroup multiple, on forgeries of every kind,
on every golden / ZIP-215 vector (undecodable and small-order keys registered too), through the
types layer and from two threads at once; the diagnostic counters say which path ran."""
import os
import random
import threading

import pytest

import oracle_ffi as of
from narwhal_amd import _lib
from test_gpu_tiny import _forge

pytestmark = pytest.mark.gpu
MSG_LENS = [0, 1, 32, 47, 48, 111, 112, 200, 512]  # 47/48, 111/112: SHA-512 padding after the 64-byte prefix


@pytest.fixture(scope="module")
def engs():
    import narwhal_amd
    e = narwhal_amd.Engine(device=0)
    e.set_comb_batch_max(4096)
    m = narwhal_amd.Engine(device=0, flags=_lib.NWV_FLAG_NO_TINY)
    a = narwhal_amd.Engine(device=0, flags=_lib.NWV_FLAG_MSM_ALWAYS)
    rnd = random.Random(4096)
    seeds = [rnd.randbytes(32) for _ in range(10)]
    keys = [of.pubkey(s) for s in seeds]
    for eng in (e, m, a):
        eng.keycache_register(keys)
    yield e, m, a, seeds, keys
    for eng in (e, m, a):
        eng.close()


def _batch(e, seeds, n, seed):
    """n valid signatures by the committee -> (key_idx, sigs, msgs)"""
    rnd = random.Random(seed)
    kidx = [rnd.randrange(len(seeds)) for _ in range(n)]
    msgs = [rnd.randbytes(rnd.choice(MSG_LENS)) for _ in range(n)]
    _, sg = e.sign_many([seeds[k] for k in kidx], msgs)
    return kidx, [sg[64 * i:64 * i + 64].tobytes() for i in range(n)], msgs


def _forge_set(keys, kidx, sigs, msgs, seed):
    """forge indices {0, 63, 64, n - 1} and n // 7 random others, the four kinds in turn ->
    (forged indices, oracle verdicts)"""
    n = len(sigs)
    rnd = random.Random(seed)
    fixed = {0, 63, 64, n - 1}
    bad = sorted(fixed | set(rnd.sample([i for i in range(n) if i not in fixed], n // 7)))
    for j, i in enumerate(bad):
        sigs[i], msgs[i] = _forge(sigs[i], msgs[i], j % 4)
    want = [of.verify(keys[kidx[i]], sigs[i], msgs[i]) for i in range(n)]
    assert [i for i, w in enumerate(want) if not w] == bad  # (a condition on the inputs)
    return bad, want


@pytest.mark.parametrize("n", [65, 127, 128, 129, 193, 257, 1000])
def test_comb_sizes_and_forgeries_match_oracle(engs, n):
    e, m, _, seeds, keys = engs
    kidx, sigs, msgs = _batch(e, seeds, n, n)
    before = e.diag_counters_ex()
    ok, bits = e.verify_batch_keyed(keys, kidx, sigs, msgs)
    assert ok and all(bits) and len(bits) == n
    after = e.diag_counters_ex()
    assert after["comb"] == before["comb"] + 1  # the comb kernel ran, and nothing else
    assert after["msm"] == before["msm"] and after["tiny"] == before["tiny"]
    ok, none = e.verify_batch_keyed(keys, kidx, sigs, msgs, want_bits=False)
    assert ok and none is None
    _, want = _forge_set(keys, kidx, sigs, msgs, 7 * n)
    before = e.diag_counters_ex()
    ok, bits = e.verify_batch_keyed(keys, kidx, sigs, msgs)
    assert bits == want
    assert not ok
    ok2, _ = e.verify_batch_keyed(keys, kidx, sigs, msgs, want_bits=False)
    assert not ok2
    after = e.diag_counters_ex()
    assert after["comb"] == before["comb"] + 2
    assert after["each"] == before["each"] and after["msm"] == before["msm"]  # no fallback pass
    okm, bm = m.verify_batch_keyed(keys, kidx, sigs, msgs)
    assert bm == want and not okm


def test_comb_golden_and_zip215_vectors(engs):
    """every committed vector (Appendix-B categories, the 196-case small-order table) as ONE keyed
    call over registered keys, undecodable and small-order keys included"""
    e, _, _, _, _ = engs
    vecs = [(bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"]))
            for v in of.load_golden("ed25519_vectors.json")["vectors"]]
    vecs += [(bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"]))
             for v in of.load_golden("zip215_small_order.json")["vectors"]]
    assert len(vecs) > 64
    keys = sorted({p for p, _, _ in vecs})
    kpos = {k: i for i, k in enumerate(keys)}
    e.keycache_register(keys)
    want = [of.verify(*v) for v in vecs]
    assert set(want) == {True, False}
    c0 = e.diag_counters_ex()["comb"]
    ok, bits = e.verify_batch_keyed(keys, [kpos[p] for p, _, _ in vecs], [s for _, s, _ in vecs],
                                    [x for _, _, x in vecs])
    assert bits == want and not ok
    assert e.diag_counters_ex()["comb"] == c0 + 1


def test_comb_path_selection(engs):
    e, m, a, seeds, keys = engs
    kidx, sigs, msgs = _batch(e, seeds, 100, 100)
    want = [True] * 100

    def run(eng, ks=keys, ki=kidx):
        b = eng.diag_counters_ex()
        ok, bits = eng.verify_batch_keyed(ks, ki, sigs, msgs)
        assert ok and bits == want
        c = eng.diag_counters_ex()
        return {k: c[k] - b[k] for k in c}

    assert run(e) == {"tiny": 0, "msm": 0, "each": 0, "comb": 1}
    # one key without a comb table (never registered; the call caches it itself): the whole call
    # takes the MSM
    extra_seed = random.Random(5).randbytes(32)
    extra = of.pubkey(extra_seed)
    sigs[50] = of.sign(extra_seed, msgs[50])
    d = run(e, keys + [extra], kidx[:50] + [10] + kidx[51:])
    assert d["comb"] == 0 and d["msm"] == 1
    sigs[50] = of.sign(seeds[kidx[50]], msgs[50])
    # contexts whose flags force a path never take the comb kernel
    for eng in (m, a):
        eng.set_comb_batch_max(4096)
        assert run(eng)["comb"] == 0
        assert eng.diag_counters_ex()["comb"] == 0
    try:
        e.set_comb_batch_max(99)
        assert e.comb_batch_max == 99
        d = run(e)
        assert d["comb"] == 0 and d["msm"] == 1
        e.set_comb_batch_max(100)
        assert run(e)["comb"] == 1
        e.set_comb_batch_max(0)
        assert e.comb_batch_max == 0
        d = run(e)
        assert d["comb"] == 0 and d["msm"] == 1
        # at or above the shard minimum a call splits over devices and keeps the MSM: clamped below
        e.set_comb_batch_max(10**9)
        assert 4096 < e.comb_batch_max < 10**9
        if "NWV_SHARD_MIN" not in os.environ:
            assert e.comb_batch_max == 16383
    finally:
        e.set_comb_batch_max(4096)
    assert e.comb_batch_max == 4096
    # 64 signatures stay on the one-launch path
    d = {k: -v for k, v in e.diag_counters_ex().items()}
    ok, bits = e.verify_batch_keyed(keys, kidx[:64], sigs[:64], msgs[:64])
    assert ok and all(bits)
    for k, v in e.diag_counters_ex().items():
        d[k] += v
    assert d == {"tiny": 1, "msm": 0, "each": 0, "comb": 0}
    # the three-counter call keeps its meaning
    assert e.diag_counters() == {k: v for k, v in e.diag_counters_ex().items() if k != "comb"}


def test_comb_types_layer_large_committee_certificate(engs):
    """Certificate::verify of a 100-node committee: 67 votes and the header's signature, 68
    signatures, through the fused digest-then-verify call; codes equal the oracle restatement"""
    import types_util as tu
    from types_util import nt
    from narwhal_amd import types as T
    e = engs[0]
    fx = nt.CommitteeFixture(100, of.pubkey, of.sign, seed=23)
    c = tu.committee(fx.committee)
    h = fx.header()
    q = fx.committee.quorum_threshold()
    assert q == 67
    cert = tu.oracle_certificate(fx, h, list(range(1, q + 1)))
    c0 = e.diag_counters_ex()["comb"]
    got = T.verify_certificates(e, c, [tu.certificate(cert)])
    assert got == [nt.certificate_verify(fx.committee, cert, of.verify)] == [0]
    s = cert["sigs"][40]
    bad = dict(cert, sigs=cert["sigs"][:40] + [s[:5] + bytes([s[5] ^ 2]) + s[6:]] + cert["sigs"][41:])
    got = T.verify_certificates(e, c, [tu.certificate(bad)])
    assert got == [nt.certificate_verify(fx.committee, bad, of.verify)] and got[0] != 0
    assert e.diag_counters_ex()["comb"] >= c0 + 2


def test_comb_two_threads_one_engine(engs):
    """two threads, five calls each of 300 signatures with different forged sets, on one engine:
    each call has its lane's workspace, so every call's bits are its own"""
    e, _, _, seeds, keys = engs
    jobs = []
    for t in range(2):
        kidx, sigs, msgs = _batch(e, seeds, 300, 300 + t)
        _, want = _forge_set(keys, kidx, sigs, msgs, 31 + t)
        jobs.append((kidx, sigs, msgs, want))
    assert jobs[0][3] != jobs[1][3]
    out = [[], []]

    def work(t):
        kidx, sigs, msgs, _ = jobs[t]
        for _ in range(5):
            out[t].append(e.verify_batch_keyed(keys, kidx, sigs, msgs))

    c0 = e.diag_counters_ex()["comb"]
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
    assert e.diag_counters_ex()["comb"] == c0 + 10
