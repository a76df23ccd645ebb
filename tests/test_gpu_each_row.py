"""The row kernel for small per-signature passes over keys without a comb table
(narwhal_amd/csrc/each_kernels.hip k_ed_each_row): nwv_ed25519_verify_each, and the pass that names
the bad set after a batch MSM rejects, of at most each_row_max signatures run in one launch, one
workgroup a signature.  Its verdict bits must equal the oracle's ZIP-215 verdicts and those of the
lane pipeline (NWV_FLAG_NO_EACH_ROW) at sizes on both sides of a verdict word and off every
multiple, on forgeries of every kind, on every golden / ZIP-215 vector, after rejected batches
(un-keyed, keyed, grouped; the reuse form that loads the MSM's records and, under
NWV_FLAG_NO_MSM_REUSE, the plain form, told apart by nwv_diag_each_row_reuse), from two threads at
once and on a three-replica context (child script tests/each_row_gpu_check.py); nwv_diag_each_row and
the per-signature counter say which path ran."""
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
from test_gpu_comb import MSG_LENS
from test_gpu_tiny import _forge

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
P_FIELD = 2**255 - 19


@pytest.fixture(scope="module")
def engs():
    import narwhal_amd
    e = narwhal_amd.Engine(device=0)
    e.set_each_row_max(4096)
    l = narwhal_amd.Engine(device=0, flags=_lib.NWV_FLAG_NO_EACH_ROW)
    l.set_each_row_max(4096)
    yield e, l
    e.close()
    l.close()


def _items(e, n, seed, nkeys=None):
    """n valid signatures by unregistered random keys -> [(pk, sig, msg)]"""
    rnd = random.Random(seed)
    seeds = [rnd.randbytes(32) for _ in range(nkeys or n)]
    use = [seeds[rnd.randrange(len(seeds))] if nkeys else seeds[i] for i in range(n)]
    msgs = [rnd.randbytes(rnd.choice(MSG_LENS)) for _ in range(n)]
    pk, sg = e.sign_many(use, msgs)
    return [(pk[32 * i:32 * i + 32].tobytes(), sg[64 * i:64 * i + 64].tobytes(), msgs[i]) for i in range(n)]


def _forge_set(items, seed, kinds=(0, 1, 2, 3)):
    """forge indices {0, 63, 64, n - 1} (those inside the batch) and n // 7 others, the kinds in
    turn -> (forged indices, oracle verdicts); the oracle's bad set must be the injected one"""
    n = len(items)
    rnd = random.Random(seed)
    fixed = {i for i in (0, 63, 64, n - 1) if 0 <= i < n}
    bad = sorted(fixed | set(rnd.sample([i for i in range(n) if i not in fixed], n // 7)))
    for j, i in enumerate(bad):
        p, s, m = items[i]
        s, m = _forge(s, m, kinds[j % len(kinds)])
        items[i] = (p, s, m)
    want = [of.verify(*it) for it in items]
    assert [i for i, w in enumerate(want) if not w] == bad  # (a condition on the inputs)
    return bad, want


def _undecodable(rnd):
    """32 bytes that are no point encoding: (y^2 - 1) / (d y^2 + 1) is a non-square"""
    d = -121665 * pow(121666, -1, P_FIELD) % P_FIELD
    while True:
        y = rnd.randrange(P_FIELD)
        x2 = (y * y - 1) * pow(d * y * y + 1, -1, P_FIELD) % P_FIELD
        if x2 and pow(x2, (P_FIELD - 1) // 2, P_FIELD) != 1:
            return y.to_bytes(32, "little")


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 200])
def test_verify_each_sizes_and_forgeries_match_oracle(engs, n):
    e, l = engs
    items = _items(e, n, n)
    r0, c0 = e.diag_each_row(), e.diag_counters_ex()
    assert e.verify_each(items) == [True] * n
    r1, c1 = e.diag_each_row(), e.diag_counters_ex()
    assert r1 == (r0[0] + 1, r0[1] + n)  # the row kernel ran, as one per-signature pass
    assert c1 == dict(c0, each=c0["each"] + 1)
    _, want = _forge_set(items, 7 * n)
    assert e.verify_each(items) == want
    assert e.diag_each_row() == (r1[0] + 1, r1[1] + n)
    assert l.verify_each(items) == want
    assert l.diag_each_row() == (0, 0)


def test_golden_and_zip215_vectors(engs):
    """every committed vector (Appendix-B categories, the 196-case small-order table) in ONE call"""
    e, _ = engs
    g = of.load_golden("ed25519_vectors.json")["vectors"]
    z = of.load_golden("zip215_small_order.json")["vectors"]
    vecs = [(bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"])) for v in g + z]
    want = [v["expect"] for v in g + z]  # the recorded verdicts
    assert want == [of.verify(*v) for v in vecs] and set(want) == {True, False} and all(want[len(g):])
    r0 = e.diag_each_row()
    assert e.verify_each(vecs) == want
    assert e.diag_each_row() == (r0[0] + 1, r0[1] + len(vecs))


@pytest.mark.parametrize("flags", [0, _lib.NWV_FLAG_NO_MSM_REUSE])
def test_rejected_batch_names_the_bad_set(engs, flags):
    """verify_batch with verdict bits: the MSM rejects (every forgery decodes) and the pass that
    names the bad set is the row kernel; then one undecodable R, which rejects before the MSM.
    By default the pass is the reuse form (k_ed_each_row_msm: the MSM's records, k and flags);
    with NWV_FLAG_NO_MSM_REUSE the plain form, which decompresses and hashes again"""
    reuse = 0 if flags else 1
    import narwhal_amd
    e = engs[0]
    if flags:
        e = narwhal_amd.Engine(device=0, flags=flags)
        e.set_each_row_max(4096)
    try:
        items = _items(e, 130, 130)
        for j, i in enumerate((63, 64, 129)):
            p, s, m = items[i]
            s, m = _forge(s, m, 1 + j % 2)  # s, or the message: R and A still decode
            items[i] = (p, s, m)
        want = [of.verify(*it) for it in items]
        assert [i for i, w in enumerate(want) if not w] == [63, 64, 129]
        r0, c0, u0 = e.diag_each_row(), e.diag_counters_ex(), e.diag_each_row_reuse()
        ok, bits = e.verify_batch(items)
        assert bits == want and not ok
        c1 = e.diag_counters_ex()
        assert e.diag_each_row() == (r0[0] + 1, r0[1] + 130)
        assert e.diag_each_row_reuse() == u0 + reuse
        assert c1["msm"] == c0["msm"] + 1 and c1["each"] == c0["each"] + 1
        p, s, m = items[7]
        items[7] = (p, _undecodable(random.Random(5)) + s[32:], m)
        want[7] = False
        assert not of.verify(*items[7])
        ok, bits = e.verify_batch(items)
        assert bits == want and not ok
        assert e.diag_each_row() == (r0[0] + 2, r0[1] + 260)
        assert e.diag_each_row_reuse() == u0 + 2 * reuse
        # verify_each has no MSM before it: always the plain form
        assert e.verify_each(items) == want
        assert e.diag_each_row_reuse() == u0 + 2 * reuse
    finally:
        if flags:
            e.close()


def test_path_selection(engs):
    import narwhal_amd
    e, l = engs
    items = _items(e, 129, 129)
    a = narwhal_amd.Engine(device=0, flags=_lib.NWV_FLAG_MSM_ALWAYS)
    a.set_each_row_max(4096)

    def rows(eng, k):
        r0, c0 = eng.diag_each_row(), eng.diag_counters()["each"]
        assert eng.verify_each(items[:k]) == [True] * k
        r1 = eng.diag_each_row()
        return r1[0] - r0[0], r1[1] - r0[1]

    try:
        e.set_each_row_max(128)
        assert e.each_row_max == 128
        assert rows(e, 128) == (1, 128)
        assert rows(e, 129) == (0, 0)
        e.set_each_row_max(0)
        assert e.each_row_max == 0
        assert rows(e, 1) == (0, 0) and rows(e, 128) == (0, 0)
        # at or above the shard minimum a call splits over devices: clamped to just below it
        e.set_each_row_max(10**9)
        assert 4096 < e.each_row_max < 10**9
        if "NWV_SHARD_MIN" not in os.environ:
            assert e.each_row_max == 16383
    finally:
        e.set_each_row_max(4096)
    assert e.each_row_max == 4096 and rows(e, 129) == (1, 129)
    # contexts whose flags keep the lane pipeline
    for eng in (l, a):
        assert eng.each_row_max == 4096
        assert rows(eng, 100) == (0, 0) and eng.diag_each_row() == (0, 0)
    a.close()
    # a staged batch run in per-signature mode keeps the lane pipeline
    pk, sig, arena, offs, lens = _lib.soa(items[:100])
    r0 = e.diag_each_row()
    st = e.stage(pk, sig, arena, offs, lens)
    try:
        st.run(0)
        st.sync()
        ok, bits = st.fetch()
        assert ok and bits.all()
    finally:
        st.free()
    assert e.diag_each_row() == r0


def test_keyed_and_grouped_fallback(engs):
    """100 signatures over 5 unregistered keys, one forgery: the keyed call and the grouped call
    name exactly it, through the row kernel"""
    e, _ = engs
    items = _items(e, 100, 500, nkeys=5)
    p, s, m = items[41]
    items[41] = (p,) + _forge(s, m, 1)
    want = [of.verify(*it) for it in items]
    assert [i for i, w in enumerate(want) if not w] == [41]
    keys = sorted({p for p, _, _ in items})
    assert len(keys) == 5
    kpos = {k: i for i, k in enumerate(keys)}
    r0, u0 = e.diag_each_row(), e.diag_each_row_reuse()
    ok, bits = e.verify_batch_keyed(keys, [kpos[p] for p, _, _ in items], [s for _, s, _ in items],
                                    [x for _, _, x in items])
    assert bits == want and not ok
    assert e.diag_each_row() == (r0[0] + 1, r0[1] + 100)
    ok, gbits = e.verify_batch_grouped_arrays(*_lib.soa(items))
    assert list(gbits) == want and not ok
    assert e.diag_each_row() == (r0[0] + 2, r0[1] + 200)
    assert e.diag_each_row_reuse() == u0  # a keyed MSM has one record a key, not one a signature


def test_two_threads_one_engine(engs):
    """two threads, 20 calls each of 100 signatures with different forged sets, on one engine"""
    e, _ = engs
    jobs = []
    for t in range(2):
        items = _items(e, 100, 900 + t)
        _, want = _forge_set(items, 77 + t)
        jobs.append((items, want))
    assert jobs[0][1] != jobs[1][1]
    out = [[], []]

    def work(t):
        for _ in range(20):
            out[t].append(e.verify_each(jobs[t][0]))

    r0 = e.diag_each_row()
    th = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=60)
    assert not any(x.is_alive() for x in th)
    for t in range(2):
        assert len(out[t]) == 20 and all(b == jobs[t][1] for b in out[t])
    assert e.diag_each_row() == (r0[0] + 40, r0[1] + 4000)


def test_three_replicas():
    """NWV_DEVICE_REPLICAS=3 (read at nwv_init: a child process): 200 signatures take the row
    kernel on one device, 40,000 split over the devices and do not; both match the oracle"""
    env = dict(os.environ, NWV_DEVICE_REPLICAS="3")
    p = subprocess.run([sys.executable, os.path.join(HERE, "each_row_gpu_check.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    assert out["devices"] == 3
    assert out["small_equal"] and out["small_bad"] > 0
    assert out["small_rows"] == [1, 200] and sorted(out["small_each_by_device"]) == [0, 0, 1]
    assert out["large_equal"] and out["large_bad"] > 0
    assert out["large_ranges"] > 1 and out["large_rows"] == [0, 0]
