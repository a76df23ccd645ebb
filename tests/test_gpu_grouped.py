"""The trait surface through nwv_ed25519_verify_batch_grouped: the fastcrypto-shaped calls
(nwv_ed25519_aggregate_verify, _aggregate_batch_verify, _verify_batch_empty_fail) name one key per
signature; the library groups them by key bytes (narwhal_amd/csrc/group_keys.h), looks the distinct
keys up in the serving device's key cache and runs keyed over the cache (one-launch / comb paths for
a registered committee), keyed and uncached, or un-keyed.  Verdicts and bad sets are the oracle's on
every path; which path ran is read from nwv_diag_counters_ex, nwv_diag_grouped and
nwv_keycache_stats as deltas around the call."""
import ctypes
import json
import os
import random
import subprocess
import sys

import pytest

import oracle_ffi as of
import zcoeff_gpu_check as zg
from narwhal_amd import _lib
from test_gpu_tiny import _forge

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
OK, BAD = _lib.NWV_OK, _lib.NWV_ERR_SIGNATURE


def _seeds(n, seed):
    rnd = random.Random(seed)
    s = [rnd.randbytes(32) for _ in range(n)]
    return s, [of.pubkey(x) for x in s]


def _sign(e, seeds, who, msgs):
    _, sg = e.sign_many([seeds[k] for k in who], msgs)
    return [sg[64 * i:64 * i + 64].tobytes() for i in range(len(msgs))]


def _grouped(e, items, seed=None, want_bits=True):
    ok, bits = e.verify_batch_grouped_arrays(*_lib.soa(items), seed=seed, want_bits=want_bits)
    return ok, (None if bits is None else [bool(b) for b in bits])


def _agg_verify(e, pks, sigs, msg, seed=None):
    return e.lib.nwv_ed25519_aggregate_verify(e._h, b"".join(sigs), len(sigs), b"".join(pks), len(pks), msg, len(msg),
                                              seed)


def _empty_fail(e, pks, sigs, msg, seed=None):
    return e.lib.nwv_ed25519_verify_batch_empty_fail(e._h, msg, len(msg), b"".join(pks), len(pks), b"".join(sigs),
                                                     len(sigs), seed)


def _agg_batch_verify(e, aggs, seed=None):
    """aggs: list of (pks, sigs, msg)"""
    arr = lambda xs: (ctypes.c_char_p * len(xs))(*xs)  # noqa: E731
    sz = lambda xs: (ctypes.c_size_t * len(xs))(*xs)  # noqa: E731
    return e.lib.nwv_ed25519_aggregate_batch_verify(
        e._h, len(aggs), arr([b"".join(s) for _, s, _ in aggs]), sz([len(s) for _, s, _ in aggs]),
        arr([b"".join(p) for p, _, _ in aggs]), sz([len(p) for p, _, _ in aggs]), arr([m for _, _, m in aggs]),
        sz([len(m) for _, _, m in aggs]), len(aggs), seed)


class Delta:
    """the counters around a call: d.ran, d.grouped, d.cache are (after - before)"""

    def __init__(self, e):
        self.e = e

    def __enter__(self):
        self.c0, self.g0, self.k0 = self.e.diag_counters_ex(), self.e.diag_grouped(), self.e.keycache_stats()
        return self

    def __exit__(self, *exc):
        c1, g1, k1 = self.e.diag_counters_ex(), self.e.diag_grouped(), self.e.keycache_stats()
        self.ran = {k: c1[k] - self.c0[k] for k in c1}
        self.grouped = {k: g1[k] - self.g0[k] for k in g1}
        self.cache = {k: k1[k] - self.k0[k] for k in k1}


def _only(**kw):
    d = {"tiny": 0, "msm": 0, "each": 0, "comb": 0}
    d.update(kw)
    return d


def _how(**kw):
    d = {"calls": 1, "cached": 0, "keyed": 0, "unkeyed": 0}
    d.update(kw)
    return d


# ---- the inputs, computed once ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    import narwhal_amd
    e = narwhal_amd.Engine(device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cert4(eng):
    """a 4-key committee and 3 of its members' signatures over one 32-byte digest"""
    seeds, keys = _seeds(4, 41)
    digest = random.Random(42).randbytes(32)
    who = [0, 2, 3]
    return keys, [keys[k] for k in who], _sign(eng, seeds, who, [digest] * 3), digest


@pytest.fixture(scope="module")
def round100(eng):
    """a 100-key committee and 3 certificates of 67 signatures each, over three digests"""
    seeds, keys = _seeds(100, 100)
    rnd = random.Random(101)
    aggs = []
    for a in range(3):
        who = sorted(rnd.sample(range(100), 67))  # committee order
        digest = rnd.randbytes(32)
        aggs.append(([keys[k] for k in who], _sign(eng, seeds, who, [digest] * 67), digest))
    return seeds, keys, aggs


@pytest.fixture(scope="module")
def strangers(eng):
    """8 unregistered keys x 40 signatures, interleaved (signature i by key i % 8)"""
    seeds, keys = _seeds(8, 8)
    rnd = random.Random(81)
    msgs = [rnd.randbytes(rnd.choice([0, 1, 32, 111, 112, 200])) for _ in range(320)]
    sigs = _sign(eng, seeds, [i % 8 for i in range(320)], msgs)
    return [(keys[i % 8], sigs[i], msgs[i]) for i in range(320)]


@pytest.fixture(scope="module")
def reg100(round100):
    """an engine with the 100-key committee registered"""
    import narwhal_amd
    e = narwhal_amd.Engine(device=0)
    e.keycache_register(round100[1])
    yield e
    e.close()


def _flat(aggs):
    return [(p, s, m) for pks, sigs, m in aggs for p, s in zip(pks, sigs)]


def _forged_items(items, bad):
    items = list(items)
    for j, i in enumerate(bad):
        p, s, m = items[i]
        s, m = _forge(s, m, j % 4)
        items[i] = (p, s, m)
    want = [of.verify(*it) for it in items]
    assert [i for i, w in enumerate(want) if not w] == sorted(bad)  # (a condition on the inputs)
    return items, want


# ---- 1: a registered 4-key committee's certificate takes the one-launch path --------------------
def test_registered_certificate_takes_the_one_launch_path(cert4):
    import narwhal_amd
    keys, pks, sigs, digest = cert4
    e = narwhal_amd.Engine(device=0)
    try:
        e.keycache_register(keys)
        with Delta(e) as d:
            assert _agg_verify(e, pks, sigs, digest) == OK
        assert d.ran == _only(tiny=1)  # k_ed_tiny, and no MSM
        assert d.grouped == _how(cached=1)
        assert d.cache["used"] == 0 and d.cache["comb_used"] == 0
        with Delta(e) as d:
            assert _empty_fail(e, pks, sigs, digest) == OK
        assert d.ran == _only(tiny=1) and d.grouped == _how(cached=1)
        zeroed = [sigs[0], bytes(64), sigs[2]]
        assert not of.verify(pks[1], zeroed[1], digest)
        with Delta(e) as d:
            assert _agg_verify(e, pks, zeroed, digest) == BAD
        assert d.ran == _only(tiny=1)
        assert _empty_fail(e, pks, zeroed, digest) == BAD
        # the same key twice in one aggregate (two entries of one group)
        assert _agg_verify(e, [pks[0], pks[0], pks[2]], [sigs[0], sigs[0], sigs[2]], digest) == OK
        assert _agg_verify(e, [pks[0], pks[0], pks[2]], [sigs[0], sigs[1], sigs[2]], digest) == BAD
    finally:
        e.close()


# ---- 2: a round's certificates of a registered 100-key committee take the comb kernel -----------
def test_registered_round_takes_the_comb_kernel(reg100, round100):
    e = reg100
    _, _, aggs = round100
    with Delta(e) as d:
        assert _agg_batch_verify(e, aggs) == OK
    assert d.ran == _only(comb=1)
    assert d.grouped == _how(cached=1)
    # one certificate of 67 > 64 signatures: the comb kernel as well
    with Delta(e) as d:
        assert _agg_verify(e, *aggs[1]) == OK
    assert d.ran == _only(comb=1)
    items, want = _forged_items(_flat(aggs), [67 + 33])
    forged = [aggs[0], (aggs[1][0], [s for _, s, _ in items[67:134]], aggs[1][2]), aggs[2]]
    assert forged[1][1][33] != aggs[1][1][33]
    with Delta(e) as d:
        assert _agg_batch_verify(e, forged) == BAD
    assert d.ran == _only(comb=1)
    with Delta(e) as d:
        ok, bits = _grouped(e, items)
    assert not ok and bits == want
    assert d.ran == _only(comb=1) and d.grouped == _how(cached=1)
    ok, bits = _grouped(e, _flat(aggs))
    assert ok and all(bits) and len(bits) == 201


# ---- 3: unregistered keys that repeat run keyed and uncached ------------------------------------
def test_repeating_strangers_run_keyed_uncached(eng, strangers):
    with Delta(eng) as d:
        ok, bits = _grouped(eng, strangers)
    assert ok and all(bits) and len(bits) == 320
    assert d.grouped == _how(keyed=1)
    assert d.ran == _only(msm=1)
    assert d.cache == {"used": 0, "cap": 0, "comb_used": 0, "comb_cap": 0}  # took no slot
    ok, none = _grouped(eng, strangers, want_bits=False)
    assert ok and none is None
    items, want = _forged_items(strangers, [0, 63, 64, 319])
    with Delta(eng) as d:
        ok, bits = _grouped(eng, items)
    assert not ok and bits == want
    assert d.grouped == _how(keyed=1)
    ok, _ = _grouped(eng, items, want_bits=False)
    assert not ok


# ---- 4: distinct strangers fall through to the un-keyed path ------------------------------------
def test_distinct_strangers_run_unkeyed(eng):
    seeds, keys = _seeds(130, 130)
    msgs = [b"m%d" % i for i in range(130)]
    sigs = _sign(eng, seeds, list(range(130)), msgs)
    items = list(zip(keys, sigs, msgs))
    with Delta(eng) as d:
        ok, bits = _grouped(eng, items)
    assert d.grouped == _how(unkeyed=1) and d.ran == _only(msm=1)
    assert (ok, bits) == eng.verify_batch(items) == (True, [True] * 130)
    bad, want = _forged_items(items, [0, 64, 129])
    with Delta(eng) as d:
        ok, bits = _grouped(eng, bad)
    assert d.grouped == _how(unkeyed=1)
    assert (ok, bits) == eng.verify_batch(bad) == (False, want)
    # 129 distinct keys of 258 signatures is the last size that still groups
    two = items[:129] * 2
    with Delta(eng) as d:
        ok, bits = _grouped(eng, two)
    assert ok and all(bits) and d.grouped == _how(keyed=1)
    with Delta(eng) as d:
        ok, bits = _grouped(eng, two[:257])
    assert ok and all(bits) and d.grouped == _how(unkeyed=1)


# ---- 5: one stranger among registered keys: lookup only, no slot taken --------------------------
def test_one_stranger_among_registered_keys(reg100, round100):
    e = reg100
    _, _, aggs = round100
    seeds, keys = _seeds(1, 555)
    msg = b"a stranger's message"
    items = _flat(aggs)
    items.insert(100, (keys[0], _sign(e, seeds, [0], [msg])[0], msg))
    with Delta(e) as d:
        ok, bits = _grouped(e, items)
    assert ok and all(bits) and len(bits) == 202
    assert d.cache["used"] == 0 and d.cache["comb_used"] == 0
    assert d.grouped == _how(keyed=1)  # not from the cache
    assert d.ran == _only(msm=1)
    bad, want = _forged_items(items, [100])
    with Delta(e) as d:
        ok, bits = _grouped(e, bad)
    assert not ok and bits == want
    assert d.cache["used"] == 0 and d.cache["comb_used"] == 0 and d.grouped["cached"] == 0
    # and through the trait call, the stranger's signature in the first aggregate
    mixed = [(aggs[0][0] + [keys[0]], aggs[0][1] + [_sign(e, seeds, [0], [aggs[0][2]])[0]], aggs[0][2]), aggs[1],
             aggs[2]]  # (at most 101 distinct keys of 202 signatures)
    with Delta(e) as d:
        assert _agg_batch_verify(e, mixed) == OK
    assert d.cache["used"] == 0 and d.grouped == _how(keyed=1)


# ---- 6: byte equality: several encodings of one point are several keys --------------------------
@pytest.fixture(scope="module")
def golden():
    out = {}
    for name in ("zip215_small_order.json", "ed25519_vectors.json"):
        vecs = [(bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"]))
                for v in of.load_golden(name)["vectors"]]
        out[name] = (vecs, [of.verify(*v) for v in vecs])
    assert len(out["zip215_small_order.json"][0]) == 196
    return out


@pytest.mark.parametrize("registered", [False, True], ids=["unregistered", "registered"])
@pytest.mark.parametrize("name", ["zip215_small_order.json", "ed25519_vectors.json"])
def test_golden_vectors_as_one_batch_and_alone(golden, name, registered):
    import narwhal_amd
    vecs, want = golden[name]
    assert len(vecs) <= 4096
    e = narwhal_amd.Engine(device=0)
    try:
        if registered:
            e.keycache_register(sorted({p for p, _, _ in vecs}))
        with Delta(e) as d:
            ok, bits = _grouped(e, vecs)
        assert bits == want and ok == all(want)
        assert d.grouped["cached"] == (1 if registered else 0)
        assert d.cache["used"] == 0
        alone = []
        for v in vecs:
            ok, b = _grouped(e, [v])
            assert ok == b[0]
            alone.append(ok)
        assert alone == want
        assert [_agg_verify(e, [p], [s], m) == OK for p, s, m in vecs] == want
    finally:
        e.close()


# ---- 7: the coefficients belong to the caller's signature index ---------------------------------
@pytest.mark.parametrize("n,m,how", [(300, 20, "keyed"), (300, 200, "unkeyed")])
def test_coefficients_under_grouping(n, m, how):
    """a cancelling set (tests/zcoeff.py) over signatures that share keys is accepted under the
    construction's seed only -- grouping did not renumber z_i -- and nwv_ed25519_verify_batch_keyed
    says the same on the same inputs"""
    import narwhal_amd
    e = narwhal_amd.Engine(device=0)
    try:
        keys, kidx, sigs, msgs = zg.signed(e, n, m, 70 + m)
        pks = [keys[k] for k in kidx]
        items = lambda f: list(zip(pks, f, msgs))  # noqa: E731

        def run(s, seed, want_bits):
            return _grouped(e, items(s), seed=seed, want_bits=want_bits)

        def checks(r):
            assert r["valid_accepts"] and r["touched_differ"] and r["oracle_rejects_touched"], r
            assert r["seed_accepts_nobits"] and r["seed_accepts_bits"] and r["no_fallback"], r
            assert r["other_rejects_nobits"] and r["other_rejects_bits"], r
            assert r["path_ran"] and r["runs"]["tiny"] == 0 and r["runs"]["comb"] == 0, r["runs"]
            assert r["n"] == r["touched"] == n

        g0 = e.diag_grouped()
        checks(zg.three_checks(e, run, items, sigs))
        g1 = e.diag_grouped()
        assert {k: g1[k] - g0[k] for k in g1} == _how(calls=5, **{how: 5})
        # positions that share keys only: two signatures of each of the first five keys
        P = [k + m * j for k in range(5) for j in range(2)] if m == 20 else [k + 200 * j for k in range(5) for j in range(2)]
        assert all(kidx[P[2 * k]] == kidx[P[2 * k + 1]] for k in range(5))
        r = zg.three_checks(e, run, items, sigs, P=P, tag=1)
        assert r["touched"] == 10 and r["seed_accepts_nobits"] and r["seed_accepts_bits"] and r["other_rejects_bits"], r
        # the keyed call on the same inputs (it fills the cache with these keys) ...
        checks(zg.three_checks(e, zg.keyed_run(e, keys, kidx, msgs), items, sigs))
        # ... after which the grouped call finds every key cached and runs the 128-bit MSM
        g1 = e.diag_grouped()
        checks(zg.three_checks(e, run, items, sigs))
        g2 = e.diag_grouped()
        assert {k: g2[k] - g1[k] for k in g2} == _how(calls=5, cached=5)
    finally:
        e.close()


# ---- 8: flags and epochs ------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["NWV_FLAG_NO_KEYCACHE", "NWV_FLAG_MSM_NEVER"])
def test_flags_keep_the_verdicts(cert4, strangers, flag):
    import narwhal_amd
    keys, pks, sigs, digest = cert4
    e = narwhal_amd.Engine(device=0, flags=getattr(_lib, flag))
    try:
        e.keycache_register(keys)
        never = flag == "NWV_FLAG_MSM_NEVER"
        with Delta(e) as d:
            assert _agg_verify(e, pks, sigs, digest) == OK
        assert d.ran["tiny"] == 0 and d.ran["comb"] == 0
        assert d.ran == (_only(each=1) if never else _only(msm=1))
        assert d.grouped == _how(unkeyed=1)  # MSM_NEVER passes through; 3 uncached keys of 3 group nothing
        assert _agg_verify(e, pks, [sigs[0], bytes(64), sigs[2]], digest) == BAD
        with Delta(e) as d:
            ok, bits = _grouped(e, strangers)
        assert ok and all(bits)
        assert d.grouped == (_how(unkeyed=1) if never else _how(keyed=1))
        items, want = _forged_items(strangers, [0, 63, 64, 319])
        ok, bits = _grouped(e, items)
        assert not ok and bits == want
    finally:
        e.close()


def test_retired_committee_takes_the_msm(cert4):
    import narwhal_amd
    keys, pks, sigs, digest = cert4
    e = narwhal_amd.Engine(device=0)
    try:
        e.keycache_register(keys)
        with Delta(e) as d:
            assert _agg_verify(e, pks, sigs, digest) == OK
        assert d.ran == _only(tiny=1)
        e.keycache_retain([])
        with Delta(e) as d:
            assert _agg_verify(e, pks, sigs, digest) == OK
        assert d.ran == _only(msm=1) and d.grouped["cached"] == 0
        assert _agg_verify(e, pks, [sigs[0], bytes(64), sigs[2]], digest) == BAD
        e.keycache_register(keys)  # the next epoch registers again
        with Delta(e) as d:
            assert _agg_verify(e, pks, sigs, digest) == OK
        assert d.ran == _only(tiny=1)
    finally:
        e.close()


# ---- 9: NWV_GROUP_MAX_N ---------------------------------------------------------------------------
def test_group_max_n_passes_larger_calls_through():
    env = dict(os.environ, NWV_GROUP_MAX_N="64")
    p = subprocess.run([sys.executable, os.path.join(HERE, "grouped_gpu_check.py"), "--sizes", "65,64"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    for n in ("65", "64"):
        assert out[n]["ok"] and out[n]["bad_rejected"] and out[n]["bad_bits_are_the_oracles"], out[n]
    assert out["65"]["delta"] == _how(unkeyed=1)
    assert out["64"]["delta"] == _how(keyed=1)


# ---- 10: the empty batch ---------------------------------------------------------------------------
def test_empty_batch(eng):
    allv = ctypes.c_int(0)
    with Delta(eng) as d:
        ok, bits = _grouped(eng, [])
        rc = eng.lib.nwv_ed25519_verify_batch_grouped(eng._h, 0, None, None, None, None, None, None,
                                                      ctypes.byref(allv), None)
        # the trait calls' own early returns are where they were
        assert eng.lib.nwv_ed25519_aggregate_verify(eng._h, None, 0, None, 0, b"x", 1, None) == OK
        assert eng.lib.nwv_ed25519_verify_batch_empty_fail(eng._h, b"x", 1, None, 0, None, 0, None) == _lib.NWV_ERR_EMPTY
        assert eng.lib.nwv_ed25519_aggregate_verify(eng._h, bytes(64), 1, bytes(64), 2, b"x", 1, None) == \
            _lib.NWV_ERR_LENGTH
    assert ok is True and bits == []
    assert rc == OK and allv.value == 1
    assert d.grouped == _how(calls=0) and d.ran == _only()
