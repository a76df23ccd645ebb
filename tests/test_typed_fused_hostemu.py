"""The one-launch typed path (nwv_set_typed_fused) on the host (tests/hostemu/typed_fused_hostemu.cpp):
blake2b.h's one-lane one-block BLAKE2b-256 against hashlib; the fused kernels' typed messages on the
emulated wave against the oracle, each vector once over a literal message and once over the digest
of an 80-byte preimage whose digest is that literal; and the plan nwv_types.cpp builds for the
engine in both modes, over a stub engine that records it.  The GPU kernels are checked by
tests/test_gpu_typed_fused.py."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

import oracle_ffi as of
import types_util as tu
from types_util import nt

from narwhal_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "_build", "libtypedfusedemu.so")
STORE = 0x80000000


def b2(m):
    return hashlib.blake2b(m, digest_size=32).digest()


@pytest.fixture(scope="module")
def he():
    if not os.path.exists(PATH):
        import subprocess
        subprocess.run(["make", "-C", ROOT, "tests/_build/libtypedfusedemu.so"], check=True)
    lib = ctypes.CDLL(PATH)
    vp = ctypes.c_void_p
    lib.he_b2_one_block.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
    lib.he_b2_one_block.restype = None
    lib.he_typed_verify.argtypes = [ctypes.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.he_typed_verify.restype = ctypes.c_int
    lib.he_plan.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int]
    lib.he_plan.restype = ctypes.c_int
    for name, (args, res) in T._SIGS.items():
        f = getattr(lib, name, None)
        if f is not None:
            f.argtypes, f.restype = args, res
    return lib


def one_block(he, m):
    out = ctypes.create_string_buffer(32)
    he.he_b2_one_block(bytes(m), len(m), out)
    return out.raw


def test_one_block_blake2b_matches_hashlib(he):
    rnd = random.Random(128)
    for n in (0, 1, 79, 80, 81, 127, 128):
        for m in (bytes(n), b"\xff" * n):
            assert one_block(he, m) == b2(m), n
    for _ in range(200):
        m = rnd.randbytes(rnd.choice([0, 1, 79, 80, 81, 127, 128, rnd.randint(0, 128)]))
        assert one_block(he, m) == b2(m), len(m)


def typed_verify(he, items):
    """items: (pk, sig, message bytes, src word) -> (verdicts, the stored digests' words)"""
    n = len(items)
    pk = np.frombuffer(b"".join(i[0] for i in items) + bytes(16), dtype=np.uint8)
    sg = np.frombuffer(b"".join(i[1] for i in items) + bytes(16), dtype=np.uint8)
    lens = np.array([len(i[2]) for i in items], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    arena = np.frombuffer(b"".join(i[2] for i in items) + bytes(16), dtype=np.uint8)
    src = np.array([i[3] for i in items], dtype=np.uint32)
    store = np.zeros(8 * (n + 1), dtype=np.uint32)
    out = np.full(n, 7, dtype=np.uint8)
    rc = he.he_typed_verify(n, pk.ctypes.data, sg.ctypes.data, arena.ctypes.data, offs.ctypes.data, lens.ctypes.data,
                            src.ctypes.data, store.ctypes.data, out.ctypes.data)
    assert rc == 0 and set(out.tolist()) <= {0, 1}
    return [bool(v) for v in out], store


def test_fused_check_literal_and_preimage_agree_with_the_oracle(he):
    """every golden and ZIP-215 vector's key and R, signed message replaced by a 32-byte one (the
    typed paths sign digests): the verdict over the literal, the verdict over an 80-byte preimage
    whose digest is that literal, and the oracle's must be equal; a valid signature of each kind too"""
    rnd = random.Random(215)
    vecs = [(bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]))
            for name in ("ed25519_vectors.json", "zip215_small_order.json") for v in of.load_golden(name)["vectors"]]
    assert len(vecs) > 300
    items, want = [], []
    for k, (pk, sig) in enumerate(vecs):
        pre = rnd.randbytes(80)
        items += [(pk, sig, b2(pre), 0), (pk, sig, pre, (k + 1) | STORE)]
        want += [of.verify(pk, sig, b2(pre))] * 2
    seeds = [rnd.randbytes(32) for _ in range(4)]
    for k, s in enumerate(seeds):
        pre = rnd.randbytes(80)
        sig = of.sign(s, b2(pre))
        j = len(vecs) + k
        items += [(of.pubkey(s), sig, b2(pre), 0), (of.pubkey(s), sig, pre, (j + 1) | STORE),
                  (of.pubkey(s), sig, pre[:-1] + bytes([pre[-1] ^ 1]), j + 1)]
        want += [True, True, False]
    assert set(want) == {True, False}
    got, store = typed_verify(he, items)
    assert got == want
    assert got[0:2 * len(vecs):2] == got[1:2 * len(vecs):2]  # literal and preimage: the same verdict
    # the digest a storing signature leaves for the host; a signature without the flag stores none
    words = store.tobytes()
    for k in (0, 7, len(vecs) - 1, len(vecs) + 3):
        assert words[32 * k:32 * k + 32] == b2(items[2 * k + 1][2] if k < len(vecs) else items[2 * len(vecs) + 3 * (k - len(vecs)) + 1][2])


# ---- the types layer's plan over the stub engine --------------------------------------------
class _Stub:
    _h = ctypes.c_void_p(1)


def _stand_in_sig(key, msg):
    return bytes(a ^ b for a, b in zip(msg, key)) + bytes(32)


def _fixture():
    fx = nt.CommitteeFixture(4, of.pubkey, _stand_in_sig_by_seed, seed=3)
    return fx


def _stand_in_sig_by_seed(seed, msg):
    return _stand_in_sig(of.pubkey(seed), msg)


def _plan(he):
    buf = np.zeros(4096, dtype=np.uint32)
    lits = np.zeros(4096, dtype=np.uint8)
    k = he.he_plan(buf.ctypes.data, len(buf), lits.ctypes.data, len(lits))
    p = buf[:k].tolist()
    entry, n_pre, n_lit, n = p[:4]
    pre = [(p[4 + 2 * j], p[5 + 2 * j]) for j in range(n_pre)]
    sigs = [(p[4 + 2 * n_pre + 2 * i], p[5 + 2 * n_pre + 2 * i]) for i in range(n)]
    return {"entry": entry, "pre": pre, "sigs": sigs, "lits": [lits[32 * j:32 * j + 32].tobytes() for j in range(n_lit)]}


def _items(fx):
    rnd = random.Random(12)
    c = fx.committee
    h = fx.header(author_idx=1, parents=sorted(rnd.randbytes(32) for _ in range(3)),
                  payload=[(rnd.randbytes(32), 1)])
    x = tu.oracle_certificate(fx, h, [0, 2, 3])
    return c, h, fx.votes(h)[:2], x


def test_plan_with_the_setting_off_is_the_digest_call(he):
    fx = _fixture()
    c, h, vs, x = _items(fx)
    he.he_set_typed_fused(0)
    cm, eng = tu.committee(c), _Stub()
    assert T._many(eng, he.nwv_header_verify_many, cm, [tu.header(h)]) == [0]
    p = _plan(he)
    hlen = 48 + 36 * 1 + 32 * 3
    a = c.keys.index(h["author"])
    assert p == {"entry": 0, "pre": [(hlen, 0)], "sigs": [(a, 0)], "lits": []}
    assert T._many(eng, he.nwv_vote_verify_many, cm, [tu.vote(v) for v in vs]) == [0, 0]
    p = _plan(he)
    assert p["entry"] == 0 and p["pre"] == [(80, 0), (80, 0)] and p["lits"] == []
    assert p["sigs"] == [(c.keys.index(v["author"]), k) for k, v in enumerate(vs)]
    assert T._many(eng, he.nwv_certificate_verify_many, cm, [tu.certificate(x)]) == [0]
    p = _plan(he)
    assert p["entry"] == 0 and p["pre"] == [(hlen, 0), (80, 0)] and p["lits"] == []
    assert p["sigs"] == [(a, 0)] + [(k, 1) for k in x["signed"]]


def test_plan_with_the_setting_on_is_the_typed_call(he):
    fx = _fixture()
    c, h, vs, x = _items(fx)
    he.he_set_typed_fused(1)
    cm, eng = tu.committee(c), _Stub()
    hlen = 48 + 36 * 1 + 32 * 3
    a = c.keys.index(h["author"])
    try:
        assert T._many(eng, he.nwv_header_verify_many, cm, [tu.header(h)]) == [0]
        # the header's signature over its id, a literal behind the one (side) preimage
        assert _plan(he) == {"entry": 1, "pre": [(hlen, 0)], "sigs": [(a, 1)], "lits": [h["id"]]}
        assert T._many(eng, he.nwv_vote_verify_many, cm, [tu.vote(v) for v in vs]) == [0, 0]
        p = _plan(he)
        assert p["entry"] == 1 and p["pre"] == [(80, 1), (80, 1)] and p["lits"] == []
        assert p["sigs"] == [(c.keys.index(v["author"]), k) for k, v in enumerate(vs)]
        assert T._many(eng, he.nwv_certificate_verify_many, cm, [tu.certificate(x)]) == [0]
        p = _plan(he)
        assert p["entry"] == 1 and p["pre"] == [(hlen, 0), (80, 1)] and p["lits"] == [h["id"]]
        assert p["sigs"] == [(a, 2)] + [(k, 1) for k in x["signed"]]
    finally:
        he.he_set_typed_fused(0)


@pytest.mark.parametrize("setting", [0, 1])
def test_id_digest_signature_cases_give_the_stated_codes(he, setting):
    fx = _fixture()
    c, h, vs, x = _items(fx)
    cm, eng = tu.committee(c), _Stub()
    a_seed = fx.seeds[fx.authorities.index(h["author"])]
    wrong = bytes(range(32))
    cases = [(dict(h, id=wrong, signature=_stand_in_sig_by_seed(a_seed, wrong)), nt.INVALID_HEADER_ID),
             (dict(h, id=wrong), nt.INVALID_HEADER_ID),
             (dict(h, signature=bytes(64)), nt.INVALID_SIGNATURE),
             (h, nt.OK)]
    he.he_set_typed_fused(setting)
    try:
        for hh, code in cases:
            assert nt.header_verify(c, hh, lambda pk, s, m: s == _stand_in_sig(pk, m)) == code
            assert T._many(eng, he.nwv_header_verify_many, cm, [tu.header(hh)]) == [code]
            assert T._many(eng, he.nwv_certificate_verify_many, cm, [tu.certificate(dict(x, header=hh))]) == [code]
        # a bad vote signature in the certificate, a bad vote
        bad = dict(x, sigs=[bytes(64)] + x["sigs"][1:])
        assert T._many(eng, he.nwv_certificate_verify_many, cm, [tu.certificate(bad)]) == [nt.INVALID_SIGNATURE]
        assert T._many(eng, he.nwv_vote_verify_many, cm, [tu.vote(dict(vs[0], signature=bytes(64)))]) == \
            [nt.INVALID_SIGNATURE]
        # all of them in one call: the per-item codes
        assert T._many(eng, he.nwv_header_verify_many, cm, [tu.header(hh) for hh, _ in cases]) == [k for _, k in cases]
    finally:
        he.he_set_typed_fused(0)
