"""The comb kernel's per-signature arithmetic (narwhal_amd/csrc/comb_kernels.hip k_ed_comb, lane
functions in comb.h) run on the host (tests/hostemu/comb_hostemu.cpp), workgroup by workgroup as
the kernel lays it out: COMB_G signatures hashed side by side, their R's decompressed one per
16-lane row of one emulated wave, each signature's comb terms summed in the kernel's tree order.
Verdicts against the oracle's ZIP-215 verdicts and against the one-launch path's emulation
(he_tiny_verify).  The GPU kernel is checked by tests/test_gpu_comb.py."""
import ctypes
import os
import random

import numpy as np
import pytest

import oracle_ffi as of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CE_PATH = os.path.join(ROOT, "tests", "_build", "libcombemu.so")
HE_PATH = os.path.join(ROOT, "tests", "_build", "libhostemu.so")
L_ORDER = 2**252 + 27742317777372353535851937790883648493


@pytest.fixture(scope="module")
def ce():
    if not (os.path.exists(CE_PATH) and os.path.exists(HE_PATH)):
        import subprocess
        subprocess.run(["make", "-C", ROOT, "hostemu"], check=True)
    lib = ctypes.CDLL(CE_PATH)
    vp = ctypes.c_void_p
    lib.he_comb_verify.argtypes = [ctypes.c_uint32, vp, vp, vp, vp, vp, vp]
    lib.he_comb_verify.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def he():
    lib = ctypes.CDLL(HE_PATH)
    lib.he_tiny_verify.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32]
    return lib


def comb_verify(ce, items):
    n = len(items)
    pk = np.frombuffer(b"".join(p for p, _, _ in items) + b"\0" * 16, dtype=np.uint8)
    sg = np.frombuffer(b"".join(s for _, s, _ in items) + b"\0" * 16, dtype=np.uint8)
    msgs = [m for _, _, m in items]
    lens = np.array([len(m) for m in msgs], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    arena = np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8)
    out = np.full(n, 7, dtype=np.uint8)
    rc = ce.he_comb_verify(n, pk.ctypes.data, sg.ctypes.data, arena.ctypes.data, offs.ctypes.data,
                           lens.ctypes.data, out.ctypes.data)
    assert rc == 0
    assert set(out.tolist()) <= {0, 1}
    return [bool(v) for v in out]


def _vectors():
    vecs = [(bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"]))
            for v in of.load_golden("ed25519_vectors.json")["vectors"]]
    vecs += [(bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"]))
             for v in of.load_golden("zip215_small_order.json")["vectors"]]
    return vecs


def _forge(sig, msg, kind):
    s = bytearray(sig)
    if kind == 0:
        s[3] ^= 0x10  # R
    elif kind == 1:
        s[40] ^= 0x01  # s
    elif kind == 2:
        msg = bytes([msg[0] ^ 0x80]) + msg[1:] if msg else b"\x01"
    else:
        v = int.from_bytes(bytes(s[32:]), "little") + L_ORDER  # s + l
        s[32:] = v.to_bytes(32, "little")
    return bytes(s), msg


def test_comb_emulation_matches_oracle_on_every_vector(ce):
    """every golden vector (every Appendix-B category) and the 196-case small-order table as ONE
    batch, so neighbouring rows of the decompression wave hold unrelated, partly undecodable R's;
    undecodable keys (the identity's table) and s >= l included"""
    vecs = _vectors()
    want = [of.verify(*v) for v in vecs]
    assert set(want) == {True, False} and len(vecs) > 300
    got = comb_verify(ce, vecs)
    bad = [(p.hex(), s.hex()) for (p, s, _), g, w in zip(vecs, got, want) if g != w]
    assert not bad, bad[:3]


def test_comb_emulation_random_batch_with_forgeries(ce, he):
    """70 signatures by a 10-key committee (not a multiple of the workgroup's four), message lengths
    on both sides of SHA-512's padding boundaries, one forgery of each kind and more; the
    one-launch path's emulation must agree signature by signature"""
    rnd = random.Random(70)
    seeds = [rnd.randbytes(32) for _ in range(10)]
    keys = [of.pubkey(s) for s in seeds]
    n = 70
    items = []
    for i in range(n):
        k = rnd.randrange(10)
        m = rnd.randbytes(rnd.choice([0, 1, 32, 47, 48, 111, 112, 200, 512]))
        items.append((keys[k], of.sign(seeds[k], m), m))
    assert all(comb_verify(ce, items))
    bad = sorted(set([0, 63, 64, n - 1] + rnd.sample(range(n), 8)))
    for j, i in enumerate(bad):
        s, m = _forge(items[i][1], items[i][2], j % 4)
        items[i] = (items[i][0], s, m)
    want = [of.verify(*it) for it in items]
    assert [i for i, w in enumerate(want) if not w] == bad
    assert comb_verify(ce, items) == want
    for i in bad + [1, 2, 3]:
        p, s, m = items[i]
        assert he.he_tiny_verify(p, s, m, len(m)) == int(want[i])


def test_comb_emulation_agrees_with_tiny_emulation_on_vectors(ce, he):
    """the comb layout and the one-launch layout are the same check: equal verdicts on a spread
    of the committed vectors, rejected ones included"""
    vecs = _vectors()
    pick = vecs[::9]
    got = comb_verify(ce, pick)
    tiny = [he.he_tiny_verify(p, s, m, len(m)) for p, s, m in pick]
    assert set(tiny) == {0, 1}
    assert [int(g) for g in got] == tiny
