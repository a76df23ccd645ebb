"""The row kernel's per-signature arithmetic (narwhal_amd/csrc/each_kernels.hip k_ed_each_row,
functions in each.h) run on the host (tests/hostemu/each_row_hostemu.cpp) on the emulated wave of
fe_row.h, every limb bound checked (NWV_BOUNDS_CHECK): R and A decompressed side by side on rows,
the tables 0..8 R and 0..8 A in cached row form, the Straus pass over the 33 digit positions of
the half-size scalars, [w]B from B's comb, the identity test; and the reuse form, which takes the
records, k and flags a batch MSM's prep leaves.  Tables against build_a_table entry
by entry, negated entries for every digit, verdicts against lane_straus_check_half (the lane
pipeline's emulation) and the oracle's ZIP-215 verdicts.  The GPU kernel is checked by
tests/test_gpu_each_row.py."""
import ctypes
import os
import random

import numpy as np
import pytest

import oracle_ffi as of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EE_PATH = os.path.join(ROOT, "tests", "_build", "libeachemu.so")
L_ORDER = 2**252 + 27742317777372353535851937790883648493
P_FIELD = 2**255 - 19


@pytest.fixture(scope="module")
def ee():
    if not os.path.exists(EE_PATH):
        import subprocess
        subprocess.run(["make", "-C", ROOT, "tests/_build/libeachemu.so"], check=True)
    lib = ctypes.CDLL(EE_PATH)
    vp = ctypes.c_void_p
    lib.he_each_verify.argtypes = [ctypes.c_uint32, vp, vp, vp, vp, vp, vp]
    lib.he_each_verify_msm.argtypes = [ctypes.c_uint32, vp, vp, vp, vp, vp, vp]
    lib.he_each_lane_verify.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32]
    lib.he_each_table_check.argtypes = [ctypes.c_char_p]
    lib.he_each_forced_k.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, vp]
    return lib


def each_verify(ee, items, reuse=False):
    """the plain form, or (reuse) the form that loads a batch MSM's records, k and flags"""
    n = len(items)
    pk = np.frombuffer(b"".join(p for p, _, _ in items) + b"\0" * 16, dtype=np.uint8)
    sg = np.frombuffer(b"".join(s for _, s, _ in items) + b"\0" * 16, dtype=np.uint8)
    msgs = [m for _, _, m in items]
    lens = np.array([len(m) for m in msgs], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    arena = np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8)
    out = np.full(n, 7, dtype=np.uint8)
    fn = ee.he_each_verify_msm if reuse else ee.he_each_verify
    rc = fn(n, pk.ctypes.data, sg.ctypes.data, arena.ctypes.data, offs.ctypes.data, lens.ctypes.data, out.ctypes.data)
    assert rc == 0
    assert set(out.tolist()) <= {0, 1}
    return [bool(v) for v in out]


def lane_verify(ee, items):
    return [bool(ee.he_each_lane_verify(p, s, m, len(m))) for p, s, m in items]


def _vectors():
    vecs = [(bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"]))
            for v in of.load_golden("ed25519_vectors.json")["vectors"]]
    vecs += [(bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"]))
             for v in of.load_golden("zip215_small_order.json")["vectors"]]
    return vecs


def _undecodable(rnd):
    """a 32-byte string that is no point encoding: y with (y^2 - 1) / (d y^2 + 1) a non-square"""
    d = -121665 * pow(121666, -1, P_FIELD) % P_FIELD
    while True:
        y = rnd.randrange(P_FIELD)
        x2 = (y * y - 1) * pow(d * y * y + 1, -1, P_FIELD) % P_FIELD
        if x2 and pow(x2, (P_FIELD - 1) // 2, P_FIELD) != 1:
            return y.to_bytes(32, "little")


def test_tables_match_build_a_table_and_negated_entries(ee):
    """entries 0..8 of the row table are the points of build_a_table's, and every digit -8..8
    loads the entry the lane code's conditional negation gives; keys, R's, small-order points"""
    rnd = random.Random(9)
    encs = [of.pubkey(rnd.randbytes(32)) for _ in range(4)]
    encs += [of.sign(rnd.randbytes(32), b"m")[:32] for _ in range(2)]
    encs += [bytes.fromhex(v["pk"]) for v in of.load_golden("zip215_small_order.json")["vectors"][::14]]
    decoded = 0
    for e in encs:
        r = ee.he_each_table_check(e)
        assert r in (0, -1), (e.hex(), r)
        decoded += r == 0
    assert decoded >= 8
    assert ee.he_each_table_check(_undecodable(rnd)) == -1


def test_every_vector_matches_oracle_and_lane_form(ee):
    """every golden vector (every Appendix-B category) and the 196-case small-order table"""
    vecs = _vectors()
    want = [of.verify(*v) for v in vecs]
    assert set(want) == {True, False} and len(vecs) > 300
    for reuse in (False, True):
        got = each_verify(ee, vecs, reuse)
        bad = [(p.hex(), s.hex()) for (p, s, _), g, w in zip(vecs, got, want) if g != w]
        assert not bad, (reuse, bad[:3])
    assert lane_verify(ee, vecs) == want


def test_undecodable_points_and_s_at_the_order(ee):
    rnd = random.Random(11)
    seed = rnd.randbytes(32)
    pk, m = of.pubkey(seed), b"edge"
    sig = of.sign(seed, m)
    junk = _undecodable(rnd)
    s = int.from_bytes(sig[32:], "little")
    items = [(pk, sig, m),
             (pk, junk + sig[32:], m),                                   # R does not decode
             (junk, sig, m),                                             # A does not decode
             (junk, junk + sig[32:], m),
             (pk, sig[:32] + L_ORDER.to_bytes(32, "little"), m),         # s = l
             (pk, sig[:32] + (L_ORDER - 1).to_bytes(32, "little"), m),   # s = l - 1: canonical, wrong
             (pk, sig[:32] + (s + L_ORDER).to_bytes(32, "little"), m)]   # s + l: right residue, not canonical
    want = [of.verify(*it) for it in items]
    assert want == [True] + [False] * 6
    assert each_verify(ee, items) == want
    assert each_verify(ee, items, reuse=True) == want
    assert lane_verify(ee, items) == want


def test_one_bit_flips(ee):
    """random valid signatures with one bit flipped in R, s, A and the message"""
    rnd = random.Random(13)
    items = []
    for j in range(12):
        seed = rnd.randbytes(32)
        m = rnd.randbytes(rnd.choice([1, 32, 47, 48, 111, 112, 200]))
        pk, sig = of.pubkey(seed), of.sign(seed, m)
        items.append((pk, sig, m))
        bit = rnd.randrange(256)
        flip = lambda b, i: b[:i // 8] + bytes([b[i // 8] ^ (1 << (i % 8))]) + b[i // 8 + 1:]
        kind = j % 4
        if kind == 0:
            items.append((pk, flip(sig, bit), m))
        elif kind == 1:
            items.append((pk, flip(sig, 256 + bit % 252), m))
        elif kind == 2:
            items.append((flip(pk, bit), sig, m))
        else:
            items.append((pk, sig, flip(m, bit % (8 * len(m)))))
    want = [of.verify(*it) for it in items]
    assert want[::2] == [True] * 12 and not any(want[1::2])
    assert each_verify(ee, items) == want
    assert each_verify(ee, items, reuse=True) == want
    assert lane_verify(ee, items) == want


def test_forced_challenge_scalars(ee):
    """k fed straight to the split and the loop, with s = r + k a so the equation holds for it, and
    s + 1 so it misses: the row form and lane_straus_check_half agree, both signs of v and digit
    positions that add the identity entry are covered"""
    rnd = random.Random(17)
    ks = [0, 1, 2, L_ORDER - 1, L_ORDER // 2, 2**127 - 1, 2**127, 2**252]
    ks += [rnd.randrange(L_ORDER) for _ in range(1000)]
    out = np.zeros(5, dtype=np.int32)
    signs, zeros = set(), 0
    for j, k in enumerate(ks):
        a, r = rnd.randrange(1, L_ORDER), rnd.randrange(1, L_ORDER)
        spoil = 1 if (j >= 8 and j % 8 == 0) else 0
        runs = [0, 1] if j < 8 else [spoil]
        for sp in runs:
            rc = ee.he_each_forced_k(k.to_bytes(32, "little"), a.to_bytes(32, "little"), r.to_bytes(32, "little"),
                                     sp, out.ctypes.data)
            assert rc == 0 and out[4] == 0, (k, rc)
            assert out[0] == out[1] == 1 - sp, (hex(k), sp, out.tolist())
            signs.add(int(out[2]))
            zeros += int(out[3])
    assert signs == {0, 1}
    assert zeros > 1000
