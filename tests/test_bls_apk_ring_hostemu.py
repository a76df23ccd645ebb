"""The key side of a BLS call that uses the aggregate-key ring, on the host
(tests/hostemu/bls_apk_ring_hostemu.cpp: bls_verify.h's w_apk_fill, the item function of
k_blsw_apk_fill, compiled for the CPU).  A ring slot holds, for a signer set, what registration
holds for one key: the [h_eff]-side affine record and its line table.  The fill makes them from the
Jacobian sum the miss item has computed anyway; here they are compared with registration's own code
run on the oracle's aggregate of the same keys, and a hit item's pairing verdict with the miss
item's and the oracle's.

A record's limbs stand for a value in [0, 2p), and two routes to one point (the sum of the keys'
[h_eff] multiples; the [h_eff] multiple of the keys' sum) need not end on the same representative.
The fill writes the canonical one, so registration's record is made canonical (bah_canon) before
the comparison; from then on -- the record, and the line table computed from it -- every word is
compared as it is."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import bls_ffi as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "_build", "libblsaremu.so")
r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
SIZES = (2, 3, 67)      # 67: lanes 0-2 add two keys each, and every level of the tree adds


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-C", ROOT, "tests/_build/libblsaremu.so"], check=True)
    L = ctypes.CDLL(SO)
    c, sz, vp, i32, u32 = ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    for f in ("bah_rec_words", "bah_jac_words", "bah_line_words"):
        getattr(L, f).restype = i32
    L.bah_key_heff.argtypes, L.bah_key_heff.restype = [c, vp], i32
    L.bah_canon.argtypes, L.bah_canon.restype = [vp, i32], None
    L.bah_key_lines.argtypes, L.bah_key_lines.restype = [vp, u32, vp], None
    L.bah_sum.argtypes, L.bah_sum.restype = [vp, sz, vp], i32
    L.bah_fill.argtypes, L.bah_fill.restype = [vp, i32, u32, vp, vp], i32
    L.bah_one_key.argtypes, L.bah_one_key.restype = [vp, vp], None
    L.bah_verdict.argtypes, L.bah_verdict.restype = [c, c, sz, c, sz, vp, vp, u32], i32
    return L


@pytest.fixture(scope="module")
def keys(emu):
    """67 key pairs and each key's registration record ([h_eff] pk), computed once"""
    rnd = random.Random(20261021)
    sks = [rnd.randrange(1, r).to_bytes(32, "big") for _ in range(67)]
    pks = []
    for sk in sks:
        rc, pk = B.keygen(sk)
        assert rc == 0
        pks.append(pk)
    W = emu.bah_rec_words()
    hrec = np.zeros((67, W), dtype=np.uint32)
    for j, pk in enumerate(pks):
        assert emu.bah_key_heff(pk, hrec[j].ctypes.data) == B.ORB_OK
    return sks, pks, hrec


@pytest.fixture(scope="module")
def filled(emu, keys):
    """per set size: (the miss item's Jacobian sum, the filled record, the filled line table)"""
    _, _, hrec = keys
    out = {}
    for n in SIZES:
        aj = np.zeros(emu.bah_jac_words(), dtype=np.uint32)
        assert emu.bah_sum(hrec[:n].ctypes.data, n, aj.ctypes.data) == B.ORB_OK
        rec = np.full(emu.bah_rec_words(), 0xDEADBEEF, dtype=np.uint32)
        lines = np.full(emu.bah_line_words(), 0xDEADBEEF, dtype=np.uint32)
        assert emu.bah_fill(aj.ctypes.data, B.ORB_OK, 0xA5A5A5A5, rec.ctypes.data, lines.ctypes.data) == 1
        out[n] = (aj, rec, lines)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_the_fill_equals_registration_of_the_oracles_key_sum(emu, keys, filled, n):
    _, pks, _ = keys
    _, rec, lines = filled[n]
    rc, apk = B.aggregate_pubkeys(pks[:n])          # the oracle's key aggregation: the affine sum
    assert rc == 0
    want = np.zeros(emu.bah_rec_words(), dtype=np.uint32)
    assert emu.bah_key_heff(apk, want.ctypes.data) == B.ORB_OK      # k_bls_key_heff's record of that point
    emu.bah_canon(want.ctypes.data, 4)
    assert np.array_equal(rec, want), "the slot's record, word for word, flag word included"
    want_lines = np.zeros(emu.bah_line_words(), dtype=np.uint32)
    emu.bah_key_lines(want.ctypes.data, 0, want_lines.ctypes.data)   # w_key_lines' table of that point
    assert np.array_equal(lines, want_lines), "the slot's line table, word for word"


def test_the_fill_does_not_depend_on_the_order_of_the_sum(emu, keys, filled):
    """the same set added up in another order is another Jacobian triple and the same slot"""
    _, _, hrec = keys
    perm = list(range(67))
    random.Random(5).shuffle(perm)
    aj = np.zeros(emu.bah_jac_words(), dtype=np.uint32)
    assert emu.bah_sum(np.ascontiguousarray(hrec[perm]).ctypes.data, 67, aj.ctypes.data) == B.ORB_OK
    assert not np.array_equal(aj, filled[67][0])
    rec = np.zeros(emu.bah_rec_words(), dtype=np.uint32)
    lines = np.zeros(emu.bah_line_words(), dtype=np.uint32)
    assert emu.bah_fill(aj.ctypes.data, B.ORB_OK, 0, rec.ctypes.data, lines.ctypes.data) == 1
    assert np.array_equal(rec, filled[67][1]) and np.array_equal(lines, filled[67][2])


@pytest.mark.parametrize("n", SIZES)
def test_a_hit_items_verdict_equals_the_miss_items(emu, keys, filled, n):
    """valid aggregate, forged aggregate, wrong message: the miss item (the Jacobian sum, computed
    lines), the hit item (the slot's record with Z = 1, the slot's line table) and the oracle"""
    sks, pks, _ = keys
    aj, rec, lines = filled[n]
    one = np.zeros(emu.bah_jac_words(), dtype=np.uint32)
    emu.bah_one_key(rec.ctypes.data, one.ctypes.data)
    m = bytes(range(32))
    rc, agg = B.aggregate([B.sign(sk, m) for sk in sks[:n]])
    assert rc == 0
    rc, forged = B.aggregate([B.sign(sk, m) for sk in sks[1:n + 1]] if n < 67 else
                             [B.sign(sk, m) for sk in sks[:n - 1]])
    assert rc == 0
    cases = [(agg, m), (forged, m), (agg, m[:-1] + b"\xff")]
    want = [B.fast_aggregate_verify(s, pks[:n], mm) for s, mm in cases]
    assert want == [B.ORB_OK, B.ORB_VERIFY_FAIL, B.ORB_VERIFY_FAIL]
    d = B.DST_NUL
    miss = [emu.bah_verdict(s, mm, len(mm), d, len(d), aj.ctypes.data, None, 0) for s, mm in cases]
    hit = [emu.bah_verdict(s, mm, len(mm), d, len(d), one.ctypes.data, lines.ctypes.data, 0xA5A5A5A5)
           for s, mm in cases]
    assert miss == want and hit == want


def test_an_identity_sum_is_pk_infinity_and_never_handed_to_the_fill(emu):
    sk = random.Random(7).randrange(1, r)
    pair = []
    for s in (sk, r - sk):
        rc, pk = B.keygen(s.to_bytes(32, "big"))
        assert rc == 0
        pair.append(pk)
    m = bytes(32)
    rc, agg = B.aggregate([B.sign(sk.to_bytes(32, "big"), m), B.sign((r - sk).to_bytes(32, "big"), m)])
    assert B.fast_aggregate_verify(agg, pair, m) == B.ORB_PK_INFINITY
    hrec = np.zeros((2, emu.bah_rec_words()), dtype=np.uint32)
    for j, pk in enumerate(pair):
        assert emu.bah_key_heff(pk, hrec[j].ctypes.data) == B.ORB_OK
    aj = np.zeros(emu.bah_jac_words(), dtype=np.uint32)
    st = emu.bah_sum(hrec.ctypes.data, 2, aj.ctypes.data)
    assert st == B.ORB_PK_INFINITY and aj[-1] == 1, "the miss path's status is the oracle's"
    for status in (st, B.ORB_OK):     # the status alone stops the fill, and so does the record's flag
        rec = np.full(emu.bah_rec_words(), 0xDEADBEEF, dtype=np.uint32)
        lines = np.full(emu.bah_line_words(), 0xDEADBEEF, dtype=np.uint32)
        assert emu.bah_fill(aj.ctypes.data, status, 0, rec.ctypes.data, lines.ctypes.data) == 0
        assert (rec == 0xDEADBEEF).all() and (lines == 0xDEADBEEF).all(), "nothing is written"
    # a valid sum behind a failed status (a bad key elsewhere in the list) is not stored either
    ok = np.zeros(emu.bah_jac_words(), dtype=np.uint32)
    emu.bah_one_key(hrec[0].ctypes.data, ok.ctypes.data)
    rec = np.full(emu.bah_rec_words(), 0xDEADBEEF, dtype=np.uint32)
    lines = np.full(emu.bah_line_words(), 0xDEADBEEF, dtype=np.uint32)
    assert emu.bah_fill(ok.ctypes.data, B.ORB_NOT_IN_GROUP, 0, rec.ctypes.data, lines.ctypes.data) == 0
    assert (rec == 0xDEADBEEF).all()
