"""The hash role of a BLS call that uses the message ring, on the host
(tests/hostemu/bls_msg_ring_hostemu.cpp: bls_verify.h's w_hash_ring_item, the item function of
k_blsw_pre_r, compiled for the CPU).  The ring keeps the RAW hashed point -- the sum of the two
isogeny maps -- and an item takes it as it is (its cached keys carry h_eff) or runs the h_eff chain
on it.  Whatever route an item's record took (computed, copied from a slot, a slot's record run
through the chain), it must equal w_hash_to_g1's word for word, identity flag included."""
import ctypes
import json
import os
import random
import subprocess

import numpy as np
import pytest

import bls_ffi as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "_build", "libblsmremu.so")
FILLS = (0, 0xA5A5A5A5)   # what the wave's slots hold before the item runs


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-C", ROOT, "tests/_build/libblsmremu.so"], check=True)
    L = ctypes.CDLL(SO)
    c, sz, vp, i32, u32 = ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    L.bmh_rec_words.restype = i32
    L.bmh_hash.argtypes, L.bmh_hash.restype = [c, sz, c, sz, i32, u32, vp, vp], None
    L.bmh_ring_item.argtypes, L.bmh_ring_item.restype = [c, sz, c, sz, vp, vp, i32, u32, vp], None
    L.bmh_affine.argtypes, L.bmh_affine.restype = [vp, vp], None
    return L


@pytest.fixture(scope="module")
def cases():
    with open(os.path.join(ROOT, "tests", "golden", "bls12381_kats.json")) as f:
        gold = json.load(f)
    out = [(bytes.fromhex(v["msg"]), v["dst"].encode(), bytes.fromhex(v["x"] + v["y"])) for v in gold["hash_to_g1"]]
    rnd = random.Random(20261020)
    for _ in range(3):   # protocol messages: 32-byte digests under the signature DST
        m = rnd.randbytes(32)
        out.append((m, B.DST_NUL, B.hash_to_g1(m)))
    return out


@pytest.fixture(scope="module")
def reference(emu, cases):
    """w_hash_to_g1's two forms of every case, computed once: (raw, cleared)"""
    W = emu.bmh_rec_words()
    ref = []
    for m, dst, _ in cases:
        raw, clr = np.zeros(W, dtype=np.uint32), np.zeros(W, dtype=np.uint32)
        emu.bmh_hash(m, len(m), dst, len(dst), 0, 0, raw.ctypes.data, None)
        emu.bmh_hash(m, len(m), dst, len(dst), 1, 0, clr.ctypes.data, None)
        ref.append((raw, clr))
    return ref


def _item(emu, case, src, want_pub, key_side, fill):
    m, dst, _ = case
    W = emu.bmh_rec_words()
    out = np.full(W, 0xDEADBEEF, dtype=np.uint32)
    pub = np.full(W, 0xDEADBEEF, dtype=np.uint32) if want_pub else None
    emu.bmh_ring_item(m, len(m), dst, len(dst), src.ctypes.data if src is not None else None,
                      pub.ctypes.data if want_pub else None, 1 if key_side else 0, fill, out.ctypes.data)
    return out, pub


def test_the_reference_forms_are_the_known_answers(emu, cases, reference):
    """the cleared form is H(m) of RFC 9380 J.9.1 / the oracle; the raw form is another point, and
    not the identity"""
    o = ctypes.create_string_buffer(96)
    for (m, dst, want), (raw, clr) in zip(cases, reference):
        emu.bmh_affine(clr.ctypes.data, o)
        assert o.raw == want
        assert raw[-1] == 0 and clr[-1] == 0 and not np.array_equal(raw, clr)


def test_w_hash_to_g1_writes_the_raw_record_before_the_chain(emu, cases, reference):
    W = emu.bmh_rec_words()
    for (m, dst, _), (raw, clr) in zip(cases, reference):
        for fill in FILLS:
            out, r = np.zeros(W, dtype=np.uint32), np.zeros(W, dtype=np.uint32)
            emu.bmh_hash(m, len(m), dst, len(dst), 1, fill, out.ctypes.data, r.ctypes.data)
            assert np.array_equal(out, clr) and np.array_equal(r, raw)


@pytest.mark.parametrize("fill", FILLS)
def test_miss_key_side(emu, cases, reference, fill):
    """computed raw, and the slot gets the same record; without a slot the item's record alone"""
    for case, (raw, _) in zip(cases, reference):
        out, pub = _item(emu, case, None, True, True, fill)
        assert np.array_equal(out, raw) and np.array_equal(pub, raw)
        out, _ = _item(emu, case, None, False, True, fill)
        assert np.array_equal(out, raw)


@pytest.mark.parametrize("fill", FILLS)
def test_miss_not_key_side(emu, cases, reference, fill):
    """the slot gets the raw record, the item the cleared one"""
    for case, (raw, clr) in zip(cases, reference):
        out, pub = _item(emu, case, None, True, False, fill)
        assert np.array_equal(out, clr) and np.array_equal(pub, raw)
        out, _ = _item(emu, case, None, False, False, fill)
        assert np.array_equal(out, clr)


@pytest.mark.parametrize("fill", FILLS)
def test_hit_key_side_copies_the_record(emu, cases, reference, fill):
    for case, (raw, _) in zip(cases, reference):
        # (the message is not read on a hit: a wrong one changes nothing)
        out, _ = _item(emu, (b"another message", case[1], None), raw.copy(), False, True, fill)
        assert np.array_equal(out, raw)


@pytest.mark.parametrize("fill", FILLS)
def test_hit_not_key_side_runs_the_chain_alone(emu, cases, reference, fill):
    """raw followed by the chain = w_hash_to_g1(clear = true), identity-flag word included"""
    for case, (raw, clr) in zip(cases, reference):
        src = raw.copy()
        out, _ = _item(emu, (b"another message", case[1], None), src, False, False, fill)
        assert np.array_equal(out, clr)
        assert np.array_equal(src, raw), "the ring's record is only read"


def test_the_identity_keeps_its_flag_through_the_chain(emu):
    """a raw record that is the identity (Z = 0; no hash gives one, the chain is exact on it
    anyway): the cleared record carries the flag"""
    W = emu.bmh_rec_words()
    src = np.zeros(W, dtype=np.uint32)
    src[-1] = 1
    nl = (W - 1) // 3
    src[nl] = 1   # (0 : y : 0)
    out, _ = _item(emu, (b"", B.DST_NUL, None), src, False, False, 0)
    assert out[-1] == 1   # (Z itself may be any representative of 0 mod p: the flag is what readers test)
    out, _ = _item(emu, (b"", B.DST_NUL, None), src, False, True, 0)
    assert np.array_equal(out, src)
