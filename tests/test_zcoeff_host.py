"""tests/zcoeff.py against the references it restates, and the cancelling-forgery construction
against the host emulation of the batch MSM (tests/hostemu, he_msm_batch / he_msm_batch_split):
a set built for the documented coefficients is accepted under its seed and rejected under any
other, while a set built for a coefficient wrong in one bit, or for two positions sharing one
coefficient, is rejected -- which is what lets tests/test_gpu_zcoeff.py pin every z_i the device
uses."""
import ctypes
import random
import struct

import numpy as np
import pytest

import oracle_ffi as of
import zcoeff as zc
from test_msm_hostemu import RFC8439_BLOCK, _chacha20_block_py, he, honest, msm_batch  # noqa: F401

SEED = bytes(range(100, 132))
OTHER = bytes(range(101, 133))
IDX = [0, 1, 255, 256, 65535, 65536, 2**32 - 1, 2**32, 2**32 + 5]
N = 12
SETS = {"pair": [3, 11], "sparse": [0, 4, 5, 9], "all": list(range(N))}


def test_vectorised_block_reproduces_rfc8439():
    """RFC 8439 section 2.3.2: key 00..1f, counter 1, nonce 00:00:00:09:00:00:00:4a:00:00:00:00;
    and several blocks at once equal the one-at-a-time reference"""
    blk = zc.chacha20_blocks(bytes(range(32)), 1, 0x09000000, 0x4a000000, 0)
    assert blk.shape == (1, 16) and blk.astype("<u4").tobytes() == RFC8439_BLOCK
    rnd = random.Random(2)
    key = rnd.randbytes(32)
    ctr = [rnd.getrandbits(32) for _ in range(7)]
    n0 = [rnd.getrandbits(32) for _ in range(7)]
    blk = zc.chacha20_blocks(key, ctr, n0, 5, 0xFFFFFFFF)
    for k in range(7):
        assert blk[k].astype("<u4").tobytes() == _chacha20_block_py(key, ctr[k], struct.pack("<3I", n0[k], 5, 0xFFFFFFFF))


def test_z_many_equals_reference_and_hostemu(he):
    out = ctypes.create_string_buffer(32)
    for seed in (SEED, bytes(32), b"\xff" * 32):
        got = zc.z_many(seed, IDX)
        assert got == zc.z_many(seed, np.array(IDX, dtype=np.uint64))
        for i, z in zip(IDX, got):
            want = bytearray(_chacha20_block_py(seed, i & 0xFFFFFFFF, struct.pack("<I", i >> 32) + b"nwv-z128")[:16])
            want[0] |= 1
            assert z == int.from_bytes(want, "little"), i
            he.he_msm_z(seed, i, out)
            assert out.raw == z.to_bytes(16, "little") + bytes(16), i
            assert z & 1 and z < 2**128
    assert len(set(zc.z_many(SEED, range(4096)))) == 4096
    assert zc.z_many(SEED, []) == []


def test_shard_seed_rule():
    assert zc.shard_seed(SEED, 0) == SEED
    s = zc.shard_seed(SEED, 0x0102030405060708)
    assert s[:24] == SEED[:24]
    assert bytes(a ^ b for a, b in zip(s[24:], SEED[24:])) == bytes([8, 7, 6, 5, 4, 3, 2, 1])
    assert zc.shard_seed(s, 0x0102030405060708) == SEED


@pytest.fixture(scope="module")
def batch():
    return honest(random.Random(1234), N)


def _with_sigs(items, sigs):
    return [(p, s, m) for (p, _, m), s in zip(items, sigs)]


def _touched_invalid(items, forged, P):
    for i in range(len(items)):
        if i in P:
            assert int.from_bytes(forged[i][1][32:], "little") < zc.L
            assert forged[i][1][:32] == items[i][1][:32]
            assert of.verify(*forged[i]) is False, i
        else:
            assert forged[i] == items[i]


@pytest.mark.parametrize("split", [False, True], ids=["plain", "split"])
@pytest.mark.parametrize("c", [8, -9])
@pytest.mark.parametrize("name", list(SETS))
def test_cancelling_set_accepts_under_its_seed_only(he, batch, name, c, split):
    P = SETS[name]
    rng = random.Random(f"{name}{c}{split}")
    forged = _with_sigs(batch, zc.cancelling([s for _, s, _ in batch], P, SEED, rng))
    _touched_invalid(batch, forged, P)
    assert msm_batch(he, batch, c, 16, seed=SEED, split=split)
    assert msm_batch(he, forged, c, 16, seed=SEED, split=split)
    assert not msm_batch(he, forged, c, 16, seed=OTHER, split=split)
    # the seed with one bit of its last byte flipped (the byte the shard rule touches)
    assert not msm_batch(he, forged, c, 16, seed=SEED[:31] + bytes([SEED[31] ^ 0x80]), split=split)


@pytest.mark.parametrize("split", [False, True], ids=["plain", "split"])
@pytest.mark.parametrize("bit", [1, 64, 127])
def test_one_wrong_coefficient_bit_is_rejected(he, batch, bit, split):
    """a set that would cancel if z_5 differed in one bit (as a truncated or mangled coefficient
    would) does not cancel under the real coefficients"""
    sigs = [s for _, s, _ in batch]
    for P in (SETS["pair"] + [5], SETS["all"]):
        zs = dict(zip(P, zc.z_many(SEED, P)))
        zs[5] ^= 1 << bit
        forged = _with_sigs(batch, zc.cancelling(sigs, P, SEED, random.Random(bit), zs=zs))
        _touched_invalid(batch, forged, P)
        assert not msm_batch(he, forged, 8, 16, seed=SEED, split=split)
    # truncated outright: only the low 32 bits of every coefficient live
    zs = {i: z & 0xFFFFFFFF for i, z in enumerate(zc.z_many(SEED, range(N)))}
    forged = _with_sigs(batch, zc.cancelling(sigs, SETS["all"], SEED, random.Random(32), zs=zs))
    assert not msm_batch(he, forged, 8, 16, seed=SEED, split=split)


@pytest.mark.parametrize("split", [False, True], ids=["plain", "split"])
def test_colliding_coefficients_are_rejected(he, batch, split):
    """a set built as if two positions shared one coefficient (s_i + d, s_j - d among them) is
    rejected; the same construction with the true coefficients is accepted"""
    sigs = [s for _, s, _ in batch]
    for P in ([3, 11], SETS["all"]):
        zs = dict(zip(P, zc.z_many(SEED, P)))
        good = _with_sigs(batch, zc.cancelling(sigs, P, SEED, random.Random(7), zs=dict(zs)))
        assert msm_batch(he, good, 8, 16, seed=SEED, split=split)
        zs[P[-1]] = zs[P[0]]
        forged = _with_sigs(batch, zc.cancelling(sigs, P, SEED, random.Random(7), zs=zs))
        _touched_invalid(batch, forged, P)
        assert not msm_batch(he, forged, 8, 16, seed=SEED, split=split)
    # the plain pair s_3 + d, s_11 - d
    d = random.Random(9).randrange(1, zc.L)
    pair = list(sigs)
    for i, e in ((3, d), (11, zc.L - d)):
        s = (int.from_bytes(pair[i][32:], "little") + e) % zc.L
        pair[i] = pair[i][:32] + s.to_bytes(32, "little")
    assert not msm_batch(he, _with_sigs(batch, pair), 8, 16, seed=SEED, split=split)


def test_cancelling_rejects_bad_position_sets(batch):
    sigs = [s for _, s, _ in batch]
    for P in ([], [3], [3, 3]):
        with pytest.raises(ValueError):
            zc.cancelling(sigs, P, SEED, random.Random(0))
