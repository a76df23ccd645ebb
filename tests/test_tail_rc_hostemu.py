"""The chunk phase of k_msm_tail by rows and columns (narwhal_amd/csrc/msm.h tail_rc_op), on the host
(tests/hostemu/tail_rc_hostemu.cpp, built with NWV_BOUNDS_CHECK: every limb bound and every
pre-carry column sum is asserted): the schedule is run level by level exactly as the workgroup's
lanes run it, and its planes are compared, plane by plane, with the single bit-plane butterfly the
kernel used before, and  sum_k 2^k T_k + U  with  sum (t + 1) S_t  added up directly.

Chunk sizes 2 .. 256 (square and rectangular views), chunks of random points, of empty buckets
(the identity), of equal points in every partner pair (the additions must be the complete one: a
doubling goes through them), of a point and its negative in partner slots (sums that pass through
the identity), and of the small-order points of tests/golden/zip215_small_order.json.
The device's code path is checked by tests/test_gpu_tail_rc.py."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import oracle_ffi as of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "_build", "libtailrcemu.so")
SIZES = [2, 4, 8, 16, 32, 64, 128, 256]
IDENTITY = (1).to_bytes(32, "little")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        import subprocess
        subprocess.run(["make", "-C", ROOT, "tests/_build/libtailrcemu.so"], check=True)
    so = ctypes.CDLL(LIB_PATH)
    so.he_tail_rc_check.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return so


@pytest.fixture(scope="module")
def points():
    """300 points of the prime-order subgroup (public keys of seeded secrets)"""
    rnd = random.Random(256)
    return [of.pubkey(bytes(rnd.getrandbits(8) for _ in range(32))) for _ in range(300)]


@pytest.fixture(scope="module")
def small_order():
    with open(os.path.join(ROOT, "tests", "golden", "zip215_small_order.json")) as f:
        return [bytes.fromhex(e) for e in json.load(f)["encodings"]]


def neg(enc):
    return enc[:31] + bytes([enc[31] ^ 0x80])


def check(lib, encs):
    C = len(encs)
    m = C.bit_length() - 1
    assert 1 << m == C
    buf = np.frombuffer(b"".join(encs), dtype=np.uint8)
    info = (ctypes.c_int * 4)()
    rc = lib.he_tail_rc_check(m, buf.ctypes.data, info)
    assert rc == 0, (C, rc, list(info))
    return list(info)


def counts(C):
    """additions, waves of additions (a level at a time, 64 operations a wave), widest level"""
    m = C.bit_length() - 1
    lc = m // 2
    lr = m - lc
    adds = waves = widest = 0
    for ph in range(m):
        ops = (C >> (ph + 1)) if ph < lc else 1 << (lr - 1)
        if lc:
            ops += (C >> (ph + 1)) if ph < lr else 1 << (lc - 1)
        adds += ops
        waves += -(-ops // 64)
        widest = max(widest, ops)
    return adds, waves, widest


@pytest.mark.parametrize("C", SIZES)
def test_random_chunk_matches_butterfly_and_direct_sum(lib, points, C):
    rnd = random.Random(C)
    info = check(lib, [rnd.choice(points) for _ in range(C)])
    assert tuple(info[0:2]) + (info[3],) == counts(C)
    assert info[3] <= C and info[2] == -1
    m = C.bit_length() - 1
    if C == 256:
        # two trees (2 x 240) and two 16-point butterflies (2 x 32), in 12 waves: the butterfly
        # of the whole chunk takes 1,024 additions in 16
        assert info[0] == 544 and info[1] == 12 < 2 * m
    else:
        # one wave a level, as the butterfly -- but two for the first level at 128, which is why
        # the kernel keeps the butterfly below 256
        assert info[1] == m + (C == 128)


@pytest.mark.parametrize("C", SIZES)
def test_empty_buckets(lib, points, C):
    """all empty; one bucket full; every other bucket empty; one bucket empty"""
    rnd = random.Random(1000 + C)
    check(lib, [IDENTITY] * C)
    for t in sorted({0, 1, C // 2, C - 1}):
        check(lib, [IDENTITY] * t + [points[t]] + [IDENTITY] * (C - 1 - t))
    check(lib, [rnd.choice(points) if t & 1 else IDENTITY for t in range(C)])
    check(lib, [rnd.choice(points) if t != C // 2 else IDENTITY for t in range(C)])


@pytest.mark.parametrize("C", SIZES)
def test_equal_points_in_partner_slots(lib, points, C):
    """the same point in every bucket: every addition of every level adds a point to itself.  And
    equal points in single pairs: neighbours, the two halves, a row apart"""
    check(lib, [points[7]] * C)
    rnd = random.Random(2000 + C)
    m = C.bit_length() - 1
    for stride in sorted({1, C // 2, 1 << (m // 2)}):
        encs = [rnd.choice(points) for _ in range(C)]
        for t in range(C):
            if t & stride:
                encs[t] = encs[t ^ stride]
        check(lib, encs)


@pytest.mark.parametrize("C", SIZES)
def test_point_and_its_negative(lib, points, C):
    """partner pairs that cancel: whole levels sum to the identity and go on from there"""
    rnd = random.Random(3000 + C)
    m = C.bit_length() - 1
    for stride in sorted({1, C // 2, 1 << (m // 2)}):
        encs = [rnd.choice(points) for _ in range(C)]
        for t in range(C):
            if t & stride:
                encs[t] = neg(encs[t ^ stride])
        check(lib, encs)
    encs = [points[3], neg(points[3])] * (C // 2)
    check(lib, encs)


@pytest.mark.parametrize("C", [2, 4, 8, 16, 64, 256])
def test_small_order_points(lib, points, small_order, C):
    """chunks of small-order points alone (with repeats: doublings and cancellations among the
    eight torsion points at every level), and mixed into honest points"""
    assert len(small_order) >= 8
    rnd = random.Random(4000 + C)
    check(lib, [small_order[t % len(small_order)] for t in range(C)])
    check(lib, [rnd.choice(small_order) for _ in range(C)])
    check(lib, [rnd.choice(small_order) if rnd.random() < 0.3 else rnd.choice(points) for _ in range(C)])
