"""The pieces trimmed out of the batch MSM's instruction stream, on the host
(tests/hostemu/trim_hostemu.cpp, built with NWV_BOUNDS_CHECK: every limb bound and every pre-carry
column sum below 2^63 is asserted):

* msm_point_seed: a bucket lane's first record becomes its running sum as (2x : 2y : 2 : 2xy)
  instead of being added to the identity;
* fe_sq's operand split (13 scaled operands): limb for limb fe_mul(f, f) and the limbs the previous
  split gave (tests/golden/fe_sq_limbs_before_operand_split.npy: fe_sq and five repeated squarings
  of fe_vectors.operand_pairs(1000, seed=20251) followed by the all-limbs-at-bound element, written
  by the library's fe_sq / fe_sqn before the split changed);
* ge_p1p1_to_p3 / _to_p2 with commuted operands: limb for limb the products in the old order;
* SHA-512 of a 64-byte prefix and a message, at every padding boundary, against hashlib.
The device's code paths are checked by tests/test_gpu_trim.py."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import fe_vectors as fv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "_build", "libtrimemu.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")
# with the 64-byte prefix these straddle every padding boundary of one to five blocks
SHA_LENGTHS = (0, 1, 46, 47, 48, 63, 64, 111, 112, 127, 128, 175, 176, 191, 192, 255, 256, 511, 512, 513)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        import subprocess
        subprocess.run(["make", "-C", ROOT, "tests/_build/libtrimemu.so"], check=True)
    so = ctypes.CDLL(LIB_PATH)
    vp = ctypes.c_void_p
    so.he_trim_dinv_ok.restype = ctypes.c_int
    so.he_trim_seed.argtypes = [ctypes.c_uint32, vp, vp, vp]
    so.he_trim_sq.argtypes = [ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_int]
    so.he_trim_p1p1.argtypes = [ctypes.c_uint32, vp, vp, vp, vp, vp]
    so.he_trim_sha512.argtypes = [vp, vp, ctypes.c_uint32, vp]
    return so


def seed_status(lib, encodings):
    enc = np.frombuffer(b"".join(encodings), dtype=np.uint8)
    status = np.full(len(encodings), 255, dtype=np.uint8)
    seed0 = np.zeros(40, dtype=np.uint32)
    lib.he_trim_seed(len(encodings), enc.ctypes.data, status.ctypes.data, seed0.ctypes.data)
    return status, seed0


def test_dinv_is_the_inverse_of_d(lib):
    assert lib.he_trim_dinv_ok() == 1


def test_seed_of_golden_and_small_order_points(lib):
    """every key and R of the golden vectors and every ZIP-215 small-order encoding, both signs"""
    with open(os.path.join(GOLDEN, "ed25519_vectors.json")) as f:
        g = json.load(f)
    with open(os.path.join(GOLDEN, "zip215_small_order.json")) as f:
        z = json.load(f)
    enc = []
    for v in g["vectors"]:
        enc += [bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"])[:32]]
    small = [bytes.fromhex(e) for e in z["encodings"]]
    enc = list(dict.fromkeys(enc + small))
    status, _ = seed_status(lib, enc)
    assert set(status.tolist()) <= {0, 1}, [(e.hex(), int(s)) for e, s in zip(enc, status) if s > 1]
    # every point of an accepted signature decodes, and every small-order encoding (ZIP-215
    # accepts them all): none of those is skipped
    for v in g["vectors"]:
        if v["expect"]:
            assert status[enc.index(bytes.fromhex(v["pk"]))] == 0
            assert status[enc.index(bytes.fromhex(v["sig"])[:32])] == 0
    assert all(status[enc.index(e)] == 0 for e in small)


def test_seed_of_x_zero_points(lib):
    """the identity (y = 1) seeds as (0 : 2 : 2 : 0); (0, -1) and the "negative zero" encodings too"""
    one = (1).to_bytes(32, "little")
    minus_one = (fv.P - 1).to_bytes(32, "little")
    neg0 = bytes(one[:31]) + bytes([one[31] | 0x80])
    neg0m = bytes(minus_one[:31]) + bytes([minus_one[31] | 0x80])
    status, seed0 = seed_status(lib, [one, minus_one, neg0, neg0m])
    assert status.tolist() == [0, 0, 0, 0]
    X, Y, Z, T = (fv.value(seed0[10 * k:10 * k + 10]) % fv.P for k in range(4))
    assert (X, Y, Z, T) == (0, 2, 2, 0)


def test_seed_of_random_points(lib):
    """256 random points (seeded): the first 256 of 700 random encodings that decode"""
    rnd = np.random.default_rng(65536)
    enc = [rnd.bytes(32) for _ in range(700)]
    status, _ = seed_status(lib, enc)
    assert set(status.tolist()) <= {0, 1}, [(e.hex(), int(s)) for e, s in zip(enc, status) if s > 1]
    assert int((status == 0).sum()) >= 256


@pytest.fixture(scope="module")
def sq_inputs():
    a, _ = fv.operand_pairs(1000, seed=20251)
    return np.ascontiguousarray(np.concatenate([a, np.array([fv.MAXLIMB], dtype=np.uint32)]))


def test_fe_sq_operand_split(lib, sq_inputs):
    a = sq_inputs
    n = len(a)
    assert list(a[-1]) == list(fv.MAXLIMB) and any(list(r) == [m - 1 for m in fv.MAXLIMB] for r in a)
    sq, mul, sqn = (np.zeros((n, 10), dtype=np.uint32) for _ in range(3))
    lib.he_trim_sq(n, a.ctypes.data, sq.ctypes.data, mul.ctypes.data, sqn.ctypes.data, 5)
    assert np.array_equal(sq, mul)
    before = np.load(os.path.join(GOLDEN, "fe_sq_limbs_before_operand_split.npy"))
    assert before.shape == (2, n, 10)
    assert np.array_equal(sq, before[0])
    assert np.array_equal(sqn, before[1])
    for k in range(n):
        x = fv.value(a[k])
        assert fv.value(sq[k]) % fv.P == x * x % fv.P
        assert fv.value(sqn[k]) % fv.P == pow(x, 32, fv.P)


def test_p1p1_conversions_keep_their_limbs(lib):
    """completed points with every limb up to the multiply's admitted magnitude (3.36), the
    all-at-bound point included"""
    rnd = np.random.default_rng(4)
    n = 2000
    pts = np.zeros((n, 40), dtype=np.uint32)
    for c in range(40):
        pts[:, c] = rnd.integers(0, fv.MAXLIMB[c % 10] + 1, size=n)
    pts[0] = np.array(list(fv.MAXLIMB) * 4, dtype=np.uint32)
    pts[1] = 0
    got, want = np.zeros((n, 40), dtype=np.uint32), np.zeros((n, 40), dtype=np.uint32)
    got2, want2 = np.zeros((n, 30), dtype=np.uint32), np.zeros((n, 30), dtype=np.uint32)
    lib.he_trim_p1p1(n, pts.ctypes.data, got.ctypes.data, want.ctypes.data, got2.ctypes.data, want2.ctypes.data)
    assert np.array_equal(got, want)
    assert np.array_equal(got2, want2)
    for k in range(0, n, 97):
        X, Y, Z, T = (fv.value(pts[k, 10 * c:10 * c + 10]) for c in range(4))
        for c, w in enumerate((X * T, Y * Z, Z * T, X * Y)):
            assert fv.value(got[k, 10 * c:10 * c + 10]) % fv.P == w % fv.P


@pytest.mark.parametrize("mlen", SHA_LENGTHS)
def test_sha512_prefixed(lib, mlen):
    rnd = np.random.default_rng(1000 + mlen)
    prefix, msg = rnd.bytes(64), rnd.bytes(mlen)
    out = ctypes.create_string_buffer(64)
    lib.he_trim_sha512(prefix, msg, mlen, out)
    assert out.raw == hashlib.sha512(prefix + msg).digest()
