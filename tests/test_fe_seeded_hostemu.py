"""fe25519.h's multiply, squaring and repeated squaring in every column-sum form (FE_COLS_*: the
carry of a column seeds the next column's sum instead of being added afterwards), on the host
(tests/hostemu/fe_seeded_hostemu.cpp, built with NWV_BOUNDS_CHECK: every pre-carry column sum,
carry-in included, is asserted below 2^63 and every input within magnitude 3.36), against Python
integers mod 2^255 - 19.  The device's inline-assembly path is checked by
tests/test_gpu_fe_seeded.py."""
import ctypes
import os

import numpy as np
import pytest

import fe_vectors as fv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "_build", "libfeseeded.so")

PLAIN, SERIAL, TWO, HALVES, THREE, BYCOL = 0, 1, 2, 3, 4, 8
FORMS = {"plain": PLAIN, "serial": SERIAL, "two_chains": TWO, "halves": HALVES, "three_chains": THREE,
         "serial_bycol": SERIAL | BYCOL, "two_chains_bycol": TWO | BYCOL, "halves_bycol": HALVES | BYCOL,
         "three_chains_bycol": THREE | BYCOL, "library": -1}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        import subprocess
        subprocess.run(["make", "-C", ROOT, "tests/_build/libfeseeded.so"], check=True)
    so = ctypes.CDLL(LIB_PATH)
    vp = ctypes.c_void_p
    so.he_fe_ops.argtypes = [ctypes.c_int, ctypes.c_uint32, vp, vp, vp, vp, vp, ctypes.c_int]
    so.he_fe_ops.restype = ctypes.c_int
    return so


def run(lib, form, a, b, nsq=fv.NSQ):
    n = len(a)
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    out = [np.zeros((n, 10), dtype=np.uint32) for _ in range(3)]
    assert lib.he_fe_ops(form, n, a.ctypes.data, b.ctypes.data, *(o.ctypes.data for o in out), nsq) == 0
    return out


@pytest.fixture(scope="module")
def cases():
    """the edge set and 10,000 random elements (carried and uncarried), with the integer reference"""
    a, b = fv.operand_pairs(10000, seed=20250)
    return a, b, fv.reference(a, b)


def test_default_form_is_seeded(lib):
    assert lib.he_fe_default_form() == SERIAL | BYCOL


@pytest.mark.parametrize("form", list(FORMS))
def test_forms_match_integers(lib, cases, form):
    a, b, ref = cases
    mul, sq, sqn = run(lib, FORMS[form], a, b)
    fv.check(a, b, mul, sq, sqn, ref)


def test_two_chain_form_gives_fe_carry64_limbs(lib, cases):
    """the two-chain form carries in fe_carry64's order: the plain form's limbs exactly; a
    by-column variant gives its term-by-term form's limbs"""
    a, b, _ = cases
    plain = run(lib, PLAIN, a[:2000], b[:2000], nsq=3)
    two = run(lib, TWO, a[:2000], b[:2000], nsq=3)
    for p, t in zip(plain, two):
        assert np.array_equal(p, t)
    for base in (SERIAL, TWO, HALVES, THREE):
        for x, y in zip(run(lib, base, a[:2000], b[:2000], nsq=3), run(lib, base | BYCOL, a[:2000], b[:2000], nsq=3)):
            assert np.array_equal(x, y)


def test_library_form_is_fully_carried(lib, cases):
    """one chain through all ten columns: limbs 2..9 leave below their width, limb 0 below 2^26,
    limb 1 below 2^25 + 2^18 (it takes the wrap's last carry, as fe_carry64's does)"""
    a, b, _ = cases
    for out in run(lib, -1, a, b, nsq=2):
        assert int(out[:, 0].max()) < 1 << 26
        assert int(out[:, 1].max()) < (1 << 25) + (1 << 18)
        for i in range(2, 10):
            assert int(out[:, i].max()) < 1 << fv.BITS[i]
