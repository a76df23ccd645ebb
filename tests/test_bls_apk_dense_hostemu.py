"""The dense key-sum stage of large BLS calls (nwv_bls_set_apk_dense_min; bls_verify.h's blsd_*
steps and jac_add_affine, bls_apk_dense.h's routing) compiled for the host
(tests/hostemu/bls_apk_dense_hostemu.cpp) and run on the CPU: k_blsd_total's 64 lanes and tree,
k_blsd_apk's L lanes and tree for L = 4, 8, 16.  Every item's sum (made affine) and status must be
the per-item kernel's (blsw_apk_item's 64 lanes over jac_add) on the same inputs, whichever way the
sum was taken: directly, or as the key table's total minus the keys a strictly ascending list
leaves out."""
import ctypes
import os
import random
import subprocess

import pytest

import bls_ffi as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
OK, NOT_ON_CURVE, NOT_IN_GROUP, PK_INFINITY = 0, 2, 3, 6
LANES = [4, 8, 16]


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(ROOT, "tests", "_build", "libblsademu.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-C", ROOT, "tests/_build/libblsademu.so"], check=True)
    L = ctypes.CDLL(path)
    c, sz, u32p, i32p = ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
    L.bh_ad_lanes.argtypes = [sz, ctypes.c_ulong]
    L.bh_ad_lanes.restype = ctypes.c_uint32
    L.bh_ad_split.argtypes = [sz, u32p, u32p, i32p]
    L.bh_ad_split.restype = None
    L.bh_ad_items.argtypes = [sz, c, c, i32p, sz, u32p, u32p, u32p, ctypes.c_uint32, i32p, i32p, i32p, i32p, i32p]
    return L


def _sk(x):
    return (x % R).to_bytes(32, "big")


@pytest.fixture(scope="module")
def keys():
    """seven keys of random secret keys, and -a, -b for the first two (sk and r - sk)"""
    rnd = random.Random(411)
    sks = [rnd.randrange(1, R) for _ in range(7)]
    return {"pk": [B.keygen(_sk(s))[1] for s in sks], "neg": [B.keygen(_sk(R - s))[1] for s in sks[:2]]}


def _run(emu, pks, items, lanes, cached=None, kst=None):
    nk, n = len(pks), len(items)
    flat = [k for ks in items for k in ks]
    off, at = [], 0
    for ks in items:
        off.append(at)
        at += len(ks)
    u32, i32 = ctypes.c_uint32, ctypes.c_int32
    st_d, st_r, same, mode = ((i32 * n)() for _ in range(4))
    flag = i32(-1)
    rc = emu.bh_ad_items(nk, b"".join(pks), bytes(cached or [1] * nk), (i32 * nk)(*(kst or [OK] * nk)), n,
                         (u32 * n)(*off), (u32 * n)(*[len(ks) for ks in items]), (u32 * len(flat))(*flat), lanes,
                         st_d, st_r, same, mode, ctypes.byref(flag))
    assert rc == 0
    return list(st_d), list(st_r), list(same), list(mode), flag.value


def _lists(nk, L, rnd):
    """list lengths 2, 3, L - 1, L, L + 1 and 7 over nk keys: a strictly ascending list and its
    reverse where the length fits the table, a list with repeats where it does not"""
    out = []
    for m in sorted({2, 3, L - 1, L, L + 1, 7}):
        if m <= nk:
            up = sorted(rnd.sample(range(nk), m))
            out += [up, up[::-1]]
        out.append([rnd.randrange(nk) for _ in range(m)])
    return out


@pytest.mark.parametrize("nk", [4, 7])
@pytest.mark.parametrize("lanes", LANES)
def test_sums_and_statuses_are_the_per_item_kernels(emu, keys, lanes, nk):
    rnd = random.Random(1000 * lanes + nk)
    items = _lists(nk, lanes, rnd)
    st_d, st_r, same, mode, flag = _run(emu, keys["pk"][:nk], items, lanes)
    assert flag == 1
    assert st_d == st_r == [OK] * len(items)
    assert same == [1] * len(items)
    for ks, m in zip(items, mode):
        strictly_up = all(a < b for a, b in zip(ks, ks[1:]))
        assert m == int(strictly_up and len(ks) > nk // 2), (ks, m)
    assert 1 in mode and 0 in mode


@pytest.mark.parametrize("lanes", LANES)
def test_path_choice_over_four_keys(emu, keys, lanes):
    """3-of-4 and 4-of-4 by complement (one absent key, none); 2-of-4, a descending list and a list
    naming one key twice directly, multiplicity kept"""
    items = [[0, 1, 3], [0, 1, 2, 3], [1, 2], [3, 1, 0], [0, 1, 1, 2], [2, 2]]
    st_d, st_r, same, mode, flag = _run(emu, keys["pk"][:4], items, lanes)
    assert flag == 1 and mode == [1, 1, 0, 0, 0, 0]
    assert st_d == st_r == [OK] * 6 and same == [1] * 6


@pytest.mark.parametrize("lanes", LANES)
def test_an_unregistered_key_in_the_table_clears_the_flag(emu, keys, lanes):
    items = [[0, 1, 3], [0, 1, 2, 3], [1, 3]]
    st_d, st_r, same, mode, flag = _run(emu, keys["pk"][:5], items, lanes, cached=[1, 1, 1, 1, 0])
    assert flag == 0 and mode == [0, 0, 0]
    assert st_d == st_r == [OK] * 3 and same == [1] * 3


@pytest.mark.parametrize("lanes", LANES)
def test_first_bad_key_in_list_order(emu, keys, lanes):
    """two slots with different bad statuses: the flag is clear, every item is direct and takes the
    status of the first bad key of its list"""
    items = [[0, 2, 1, 3], [0, 1, 2, 3], [3, 0], [0, 3, 3, 0, 3, 0, 2, 1, 0]]
    st_d, st_r, same, mode, flag = _run(emu, keys["pk"][:4], items, lanes, kst=[OK, NOT_ON_CURVE, NOT_IN_GROUP, OK])
    assert flag == 0 and mode == [0] * 4
    assert st_d == st_r == [NOT_IN_GROUP, NOT_ON_CURVE, OK, NOT_IN_GROUP]
    assert same == [1] * 4


@pytest.mark.parametrize("lanes", LANES)
def test_identity_sums(emu, keys, lanes):
    a, b = keys["pk"][:2]
    na, nb = keys["neg"]
    # {a, -a, b}: signed by {a, -a} (the complement b equals the total), by {a, b}
    st_d, st_r, same, mode, _ = _run(emu, [a, na, b], [[0, 1], [0, 2]], lanes)
    assert mode == [1, 1] and st_d == st_r == [PK_INFINITY, OK] and same == [1, 1]
    # {a, -a} signed by both: an identity total and an empty complement
    st_d, st_r, same, mode, _ = _run(emu, [a, na], [[0, 1]], lanes)
    assert mode == [1] and st_d == st_r == [PK_INFINITY] and same == [1]
    # {a, -a, b, -b} signed by {a, b, -b}: an identity total; and directly: a twice, a and -a mixed in
    st_d, st_r, same, mode, _ = _run(emu, [a, na, b, nb], [[0, 2, 3], [0, 0], [1, 0, 2, 0, 1]], lanes)
    assert mode == [1, 0, 0] and st_d == st_r == [OK, OK, OK] and same == [1, 1, 1]
    assert B.aggregate_pubkeys([a, b, nb])[1] == a


def test_lanes_and_split(emu):
    """the largest L of 4, 8, 16 that fills 65,536 lanes, else 4; a forced value only when it is one
    of the three; dense items have every key cached and at least two keys"""
    assert [emu.bh_ad_lanes(n, 0) for n in (1, 4095, 4096, 8191, 8192, 16383, 16384, 1 << 20)] == \
        [4, 4, 16, 16, 16, 16, 16, 16]
    assert [emu.bh_ad_lanes(n, 0) for n in (4096 - 1, 8192 - 1)] == [4, 16]
    assert [emu.bh_ad_lanes(100, f) for f in (4, 8, 16, 5, 32)] == [4, 8, 16, 4, 4]
    u32, i32 = ctypes.c_uint32, ctypes.c_int32
    kind = (i32 * 6)(*([-1] * 6))
    emu.bh_ad_split(6, (u32 * 6)(1, 1, 0, 1, 1, 0), (u32 * 6)(2, 1, 3, 0, 67, 1), kind)
    assert list(kind) == [1, 0, 0, 0, 1, 0]
    emu.bh_ad_split(6, None, (u32 * 6)(2, 1, 3, 0, 67, 1), kind)
    assert list(kind) == [0] * 6
