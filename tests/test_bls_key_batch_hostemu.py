"""The key-transposed batch check (bls_key_batch.h's plan, bls_verify.h's stages, the wave engine's
Miller script and product tree) compiled for the host (tests/hostemu/bls_key_batch_hostemu.cpp) and
run on the CPU.  Two groups with one-key items and certificates side by side: each group's Fp12
value after the final exponentiation must equal the product of its items' own pairing values
raised to their coefficients (computed item by item with the scalar code), and a group accepts
exactly when bls_ffi.fast_aggregate_verify accepts every one of its items."""
import ctypes
import json
import os
import subprocess

import pytest

import bls_ffi as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = bytes(range(40, 72))
GROUP = 4


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(ROOT, "tests", "_build", "libblskbemu.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-C", ROOT, "tests/_build/libblskbemu.so"], check=True)
    L = ctypes.CDLL(path)
    c, sz, u32p, i32p = ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
    L.bh_kb_groups.argtypes = [sz, c, sz, c, u32p, u32p, u32p, c, c, c, sz, ctypes.c_uint32, ctypes.c_uint32,
                               ctypes.c_int, i32p, i32p, i32p, u32p]
    return L


@pytest.fixture(scope="module")
def call():
    """three keys; seven items, groups of four: one-key items and certificates in both groups, a
    certificate that names key 0 twice, key 1 on three different messages, one message signed by
    two different keys (items 1 and 5): (sig, key numbers, msg)"""
    with open(os.path.join(ROOT, "tests", "golden", "bls12381_kats.json")) as f:
        gold = json.load(f)["keygen"][:3]
    sks = [bytes.fromhex(k["sk"]) for k in gold]
    pks = [bytes.fromhex(k["pk"]) for k in gold]
    who = [[0], [1], [0, 1, 2], [1], [0, 2, 0], [2], [1, 2]]
    msgs = [bytes([i + 1]) * 32 for i in range(7)]
    msgs[5] = msgs[1]
    items = []
    for ks, m in zip(who, msgs):
        rc, agg = B.aggregate([B.sign(sks[k], m) for k in ks])
        assert rc == 0
        items.append((agg, ks, m))
    return pks, items


def _run(emu, pks, items, skew=-1, fan=0):
    n = len(items)
    flat = [k for _, ks, _ in items for k in ks]
    off, at = [], 0
    for _, ks, _ in items:
        off.append(at)
        at += len(ks)
    u32 = ctypes.c_uint32
    ng_max = (n + GROUP - 1) // GROUP
    verdict, same, one = ((ctypes.c_int32 * ng_max)() for _ in range(3))
    mill = (u32 * ng_max)()
    ng = emu.bh_kb_groups(n, b"".join(i[0] for i in items), len(pks), b"".join(pks), (u32 * n)(*off),
                          (u32 * n)(*[len(i[1]) for i in items]), (u32 * len(flat))(*flat),
                          b"".join(i[2] for i in items), SEED, B.DST_NUL, len(B.DST_NUL), GROUP, fan, skew,
                          verdict, same, one, mill)
    assert ng == ng_max
    return list(verdict), list(same), list(one), list(mill)


def _oracle_groups(pks, items):
    ok = [B.fast_aggregate_verify(s, [pks[k] for k in ks], m) == 0 for s, ks, m in items]
    return [int(all(ok[lo:lo + GROUP])) for lo in range(0, len(items), GROUP)]


@pytest.mark.parametrize("fan", [0, 2])
def test_groups_equal_the_items_weighted_product(emu, call, fan):
    """all valid: both groups accept, each value equals prod t_i^{r_i} (which is 1), and a group
    over K distinct keys ran K + 1 Miller entries; fan 2: a tree of three levels"""
    pks, items = call
    assert _oracle_groups(pks, items) == [1, 1]
    verdict, same, one, mill = _run(emu, pks, items, fan=fan)
    assert verdict == [1, 1] and same == [1, 1] and one == [1, 1]
    assert mill == [4, 4]  # keys {0, 1, 2} + 1 in the first group, {0, 2, 1} + 1 in the second


def test_a_forged_item_moves_its_group_to_the_same_value_as_the_items(emu, call):
    """item 4 (the certificate that names key 0 twice) on another message: its group rejects, and
    its value is still the product of the items' values raised to their coefficients, not 1"""
    pks, items = call
    its = list(items)
    s, ks, m = its[4]
    its[4] = (s, ks, bytes([0xEE]) * 32)
    assert _oracle_groups(pks, its) == [1, 0]
    verdict, same, one, _ = _run(emu, pks, its)
    assert verdict == [1, 0] and same == [1, 1] and one == [1, 0]


@pytest.mark.parametrize("skew", [2, 5])
def test_coefficient_on_the_hash_side_only_flips_the_verdict(emu, call, skew):
    """r_i must multiply the item's signature as well as its hash contributions: with the
    signature of one valid item (a certificate, a one-key item) entering unweighted, its group
    rejects and its value leaves the items' product"""
    pks, items = call
    verdict, same, one, _ = _run(emu, pks, items, skew=skew)
    g = skew // GROUP
    assert one == [1, 1]
    assert verdict[g] == 0 and same[g] == 0
    assert verdict[1 - g] == 1 and same[1 - g] == 1


def test_swapped_signers_on_one_message_reject(emu, call):
    """item A carries key 0's signature and names key 1, item B the reverse, on one message in one
    group: the product without coefficients is 1, the weighted one is not"""
    pks, items = call
    with open(os.path.join(ROOT, "tests", "golden", "bls12381_kats.json")) as f:
        gold = json.load(f)["keygen"][:2]
    m = bytes([0x5A]) * 32
    s0, s1 = (B.sign(bytes.fromhex(k["sk"]), m) for k in gold)
    its = [(s0, [1], m), (s1, [0], m)] + list(items[2:4])
    assert B.fast_aggregate_verify(B.aggregate([s0, s1])[1], [pks[1], pks[0]], m) == 0  # unweighted: holds
    assert _oracle_groups(pks, its) == [0]
    verdict, same, one, _ = _run(emu, pks, its)
    assert verdict == [0] and same == [1] and one == [0]
