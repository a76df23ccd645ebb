"""The wave engine's batch check (one final exponentiation per group of items: bls_verify.h
wb_points / wb_sfold / wb_sig_item, wave::miller_script, w_ffold_step, w_group_final) compiled for
the host (tests/hostemu/bls_wave_batch_hostemu.cpp) and run on the CPU with the interpreter and
stage tables the kernels use.  A group must accept exactly when bls_ffi.fast_aggregate_verify
accepts every one of its items."""
import ctypes
import json
import os
import subprocess

import pytest

import bls_ffi as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = bytes(range(100, 132))


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(ROOT, "tests", "_build", "libblswbemu.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-C", ROOT, "tests/_build/libblswbemu.so"], check=True)
    L = ctypes.CDLL(path)
    c, sz = ctypes.c_char_p, ctypes.c_size_t
    L.bh_wb_group.argtypes = [sz, c, c, c, ctypes.POINTER(ctypes.c_int), c, c, sz, ctypes.c_int, ctypes.c_uint32]
    L.bh_wb_script_is_prefix.argtypes = [ctypes.c_int]
    L.bh_wb_script_len.argtypes = [ctypes.c_int]
    return L


@pytest.fixture(scope="module")
def items():
    """five items over the golden keys (the fifth on the first key again), each a signature of
    its own 32-byte message: (sig, pk, msg)"""
    with open(os.path.join(ROOT, "tests", "golden", "bls12381_kats.json")) as f:
        gold = json.load(f)
    out = []
    for i in range(5):
        k = gold["keygen"][i % len(gold["keygen"])]
        m = bytes([i + 1]) * 32
        out.append((B.sign(bytes.fromhex(k["sk"]), m), bytes.fromhex(k["pk"]), m))
    assert len(out) == 5
    return out


def _neg(sig):
    """-P of a compressed G1 point: the encoding's sign bit flipped"""
    b = bytearray(sig)
    b[0] ^= 0x20
    return bytes(b)


def _group(emu, its, modes=None, script_len=-1, fan=0, seed=SEED):
    n = len(its)
    modes = modes or [0] * n
    return emu.bh_wb_group(n, b"".join(i[0] for i in its), b"".join(i[1] for i in its), b"".join(i[2] for i in its),
                           (ctypes.c_int * n)(*modes), seed, B.DST_NUL, len(B.DST_NUL), script_len, fan)


def _oracle_all(its):
    return all(B.fast_aggregate_verify(s, [pk], m) == 0 for s, pk, m in its)


@pytest.mark.parametrize("fixed", [0, 1])
def test_miller_script_is_pairing_script_prefix(emu, fixed):
    """both line modes: the same ops up to pairing_script's P_CONJ_F, all 68 LINES steps, no
    inversion, next_run links that stay inside the cut script"""
    assert emu.bh_wb_script_is_prefix(fixed) == 1
    assert emu.bh_wb_script_len(fixed) > 0


@pytest.mark.parametrize("n", [1, 2, 5])
def test_group_accepts_valid_items(emu, items, n):
    its = items[:n]
    assert _oracle_all(its)
    assert _group(emu, its) == 1


def test_group_accepts_every_line_and_clearing_mode(emu, items):
    """computed lines, a key's line table, and the key-side form (H0 not cofactor-cleared, the key
    record [h_eff] pk with its line table: [r] is applied to H0) side by side in one group, and
    a tree of two records a step (three levels over six records)"""
    assert _group(emu, items, modes=[0, 1, 2, 2, 1]) == 1
    assert _group(emu, items[:3], modes=[2, 0, 1], fan=2) == 1
    assert _group(emu, items, fan=2) == 1


@pytest.mark.parametrize("n,bad", [(1, 0), (2, 1), (5, 2)])
def test_group_rejects_one_invalid_item(emu, items, n, bad):
    its = list(items[:n])
    s, pk, m = its[bad]
    its[bad] = (s, pk, bytes([0xEE]) * 32)  # a wrong message
    assert not _oracle_all(its)
    assert _group(emu, its) == 0
    assert _group(emu, its, modes=[2] * n) == 0


def test_group_rejects_cancelling_pair(emu, items):
    """sig_a + D and sig_b - D: the unweighted product of the items' equations is 1, the weighted
    one is not"""
    its = list(items)
    D = items[4][0]
    a, b = 1, 3
    rc, sa = B.aggregate([its[a][0], D])
    assert rc == 0
    rc, sb = B.aggregate([its[b][0], _neg(D)])
    assert rc == 0
    its[a] = (sa, its[a][1], its[a][2])
    its[b] = (sb, its[b][1], its[b][2])
    assert B.fast_aggregate_verify(*[its[a][0], [its[a][1]], its[a][2]]) == B.ORB_VERIFY_FAIL
    assert B.fast_aggregate_verify(*[its[b][0], [its[b][1]], its[b][2]]) == B.ORB_VERIFY_FAIL
    # the two signatures still sum to sig_a + sig_b
    assert B.aggregate([sa, sb])[1] == B.aggregate([items[a][0], items[b][0]])[1]
    assert _group(emu, its) == 0
    assert _group(emu, its, modes=[1, 2, 0, 2, 1]) == 0
    assert _group(emu, [its[a], its[b]]) == 0


def test_group_rejects_when_script_is_empty_or_cut(emu, items):
    """fail closed: a Miller pass that finds no script (or stops before its last step) leaves F
    records that count no Miller output, and the group's last wave rejects"""
    assert _group(emu, items[:2], script_len=0) == 0
    assert _group(emu, items[:1], script_len=0) == 0
    assert _group(emu, items[:2], script_len=emu.bh_wb_script_len(0) - 2) == 0
