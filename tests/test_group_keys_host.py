"""The trait surface's grouping of a batch's keys (narwhal_amd/csrc/group_keys.h) on the host, with
no HIP, through the C interface of tests/hostemu/group_keys_stub.cpp: the distinct keys in order of
first occurrence, key_idx into them, byte equality, crafted keys, scratch reuse.
tests/test_gpu_grouped.py runs the same helper inside the library."""
import ctypes
import os
import subprocess
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "_build", "libgroupkeys.so")


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", ROOT, "tests/_build/libgroupkeys.so"], check=True)
    L = ctypes.CDLL(SO)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.gk_new.argtypes, L.gk_new.restype = [], vp
    L.gk_free.argtypes, L.gk_free.restype = [vp], None
    L.gk_group.argtypes, L.gk_group.restype = [vp, vp, u64, u64, vp, vp], ctypes.c_int64
    L.gk_group_tls.argtypes, L.gk_group_tls.restype = [vp, u64, vp, vp, vp], ctypes.c_int64
    L.gk_caps.argtypes, L.gk_caps.restype = [vp, vp], None
    L.gk_time_ns.argtypes, L.gk_time_ns.restype = [vp, vp, u64, u64, u64], ctypes.c_double
    return L


class Grouper:
    def __init__(self, lib):
        self.lib, self.h = lib, lib.gk_new()

    def close(self):
        self.lib.gk_free(self.h)

    def group(self, keys, max_distinct=0):
        """keys: list of 32-byte strings -> (distinct keys, key_idx), or None if it gave up"""
        n = len(keys)
        kb = np.frombuffer(b"".join(keys) + b"\0", dtype=np.uint8)
        idx = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
        out = np.zeros(32 * max(n, 1), dtype=np.uint8)
        m = self.lib.gk_group(self.h, kb.ctypes.data, n, max_distinct, idx.ctypes.data, out.ctypes.data)
        if m < 0:
            return None
        return [out[32 * j:32 * j + 32].tobytes() for j in range(m)], idx[:n].tolist()

    def caps(self):
        out = np.zeros(2, dtype=np.uint64)
        self.lib.gk_caps(self.h, out.ctypes.data)
        return int(out[0]), int(out[1])


@pytest.fixture
def g(lib):
    x = Grouper(lib)
    yield x
    x.close()


def reference(keys):
    """the distinct keys in order of first occurrence and the index of each key among them"""
    seen, distinct, idx = {}, [], []
    for k in keys:
        if k not in seen:
            seen[k] = len(distinct)
            distinct.append(k)
        idx.append(seen[k])
    return distinct, idx


def rand_keys(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]


def test_empty_and_single(g):
    assert g.group([]) == ([], [])
    k = rand_keys(1, 1)
    assert g.group(k) == (k, [0])


def test_all_equal(g):
    k = rand_keys(1, 2) * 300
    assert g.group(k) == (k[:1], [0] * 300)


def test_all_distinct(g):
    k = rand_keys(1000, 3)
    assert len(set(k)) == 1000
    assert g.group(k) == (k, list(range(1000)))


def test_committee_order_6800_over_100(g):
    """68 certificates of a 100-key committee, each signed by the same 100 keys in committee order"""
    c = rand_keys(100, 4)
    keys = c * 68
    distinct, idx = g.group(keys)
    assert distinct == c
    assert idx == list(range(100)) * 68


def test_first_occurrence_order(g):
    a, b, c, d = rand_keys(4, 5)
    keys = [c, a, c, d, a, b, d, c, b]
    assert g.group(keys) == ([c, a, d, b], [0, 1, 0, 2, 1, 3, 2, 0, 3])
    assert g.group(keys) == reference(keys)
    mixed = [rand_keys(37, 6)[i % 37] for i in np.random.default_rng(7).integers(0, 37, 500)]
    assert g.group(mixed) == reference(mixed)


def test_byte_equality_not_point_equality(g):
    """keys that differ only in the sign bit of x (byte 31's top bit) or only in byte 0 are
    different keys, whatever points they decode to"""
    k = bytearray(rand_keys(1, 8)[0])
    k[31] &= 0x7F
    hi = bytearray(k)
    hi[31] |= 0x80
    lo = bytearray(k)
    lo[0] ^= 0x01
    keys = [bytes(k), bytes(hi), bytes(lo), bytes(k), bytes(hi), bytes(lo)]
    assert g.group(keys) == ([bytes(k), bytes(hi), bytes(lo)], [0, 1, 2, 0, 1, 2])
    # y = 1 and its non-canonical encoding p + 1 decode to one point and are two keys
    one = (1).to_bytes(32, "little")
    one_nc = ((1 << 255) - 19 + 1).to_bytes(32, "little")
    assert g.group([one, one_nc, one]) == ([one, one_nc], [0, 1, 0])


def test_crafted_keys_stay_distinct_and_quick(g):
    """4,096 keys that share their first and last 8 bytes (what a hash of the ends alone would
    collide on) stay distinct, and the pass stays far below a second"""
    head, tail = b"\xAA" * 8, b"\x55" * 8
    keys = [head + i.to_bytes(8, "little") + (i * 0x9E3779B97F4A7C15 % (1 << 64)).to_bytes(8, "little") + tail
            for i in range(4096)]
    t0 = time.perf_counter()
    distinct, idx = g.group(keys)
    dt = time.perf_counter() - t0
    assert distinct == keys and idx == list(range(4096))
    assert dt < 0.25, dt
    # and only the middle byte differing
    keys = [head + bytes(8) + i.to_bytes(8, "big") + tail for i in range(4096)]
    assert g.group(keys + keys) == (keys, list(range(4096)) * 2)


def test_gives_up_past_the_limit(g):
    k = rand_keys(64, 9)
    assert g.group(k, max_distinct=32) is None
    assert g.group(k, max_distinct=64) == (k, list(range(64)))
    rep = k[:16] * 4
    assert g.group(rep, max_distinct=32) == (k[:16], list(range(16)) * 4)
    # a grouper that gave up is as good as new
    assert g.group(k) == (k, list(range(64)))


def test_scratch_reuse_across_sizes(g):
    """two calls on one grouper with different sizes: the second is right, and a call no larger
    than an earlier one leaves the scratch as it is (no allocation per call once grown)"""
    big = rand_keys(50, 10) * 40
    small = rand_keys(7, 11) * 3
    assert g.group(big) == reference(big)
    caps = g.caps()
    assert caps[0] >= 2 * len(big)
    assert g.group(small) == reference(small)
    assert g.caps() == caps
    assert g.group(big) == reference(big)
    assert g.caps() == caps
    # many calls: stale entries of earlier calls never come back to life
    for r in range(300):
        ks = rand_keys(5, 100 + r) * 2
        assert g.group(ks) == reference(ks)
    assert g.caps() == caps


def test_scratch_reuse_on_one_thread(lib):
    """the thread-local form, as the engine holds it"""
    caps = np.zeros(2, dtype=np.uint64)
    got = []
    for keys in (rand_keys(200, 12) * 5, rand_keys(3, 13) * 2, rand_keys(200, 12) * 5):
        n = len(keys)
        kb = np.frombuffer(b"".join(keys), dtype=np.uint8)
        idx = np.zeros(n, dtype=np.uint32)
        out = np.zeros(32 * n, dtype=np.uint8)
        m = lib.gk_group_tls(kb.ctypes.data, n, idx.ctypes.data, out.ctypes.data, caps.ctypes.data)
        assert ([out[32 * j:32 * j + 32].tobytes() for j in range(m)], idx.tolist()) == reference(keys)
        got.append(tuple(int(c) for c in caps))
    assert got[0] == got[1] == got[2]
