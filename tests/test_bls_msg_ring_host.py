"""The BLS message ring's bookkeeping (narwhal_amd/csrc/bls_msg_ring.h) on the host, with no HIP:
lookups, pins, reservations, publishes and the FIFO cursor through the C interface of
tests/hostemu/bls_msg_ring_stub.cpp, against a Python model.  tests/test_gpu_bls_msg_ring.py runs
the same bookkeeping inside the library, with the device records behind it."""
import ctypes
import os
import random
import subprocess
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "_build", "libblsmsgring.so")
STUB = os.path.join(ROOT, "tests", "hostemu", "bls_msg_ring_stub.cpp")
NONE = 0xFFFFFFFF
DST = b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_"


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", ROOT, "tests/_build/libblsmsgring.so"], check=True)
    L = ctypes.CDLL(SO)
    vp, u64, u32, i32, cp = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_char_p
    key = [cp, u64, cp, u64]
    L.bmr_new.argtypes, L.bmr_new.restype = [u32, i32], vp
    L.bmr_free.argtypes, L.bmr_free.restype = [vp], None
    L.bmr_cacheable.argtypes, L.bmr_cacheable.restype = [u64, u64], i32
    L.bmr_lookup_pin.argtypes, L.bmr_lookup_pin.restype = [vp] + key, u32
    L.bmr_contains.argtypes, L.bmr_contains.restype = [vp] + key, i32
    L.bmr_reserve.argtypes, L.bmr_reserve.restype = [vp], u32
    L.bmr_publish.argtypes, L.bmr_publish.restype = [vp, u32] + key, u32
    L.bmr_release.argtypes, L.bmr_release.restype = [vp, u32], None
    L.bmr_unpin.argtypes, L.bmr_unpin.restype = [vp, u32], None
    L.bmr_counts.argtypes, L.bmr_counts.restype = [vp, vp], None
    L.bmr_slot_state.argtypes, L.bmr_slot_state.restype = [vp, u32], u32
    L.bmr_hash.argtypes, L.bmr_hash.restype = key, u64
    L.bmr_race.argtypes, L.bmr_race.restype = [vp, i32, i32, vp], None
    return L


class Ring:
    def __init__(self, lib, cap, lg=-1):
        self.lib, self.cap = lib, cap
        self.h = lib.bmr_new(cap, lg)

    def close(self):
        self.lib.bmr_free(self.h)

    @staticmethod
    def _k(key):
        dst, msg = key
        return dst, len(dst), msg, len(msg)

    def lookup_pin(self, key):
        return self.lib.bmr_lookup_pin(self.h, *self._k(key))

    def contains(self, key):
        return bool(self.lib.bmr_contains(self.h, *self._k(key)))

    def reserve(self):
        return self.lib.bmr_reserve(self.h)

    def publish(self, slot, key):
        return self.lib.bmr_publish(self.h, slot, *self._k(key))

    def release(self, slot):
        self.lib.bmr_release(self.h, slot)

    def unpin(self, slot):
        self.lib.bmr_unpin(self.h, slot)

    def counts(self):
        out = np.zeros(3, dtype=np.uint64)
        self.lib.bmr_counts(self.h, out.ctypes.data)
        return tuple(int(x) for x in out)

    def state(self, slot):
        s = self.lib.bmr_slot_state(self.h, slot)
        return bool(s & 1), bool(s & 2), s >> 8


@pytest.fixture
def ring(lib):
    made = []

    def make(cap, lg=-1):
        made.append(Ring(lib, cap, lg))
        return made[-1]
    yield make
    for r in made:
        r.close()


def key(i, dst=DST):
    return dst, (b"digest-%06d" % i).ljust(32, b".")


@pytest.mark.parametrize("cap", [1, 2, 7])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_operations_match_a_model(ring, cap, seed):
    """lookup_pin / reserve / publish / release / unpin in seeded random order against a model:
    key -> slot and slot -> key as dicts, busy as a set, pins as a dict, the cursor as an index."""
    rng = random.Random(1000 * cap + seed)
    r = ring(cap)
    slot_of, key_of, busy, pins = {}, {}, set(), {}
    held_pins = []          # (slot) one entry per pin taken
    cursor = 0
    nkeys = 2 * cap + 3
    full_seen = reuse_seen = 0
    for step in range(4000):
        op = rng.choice(("lookup", "lookup", "reserve", "reserve", "publish", "publish", "release", "unpin", "unpin"))
        if op == "lookup":
            k = rng.randrange(nkeys)
            got = r.lookup_pin(key(k))
            assert got == slot_of.get(k, NONE), "only published keys are found, at their slot"
            if got != NONE:
                pins[got] = pins.get(got, 0) + 1
                held_pins.append(got)
        elif op == "reserve":
            got = r.reserve()
            want = NONE
            for j in range(cap):
                t = (cursor + j) % cap
                if t not in busy and not pins.get(t, 0):
                    want = t
                    break
            assert got == want, "the first slot from the cursor that is neither busy nor pinned"
            if got == NONE:
                assert all(t in busy or pins.get(t, 0) for t in range(cap))
                full_seen += 1
            else:
                assert got not in busy and not pins.get(got, 0), "a busy or pinned slot is never handed out"
                if got in key_of:       # unmapped
                    del slot_of[key_of.pop(got)]
                    reuse_seen += 1
                busy.add(got)
                cursor = (got + 1) % cap
        elif op == "publish" and busy:
            s = rng.choice(sorted(busy))
            k = rng.randrange(nkeys)
            got = r.publish(s, key(k))
            busy.discard(s)
            if k in slot_of:            # published meanwhile by another call: one mapping stays
                assert got == slot_of[k] and got != s
            else:
                assert got == s
                slot_of[k] = s
                key_of[s] = k
        elif op == "release" and busy:
            s = rng.choice(sorted(busy))
            r.release(s)
            busy.discard(s)
        elif op == "unpin" and held_pins:
            s = held_pins.pop(rng.randrange(len(held_pins)))
            r.unpin(s)
            pins[s] -= 1
        else:
            continue
        # the whole state against the model, every step
        assert len(set(slot_of.values())) == len(slot_of), "a key maps to at most one slot"
        for t in range(cap):
            assert r.state(t) == (t in key_of, t in busy, pins.get(t, 0))
        for k in range(nkeys):
            assert r.contains(key(k)) == (k in slot_of)
        assert r.counts() == (len(key_of), len(busy), sum(1 for t in range(cap) if pins.get(t, 0)))
    assert full_seen > 0 and reuse_seen > 0
    # after release and unpin every slot is reusable
    for s in sorted(busy):
        r.release(s)
    for s in held_pins:
        r.unpin(s)
    got = sorted(r.reserve() for _ in range(cap))
    assert got == list(range(cap)) and r.reserve() == NONE
    assert r.counts() == (0, cap, 0)


def test_reserve_with_every_slot_busy_or_pinned_returns_none(ring):
    r = ring(3)
    a, b, c = r.reserve(), r.reserve(), r.reserve()
    assert (a, b, c) == (0, 1, 2) and r.reserve() == NONE
    assert r.publish(a, key(1)) == a and r.publish(b, key(2)) == b
    assert r.lookup_pin(key(1)) == a and r.lookup_pin(key(2)) == b      # two pinned, one busy
    assert r.reserve() == NONE
    r.unpin(a)
    assert r.reserve() == a and not r.contains(key(1))                   # the unpinned one, unmapped
    assert r.reserve() == NONE
    r.unpin(b)
    r.release(c)
    assert r.reserve() == b and r.reserve() == c                         # FIFO order from the cursor


def test_fifo_keeps_the_newest(ring):
    r = ring(4)
    for k in range(6):
        s = r.reserve()
        assert s == k % 4
        assert r.publish(s, key(k)) == s
    assert [r.contains(key(k)) for k in range(6)] == [False, False, True, True, True, True]


def test_two_publishers_of_one_key_keep_one_mapping(ring):
    r = ring(4)
    a, b = r.reserve(), r.reserve()
    assert r.publish(b, key(5)) == b
    assert r.publish(a, key(5)) == b, "the later publisher is told the slot that stays"
    assert r.state(a) == (False, False, 0) and r.counts() == (1, 0, 0)
    assert r.lookup_pin(key(5)) == b


def test_keys_in_one_bucket_and_near_keys_stay_distinct(ring, lib):
    """lg_buckets = 0 puts every key into the table's one bucket; keys that differ only in dst, only
    in a length, or only in the last byte are different keys"""
    r = ring(8, 0)
    msg = bytes(range(32))
    keys = [(DST, msg),
            (DST[:-1] + b"X", msg),                # only the dst differs
            (DST, msg[:-1] + bytes([msg[-1] ^ 1])),  # only the last byte
            (DST, msg[:-1]),                       # only the length: a prefix ...
            (DST, msg + b"\0"),                    # ... and a zero-padded extension
            (DST[:-1], msg),                       # a shorter dst
            (DST + msg[:1], msg[1:]),              # the same bytes, split elsewhere
            (b"", b"")]
    slots = []
    for k in keys:
        s = r.reserve()
        assert r.publish(s, k) == s
        slots.append(s)
    assert sorted(slots) == list(range(8))
    for k, s in zip(keys, slots):
        assert r.lookup_pin(k) == s
        r.unpin(s)
    assert not r.contains((DST, msg + b"\1"))
    # (the table hash is salted per process: equal keys hash equal, and the salt is not the identity)
    assert lib.bmr_hash(DST, len(DST), msg, 32) == lib.bmr_hash(DST, len(DST), msg, 32)
    assert len({lib.bmr_hash(*Ring._k(k)) for k in keys}) == len(keys)


def test_the_length_limits(lib):
    assert lib.bmr_cacheable(43, 32) and lib.bmr_cacheable(64, 64) and lib.bmr_cacheable(0, 0)
    assert not lib.bmr_cacheable(43, 65), "a 65-byte message is not cached"
    assert not lib.bmr_cacheable(65, 32)


def test_two_readers_against_two_writers(lib, ring):
    r = ring(4)
    out = np.zeros(4, dtype=np.uint64)
    t = threading.Thread(target=lib.bmr_race, args=(r.h, 9, 20000, out.ctypes.data))  # (ctypes drops the GIL)
    t.start()
    t.join(120)
    assert not t.is_alive()
    hits, bad, pubs, full = (int(x) for x in out)
    print("hits %d, wrong reads %d, publishes %d, full %d" % (hits, bad, pubs, full))
    assert bad == 0 and pubs > 0
    assert r.counts()[1:] == (0, 0)


def test_the_race_is_clean_under_the_thread_sanitizer(tmp_path):
    """bls_msg_ring_stub.cpp as a stand-alone program (its own main), built with -fsanitize=thread
    and run on the CPU; never loaded into Python.  Sanitizer runs stay off machines with a GPU
    (skipped where the compute device node exists); also skipped where the compiler cannot link the
    sanitizer's runtime or the runtime cannot map its shadow memory on this kernel."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer runs are for CPU-only machines")
    exe = str(tmp_path / "blsmr_tsan")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=thread", "-DBLSMR_STUB_MAIN",
                        "-o", exe, STUB], capture_output=True, text=True, timeout=300)
    if b.returncode != 0:
        pytest.skip("cannot build with -fsanitize=thread here: " + b.stderr[-300:])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if "unexpected memory mapping" in p.stderr:
        pytest.skip("the thread sanitizer's runtime cannot start on this kernel")
    print(p.stdout.strip())
    assert p.returncode == 0 and "WARNING: ThreadSanitizer" not in p.stderr, p.stdout + p.stderr[-3000:]
    assert "0 wrong reads" in p.stdout and ", ok" in p.stdout
