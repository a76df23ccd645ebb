"""The BLS aggregate-key ring's bookkeeping (narwhal_amd/csrc/bls_apk_ring.h) on the host, with no
HIP: lookups, pins, the second-sighting filter, reservations, publishes, the FIFO cursor and the
epoch reset through the C interface of tests/hostemu/bls_apk_ring_stub.cpp, against a Python model.
tests/test_gpu_bls_apk_ring.py runs the same bookkeeping inside the library, with the device records
behind it."""
import ctypes
import os
import random
import subprocess
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "_build", "libblsapkring.so")
STUB = os.path.join(ROOT, "tests", "hostemu", "bls_apk_ring_stub.cpp")
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", ROOT, "tests/_build/libblsapkring.so"], check=True)
    L = ctypes.CDLL(SO)
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    key = [vp, u64]
    L.bar_new.argtypes, L.bar_new.restype = [u32, i32], vp
    L.bar_free.argtypes, L.bar_free.restype = [vp], None
    L.bar_eligible.argtypes, L.bar_eligible.restype = [u64], i32
    L.bar_lookup_pin.argtypes, L.bar_lookup_pin.restype = [vp] + key, u32
    L.bar_contains.argtypes, L.bar_contains.restype = [vp] + key, i32
    L.bar_miss.argtypes, L.bar_miss.restype = [vp] + key + [vp], u32
    L.bar_reserve.argtypes, L.bar_reserve.restype = [vp], u32
    L.bar_publish.argtypes, L.bar_publish.restype = [vp, u32] + key, u32
    L.bar_release.argtypes, L.bar_release.restype = [vp, u32], None
    L.bar_unpin.argtypes, L.bar_unpin.restype = [vp, u32], None
    L.bar_reset.argtypes, L.bar_reset.restype = [vp], None
    L.bar_counts.argtypes, L.bar_counts.restype = [vp, vp], None
    L.bar_slot_state.argtypes, L.bar_slot_state.restype = [vp, u32], u32
    L.bar_filter_used.argtypes, L.bar_filter_used.restype = [vp], u64
    L.bar_hash.argtypes, L.bar_hash.restype = key, u64
    L.bar_filter_entry.argtypes, L.bar_filter_entry.restype = [vp] + key, u64
    L.bar_race.argtypes, L.bar_race.restype = [vp, i32, i32, vp], None
    return L


def _k(idx):
    a = np.asarray(list(idx), dtype=np.uint32)
    return a, (a.ctypes.data, len(a))


class Ring:
    def __init__(self, lib, cap, lg=-1):
        self.lib, self.cap = lib, cap
        self.h = lib.bar_new(cap, lg)

    def close(self):
        self.lib.bar_free(self.h)

    def lookup_pin(self, idx):
        a, k = _k(idx)
        return self.lib.bar_lookup_pin(self.h, *k)

    def contains(self, idx):
        a, k = _k(idx)
        return bool(self.lib.bar_contains(self.h, *k))

    def miss(self, idx):
        """(slot or NONE, noted)"""
        a, k = _k(idx)
        noted = ctypes.c_int(0)
        s = self.lib.bar_miss(self.h, *k, ctypes.addressof(noted))
        return s, bool(noted.value)

    def reserve(self):
        return self.lib.bar_reserve(self.h)

    def publish(self, slot, idx):
        a, k = _k(idx)
        return self.lib.bar_publish(self.h, slot, *k)

    def release(self, slot):
        self.lib.bar_release(self.h, slot)

    def unpin(self, slot):
        self.lib.bar_unpin(self.h, slot)

    def reset(self):
        self.lib.bar_reset(self.h)

    def counts(self):
        out = np.zeros(3, dtype=np.uint64)
        self.lib.bar_counts(self.h, out.ctypes.data)
        return tuple(int(x) for x in out)

    def state(self, slot):
        s = self.lib.bar_slot_state(self.h, slot)
        return bool(s & 1), bool(s & 2), s >> 8

    def filter_used(self):
        return int(self.lib.bar_filter_used(self.h))

    def hash(self, idx):
        a, k = _k(idx)
        return int(self.lib.bar_hash(*k))

    def entry(self, idx):
        a, k = _k(idx)
        return int(self.lib.bar_filter_entry(self.h, *k))


@pytest.fixture
def ring(lib):
    made = []

    def make(cap, lg=-1):
        made.append(Ring(lib, cap, lg))
        return made[-1]
    yield make
    for r in made:
        r.close()


def sset(i):
    """set i of the model's universe: three indices, written out of order"""
    return [i + 7, i, 2 * i + 1]


@pytest.mark.parametrize("cap", [1, 2, 8])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_operations_match_a_model(ring, cap, seed):
    """lookup_pin / miss / reserve / publish / release / unpin / reset in seeded random order
    against a model: set -> slot and slot -> set as dicts, busy as a set, pins as a dict, the cursor
    as an index, the filter as entry -> hash (entries and hashes read from the stub: the hash is
    salted per process)."""
    rng = random.Random(1000 * cap + seed)
    r = ring(cap)
    slot_of, key_of, busy, pins, filt = {}, {}, set(), {}, {}
    held_pins = []
    cursor = 0
    nsets = 2 * cap + 3
    hh = {k: r.hash(sset(k)) for k in range(nsets)}
    ee = {k: r.entry(sset(k)) for k in range(nsets)}
    assert all(e == hh[k] % (4 * cap) for k, e in ee.items()), "4 x slots entries, direct mapped"
    seen = dict(full=0, reuse=0, noted=0, filled=0, reset=0)

    def model_reserve():
        nonlocal cursor
        for j in range(cap):
            t = (cursor + j) % cap
            if t not in busy and not pins.get(t, 0):
                if t in key_of:
                    del slot_of[key_of.pop(t)]
                    seen["reuse"] += 1
                busy.add(t)
                cursor = (t + 1) % cap
                return t
        seen["full"] += 1
        return NONE

    ops = ("lookup", "lookup", "miss", "miss", "miss", "reserve", "publish", "publish", "release", "unpin", "unpin")
    for step in range(4000):
        op = rng.choice(ops) if rng.randrange(400) else "reset"
        if op == "lookup":
            k = rng.randrange(nsets)
            idx = sset(k)
            rng.shuffle(idx)
            got = r.lookup_pin(idx)
            assert got == slot_of.get(k, NONE), "only published sets are found, at their slot"
            if got != NONE:
                pins[got] = pins.get(got, 0) + 1
                held_pins.append(got)
        elif op == "miss":
            k = rng.randrange(nsets)
            if k in slot_of:
                continue        # (the engine calls miss only after a lookup found nothing)
            got, noted = r.miss(sset(k))
            if filt.get(ee[k]) == hh[k]:
                assert not noted
                assert got == model_reserve()
                seen["filled"] += got != NONE
            else:
                assert noted and got == NONE, "a first sighting never reserves"
                filt[ee[k]] = hh[k]
                seen["noted"] += 1
        elif op == "reserve":
            assert r.reserve() == model_reserve()
        elif op == "publish" and busy:
            s = rng.choice(sorted(busy))
            k = rng.randrange(nsets)
            got = r.publish(s, sset(k))
            busy.discard(s)
            if k in slot_of:
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
        elif op == "reset":
            # (the engine resets with no call in flight; busy and pinned slots of the model stand
            # for abandoned ones and stay as they are)
            r.reset()
            slot_of.clear()
            key_of.clear()
            filt.clear()
            cursor = 0
            seen["reset"] += 1
        else:
            continue
        assert len(set(slot_of.values())) == len(slot_of), "a set maps to at most one slot"
        for t in range(cap):
            assert r.state(t) == (t in key_of, t in busy, pins.get(t, 0))
        for k in range(nsets):
            assert r.contains(sset(k)) == (k in slot_of)
        assert r.counts() == (len(key_of), len(busy), sum(1 for t in range(cap) if pins.get(t, 0)))
        assert r.filter_used() == len(filt)
    assert all(v > 0 for v in seen.values()), seen
    for s in sorted(busy):
        r.release(s)
    for s in held_pins:
        r.unpin(s)
    got = sorted(r.reserve() for _ in range(cap))
    assert got == list(range(cap)) and r.reserve() == NONE
    assert r.counts() == (0, cap, 0)


def test_keys_are_sorted_multisets(ring):
    r = ring(8, 0)          # (one bucket: every lookup walks every published set)
    a, b, c = 5, 9, 70000
    s = r.reserve()
    assert r.publish(s, [a, b, c]) == s
    for perm in ([a, b, c], [c, b, a], [b, a, c], [b, c, a]):
        assert r.lookup_pin(perm) == s, "order does not matter"
        r.unpin(s)
    for other in ([a, b], [a, a, b], [a, b, b, c], [a, b, c, c], [a, b, c + 1], [a, a, b, c]):
        assert not r.contains(other)
    s2 = r.reserve()
    assert r.publish(s2, [a, a, b]) == s2
    s3 = r.reserve()
    assert r.publish(s3, [b, a]) == s3 and s3 != s2, "[a, a, b] is not [a, b]: the sums differ"
    assert r.lookup_pin([a, b, a]) == s2 and r.lookup_pin([a, b]) == s3
    assert len({r.hash([a, a, b]), r.hash([a, b]), r.hash([a, b, b])}) == 3
    assert r.hash([a, b, c]) == r.hash([c, a, b])


def test_the_length_limits(lib, ring):
    assert not lib.bar_eligible(0) and not lib.bar_eligible(1), "a one-key item has its key's own table"
    assert lib.bar_eligible(2) and lib.bar_eligible(1024)
    assert not lib.bar_eligible(1025)
    r = ring(2)
    big = list(range(1024))
    s = r.reserve()
    assert r.publish(s, big) == s
    assert r.lookup_pin(big[::-1]) == s
    assert not r.contains(big[:-1] + [2000]) and not r.contains(big[:-1])


def _apart(r, n):
    """n sets in n different filter entries (the hash is salted per process)"""
    got, used = [], set()
    for k in range(1000):
        if r.entry(sset(k)) not in used:
            used.add(r.entry(sset(k)))
            got.append(k)
            if len(got) == n:
                return got
    raise AssertionError("fewer than %d entries reached" % n)


def test_first_sighting_never_reserves_and_the_second_does(ring):
    r = ring(4)
    ks = _apart(r, 3)
    for k in ks:
        assert r.miss(sset(k)) == (NONE, True)
        assert r.counts() == (0, 0, 0)
    assert r.miss(sset(ks[0])) == (0, False)
    assert r.counts() == (0, 1, 0)
    assert r.publish(0, sset(ks[0])) == 0
    assert r.lookup_pin(sset(ks[0])) == 0


def _colliding(r, n_entries):
    """two sets in one filter entry, and a third elsewhere"""
    by = {}
    for k in range(200):
        e = r.entry(sset(k))
        by.setdefault(e, []).append(k)
        if len(by[e]) == 2:
            a, b = by[e]
            c = next(j for j in range(200) if r.entry(sset(j)) != e)
            return a, b, c
    raise AssertionError("no collision among 200 sets in %d entries" % n_entries)


def test_a_bucket_collision_changes_only_when_a_fill_happens(ring):
    r = ring(1)             # 4 filter entries
    a, b, c = _colliding(r, 4)
    assert r.hash(sset(a)) != r.hash(sset(b))
    assert r.miss(sset(a)) == (NONE, True)
    assert r.miss(sset(b)) == (NONE, True), "b pushed a's hash out of the shared entry"
    assert r.miss(sset(a)) == (NONE, True), "so a's second sighting looks like a first: the fill comes later"
    s, noted = r.miss(sset(a))
    assert (s, noted) == (0, False)
    assert r.publish(s, sset(a)) == s
    # lookups are keyed on the whole list: b, in a's entry, is not found under a's slot
    assert r.lookup_pin(sset(b)) == NONE and r.lookup_pin(sset(a)) == 0
    r.unpin(0)
    assert r.miss(sset(c)) == (NONE, True), "another entry is untouched by all this"


def test_reserve_with_every_slot_busy_or_pinned_returns_none(ring):
    r = ring(3)
    a, b, c = r.reserve(), r.reserve(), r.reserve()
    assert (a, b, c) == (0, 1, 2) and r.reserve() == NONE
    assert r.publish(a, sset(1)) == a and r.publish(b, sset(2)) == b
    assert r.lookup_pin(sset(1)) == a and r.lookup_pin(sset(2)) == b      # two pinned, one busy
    assert r.reserve() == NONE
    assert r.miss(sset(3)) == (NONE, True)
    assert r.miss(sset(3)) == (NONE, False), "a second sighting with no free slot just computes"
    r.unpin(a)
    assert r.reserve() == a and not r.contains(sset(1))
    assert r.reserve() == NONE
    r.unpin(b)
    r.release(c)
    assert r.reserve() == b and r.reserve() == c


def test_two_publishers_of_one_set_keep_one_mapping(ring):
    r = ring(4)
    a, b = r.reserve(), r.reserve()
    assert r.publish(b, [3, 1, 2]) == b
    assert r.publish(a, [1, 2, 3]) == b, "the later publisher is told the slot that stays"
    assert r.state(a) == (False, False, 0) and r.counts() == (1, 0, 0)
    assert r.lookup_pin([2, 3, 1]) == b


def test_reset_drops_everything_the_filter_included(ring):
    r = ring(4)
    ks = _apart(r, 4)
    for k in ks[:3]:
        assert r.miss(sset(k)) == (NONE, True)
        s, noted = r.miss(sset(k))
        assert not noted and r.publish(s, sset(k)) == s
    assert r.miss(sset(ks[3])) == (NONE, True)
    assert r.counts() == (3, 0, 0) and r.filter_used() == 4
    r.reset()
    assert r.counts() == (0, 0, 0) and r.filter_used() == 0
    for k in ks:
        assert not r.contains(sset(k))
        assert r.miss(sset(k)) == (NONE, True), "after a reset every set is a first sighting again"
    assert r.miss(sset(ks[0])) == (0, False), "and the cursor starts over"


def test_two_readers_against_two_writers(lib, ring):
    r = ring(4)
    out = np.zeros(4, dtype=np.uint64)
    t = threading.Thread(target=lib.bar_race, args=(r.h, 9, 20000, out.ctypes.data))  # (ctypes drops the GIL)
    t.start()
    t.join(120)
    assert not t.is_alive()
    hits, bad, pubs, none = (int(x) for x in out)
    print("hits %d, wrong reads %d, publishes %d, without a slot %d" % (hits, bad, pubs, none))
    assert bad == 0 and pubs > 0
    assert r.counts()[1:] == (0, 0)


def test_the_race_is_clean_under_the_thread_sanitizer(tmp_path):
    """bls_apk_ring_stub.cpp as a stand-alone program (its own main), built with -fsanitize=thread
    and run on the CPU; never loaded into Python.  Sanitizer runs stay off machines with a GPU
    (skipped where the compute device node exists); also skipped where the compiler cannot link the
    sanitizer's runtime or the runtime cannot map its shadow memory on this kernel."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer runs are for CPU-only machines")
    exe = str(tmp_path / "blsar_tsan")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=thread", "-DBLSAR_STUB_MAIN",
                        "-o", exe, STUB], capture_output=True, text=True, timeout=300)
    if b.returncode != 0:
        pytest.skip("cannot build with -fsanitize=thread here: " + b.stderr[-300:])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if "unexpected memory mapping" in p.stderr:
        pytest.skip("the thread sanitizer's runtime cannot start on this kernel")
    print(p.stdout.strip())
    assert p.returncode == 0 and "WARNING: ThreadSanitizer" not in p.stderr, p.stdout + p.stderr[-3000:]
    assert "0 wrong reads" in p.stdout and ", ok" in p.stdout
