"""The Ed25519 key cache's bookkeeping (narwhal_amd/csrc/keycache_alloc.h) on the host, with no HIP:
the key -> slot map, the slot and comb-table free lists, the pins of staged batches, the
registered-list fingerprint and the hold of in-flight calls, through the C interface of
tests/hostemu/keycache_alloc_stub.cpp.  tests/test_gpu_keycache_retain.py runs the same bookkeeping
inside the library, with the device records behind it."""
import ctypes
import os
import random
import subprocess
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "_build", "libkcalloc.so")
STUB = os.path.join(ROOT, "tests", "hostemu", "keycache_alloc_stub.cpp")
NONE = 0xFFFFFFFF
SLOTS, TABLES = 8, 4


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", ROOT, "tests/_build/libkcalloc.so"], check=True)
    L = ctypes.CDLL(SO)
    vp, u64, u32, i32, cp = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_char_p
    L.kca_new.argtypes, L.kca_new.restype = [u32, u32], vp
    L.kca_free.argtypes, L.kca_free.restype = [vp], None
    for name, args in (("kca_find", [vp, cp]), ("kca_assign", [vp, cp]), ("kca_take_and_give_back", [vp]),
                       ("kca_assign_table", [vp, cp]), ("kca_table_of", [vp, u32]), ("kca_pins", [vp, u32])):
        getattr(L, name).argtypes, getattr(L, name).restype = args, u32
    L.kca_pin.argtypes, L.kca_pin.restype = [vp, u32], None
    L.kca_unpin.argtypes, L.kca_unpin.restype = [vp, u32], None
    L.kca_retain.argtypes, L.kca_retain.restype = [vp, cp, u64, vp], None
    L.kca_set_registered.argtypes, L.kca_set_registered.restype = [vp, u64, cp, u64], None
    L.kca_reg_fp.argtypes, L.kca_reg_fp.restype = [vp], u64
    L.kca_counts.argtypes, L.kca_counts.restype = [vp, vp], None
    L.kca_hold_shared.argtypes, L.kca_hold_shared.restype = [vp], None
    L.kca_release_shared.argtypes, L.kca_release_shared.restype = [vp], None
    L.kca_race.argtypes, L.kca_race.restype = [vp, i32, i32, vp], None
    return L


def key(i):
    return (b"key-%06d" % i).ljust(32, b".")


class Cache:
    def __init__(self, lib, slots=SLOTS, tables=TABLES):
        self.lib = lib
        self.h = lib.kca_new(slots, tables)

    def close(self):
        self.lib.kca_free(self.h)

    def retain(self, keys):
        out = np.zeros(3, dtype=np.uint64)
        self.lib.kca_retain(self.h, b"".join(keys) if keys else None, len(keys), out.ctypes.data)
        return [int(x) for x in out]

    def counts(self):
        out = np.zeros(4, dtype=np.uint64)
        self.lib.kca_counts(self.h, out.ctypes.data)
        return dict(zip(("slots", "tables", "slot_hw", "table_hw"), (int(x) for x in out)))

    def __getattr__(self, name):
        f = getattr(self.lib, "kca_" + name)
        return lambda *a: f(self.h, *a)


@pytest.fixture
def cache(lib):
    made = []

    def make(*a):
        made.append(Cache(lib, *a))
        return made[-1]
    yield make
    for c in made:
        c.close()


def test_ten_thousand_random_operations_match_a_dict(cache):
    """assign / table assign / pin / unpin / retain against a model: key -> slot and slot -> table as
    Python dicts, pins as a dict, the two free lists as the sets of retired and not yet reused
    indices."""
    rng = random.Random(20261019)
    c = cache()
    slot, table, pins = {}, {}, {}          # key -> slot, slot -> table, slot -> pin count
    free_s, free_t = set(), set()           # retired, not reused yet
    hw_s, hw_t = 1, 0
    nkeys = 14
    ops = 0
    for step in range(10000):
        op = rng.choice(("assign", "assign", "table", "table", "pin", "unpin", "retain", "giveback"))
        k = rng.randrange(nkeys)
        if op == "assign":
            got = c.assign(key(k))
            if k in slot:
                assert got == slot[k]
            elif free_s:
                assert got in free_s, "a freed slot is reused before the high-water mark grows"
                free_s.discard(got)
                slot[k] = got
            elif hw_s < SLOTS:
                assert got == hw_s
                hw_s += 1
                slot[k] = got
            else:
                assert got == NONE
            assert got != 0, "slot 0 is never handed out"
        elif op == "giveback":
            got = c.take_and_give_back()
            if free_s:
                assert got in free_s
            elif hw_s < SLOTS:
                assert got == hw_s
                hw_s += 1
                free_s.add(got)
            else:
                assert got == NONE
        elif op == "table":
            got = c.assign_table(key(k))
            if k not in slot:
                assert got == NONE
            elif slot[k] in table:
                assert got == table[slot[k]]
            elif free_t:
                assert got in free_t, "a freed table is reused before the high-water mark grows"
                free_t.discard(got)
                table[slot[k]] = got
            elif hw_t < TABLES:
                assert got == hw_t
                hw_t += 1
                table[slot[k]] = got
            else:
                assert got == NONE
        elif op == "pin" and k in slot:
            c.pin(slot[k])
            pins[slot[k]] = pins.get(slot[k], 0) + 1
        elif op == "unpin" and k in slot and pins.get(slot[k], 0):
            c.unpin(slot[k])
            pins[slot[k]] -= 1
        elif op == "retain":
            keep = rng.sample(range(nkeys + 3), rng.randrange(0, 6))  # (some names are not cached)
            keep = keep + keep[:1]                                     # (a duplicate)
            out = c.retain([key(j) for j in keep])
            # (a slot whose pins are all gone is in `gone` at once: the first retain after the unpin)
            gone = [j for j in slot if j not in keep and not pins.get(slot[j], 0)]
            kept_pinned = [j for j in slot if j not in keep and pins.get(slot[j], 0)]
            assert out == [len(gone), sum(slot[j] in table for j in gone), len(kept_pinned)]
            for j in gone:
                s = slot.pop(j)
                assert s != 0, "slot 0 is never freed"
                free_s.add(s)
                if s in table:
                    free_t.add(table.pop(s))
            for j in kept_pinned:
                assert c.find(key(j)) == slot[j], "a pinned slot survives a retain"
                assert c.table_of(slot[j]) == table.get(slot[j], NONE), "with its table"
        else:
            continue
        ops += 1
        # the whole state against the model, every step
        live = {}
        for j in range(nkeys):
            s = c.find(key(j))
            assert s == slot.get(j, NONE)
            if s != NONE:
                assert s not in live, "two live keys share a slot"
                live[s] = j
                assert c.pins(s) == pins.get(s, 0)
        tabs = [c.table_of(s) for s in live]
        tabs = [t for t in tabs if t != NONE]
        assert len(tabs) == len(set(tabs)), "two live keys share a table"
        assert sorted(tabs) == sorted(table.values())
        assert all(c.table_of(s) == NONE for s in free_s), "a freed slot has no table"
        assert c.counts() == {"slots": 1 + len(slot), "tables": len(table), "slot_hw": hw_s, "table_hw": hw_t}
        assert hw_s - len(free_s) == 1 + len(slot) and hw_t - len(free_t) == len(table)
    assert ops > 8000 and hw_s == SLOTS and hw_t == TABLES


def test_a_pinned_slot_goes_at_the_first_retain_after_its_unpin(cache):
    c = cache()
    s = [c.assign(key(j)) for j in range(3)]
    t = [c.assign_table(key(j)) for j in range(3)]
    assert s == [1, 2, 3] and t == [0, 1, 2]
    c.pin(s[1])
    c.pin(s[1])  # two staged batches read it
    assert c.retain([]) == [2, 2, 1]
    assert c.find(key(1)) == 2 and c.table_of(2) == 1 and c.find(key(0)) == NONE
    c.unpin(s[1])
    assert c.retain([]) == [0, 0, 1]  # one batch still lives
    c.unpin(s[1])
    assert c.retain([key(1)]) == [0, 0, 0]  # named: kept, and not "only because it is pinned"
    assert c.retain([]) == [1, 1, 0]
    assert c.counts() == {"slots": 1, "tables": 0, "slot_hw": 4, "table_hw": 3}
    # the freed indices come back before a new one is touched
    again = sorted(c.assign(key(10 + j)) for j in range(3))
    assert again == [1, 2, 3] and c.counts()["slot_hw"] == 4
    assert sorted(c.assign_table(key(10 + j)) for j in range(3)) == [0, 1, 2] and c.counts()["table_hw"] == 3


def test_the_fingerprint_is_cleared_exactly_when_a_registered_key_is_retired(cache):
    c = cache()
    reg = [key(j) for j in range(3)]
    other = [key(j) for j in range(3, 6)]
    for k in reg + other:
        c.assign(k)
    c.set_registered(0xABCDEF, b"".join(reg), 3)
    assert c.reg_fp() == 0xABCDEF
    assert c.retain(reg + other) == [0, 0, 0] and c.reg_fp() == 0xABCDEF       # nothing retired
    assert c.retain(reg + other[:1]) == [2, 0, 0] and c.reg_fp() == 0xABCDEF   # only keys outside the list
    c.pin(c.find(reg[0]))
    assert c.retain(reg[1:]) == [1, 0, 1] and c.reg_fp() == 0xABCDEF           # a pinned member stays: still whole
    c.unpin(c.find(reg[0]))
    assert c.retain(reg[1:]) == [1, 0, 0] and c.reg_fp() == 0                  # a member went
    c.set_registered(0x1234, b"".join(reg[1:]), 2)
    assert c.retain([]) == [2, 0, 0] and c.reg_fp() == 0


def test_slot_zero_and_capacity(cache):
    c = cache(4, 2)
    assert [c.assign(key(j)) for j in range(5)] == [1, 2, 3, NONE, NONE]
    assert [c.assign_table(key(j)) for j in range(4)] == [0, 1, NONE, NONE]
    c.pin(0)
    c.unpin(0)
    assert c.pins(0) == 0
    assert c.retain([]) == [3, 2, 0] and c.counts()["slots"] == 1
    assert 0 not in [c.assign(key(10 + j)) for j in range(3)]


def test_a_retainer_finishes_under_four_overlapping_holders_and_is_alone_inside(lib, cache):
    c = cache()
    out = np.zeros(4, dtype=np.uint64)
    t = threading.Thread(target=lib.kca_race, args=(c.h, 4, 1000, out.ctypes.data))  # (ctypes drops the GIL)
    t.start()
    t.join(120)
    assert not t.is_alive(), "the retainer starved"
    retains, overlaps, holds, during = (int(x) for x in out)
    print("retains %d, holds %d (%d while retains were pending), overlaps %d" % (retains, holds, during, overlaps))
    assert retains == 1000 and overlaps == 0
    assert during >= 999  # every retain met holders that had got in since the one before


def test_the_hold_loop_is_clean_under_the_thread_sanitizer(tmp_path):
    """keycache_alloc_stub.cpp as a stand-alone program (its own main), built with -fsanitize=thread
    and run on the CPU; never loaded into Python.  Sanitizer runs stay off machines with a GPU
    (skipped where the compute device node exists); also skipped where the compiler cannot link the
    sanitizer's runtime or the runtime cannot map its shadow memory on this kernel."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer runs are for CPU-only machines")
    exe = str(tmp_path / "kcalloc_tsan")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=thread", "-DKCALLOC_STUB_MAIN",
                        "-o", exe, STUB], capture_output=True, text=True, timeout=300)
    if b.returncode != 0:
        pytest.skip("cannot build with -fsanitize=thread here: " + b.stderr[-300:])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if "unexpected memory mapping" in p.stderr:
        pytest.skip("the thread sanitizer's runtime cannot start on this kernel")
    print(p.stdout.strip())
    assert p.returncode == 0 and "WARNING: ThreadSanitizer" not in p.stderr, p.stdout + p.stderr[-3000:]
    assert "1000 retains" in p.stdout and ", ok" in p.stdout
