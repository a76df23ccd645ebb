"""The host pass of the key-transposed batch check (narwhal_amd/csrc/bls_key_batch.h through
tests/hostemu/bls_key_batch_stub.cpp, no GPU): which items enter the groups, the groups' key
entries and key-major lists with one entry per occurrence, the quarter rule, the half rule, and the
per-item launch ranges -- against a plain Python transposition of random inputs."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8, u32, u64 = np.uint8, np.uint32, np.uint64


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "tests", "_build", "libblskeybatch.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-C", ROOT, "tests/_build/libblskeybatch.so"], check=True)
    L = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    L.bkb_plan.argtypes = [ctypes.c_uint64, vp, vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    L.bkb_plan.restype = vp
    L.bkb_free.argtypes = [vp]
    L.bkb_sizes.argtypes = [vp, vp]
    L.bkb_get.argtypes = [vp, ctypes.c_int, vp]
    L.bkb_ranges.argtypes = [ctypes.c_uint64, vp, ctypes.c_uint64, vp]
    L.bkb_ranges.restype = ctypes.c_uint64
    return L


NAMES = ("items", "gfirst", "goff", "eslot", "egrp", "coff", "cidx", "outside")


def plan(lib, ok, elig, lists, slot_cap, group, ratio):
    n = len(lists)
    off = np.array([sum(len(x) for x in lists[:i]) for i in range(n)], dtype=u32)
    cnt = np.array([len(x) for x in lists], dtype=u32)
    idx = np.array([s for x in lists for s in x] + [0], dtype=u32)
    a_ok, a_el = np.array(ok + [0], dtype=u8), np.array(elig + [0], dtype=u8)
    h = lib.bkb_plan(n, a_ok.ctypes.data, a_el.ctypes.data, off.ctypes.data, cnt.ctypes.data, idx.ctypes.data,
                     slot_cap, group, ratio)
    sizes = np.zeros(14, dtype=u64)
    lib.bkb_sizes(h, sizes.ctypes.data)
    out = dict(zip(("run", "n_ok", "n_eligible", "groups", "entries", "millers"), (int(x) for x in sizes[:6])))
    for k, name in enumerate(NAMES):
        a = np.zeros(int(sizes[6 + k]) + 1, dtype=u32)
        lib.bkb_get(h, k, a.ctypes.data)
        out[name] = [int(x) for x in a[:-1]]
    lib.bkb_free(h)
    return out


def model(ok, elig, lists, group, ratio):
    """the same plan in plain Python: dicts keep a group's keys in first-occurrence order"""
    n = len(lists)
    n_ok = sum(ok)
    el = [i for i in range(n) if ok[i] and elig[i] and lists[i]]
    off = {"run": 0, "n_ok": n_ok, "n_eligible": len(el), "groups": 0, "entries": 0, "millers": 0, "items": [],
           "gfirst": [], "goff": [], "eslot": [], "egrp": [], "coff": [], "cidx": [],
           "outside": [i for i in range(n) if ok[i]]}
    if not el or 2 * len(el) < n_ok:
        return off
    items, gfirst, goff, eslot, egrp, coff, cidx = [], [0], [0], [], [], [0], []
    for lo in range(0, len(el), group):
        grp = el[lo:lo + group]
        occ = {}
        for p, i in enumerate(grp):
            for s in lists[i]:
                occ.setdefault(s, []).append(len(items) + p)
        if ratio and (len(occ) + 1) * ratio > len(grp):
            continue
        for s, where in occ.items():
            eslot.append(s)
            egrp.append(len(gfirst) - 1)
            cidx += where
            coff.append(len(cidx))
        items += grp
        gfirst.append(len(items))
        goff.append(len(eslot))
    if len(gfirst) == 1:
        return off
    kept = set(items)
    return {"run": 1, "n_ok": n_ok, "n_eligible": len(el), "groups": len(gfirst) - 1, "entries": len(eslot),
            "millers": len(eslot) + len(gfirst) - 1, "items": items, "gfirst": gfirst, "goff": goff, "eslot": eslot,
            "egrp": egrp, "coff": coff, "cidx": cidx, "outside": [i for i in range(n) if ok[i] and i not in kept]}


def random_call(rnd, n, slots, p_ok=0.95, p_el=0.9):
    ok = [int(rnd.random() < p_ok) for _ in range(n)]
    elig = [int(rnd.random() < p_el) for _ in range(n)]
    lists = []
    for _ in range(n):
        kind = rnd.random()
        if kind < 0.05:
            lists.append([])  # (an empty list never has OK statuses in the engine; the plan skips it all the same)
        elif kind < 0.6:
            lists.append([rnd.randrange(slots)])
        else:
            lists.append([rnd.randrange(slots) for _ in range(rnd.randrange(2, 9))])  # duplicates included
    return ok, elig, lists


@pytest.mark.parametrize("seed", range(8))
def test_plan_matches_python_transposition(lib, seed):
    rnd = random.Random(1000 + seed)
    n, slots = rnd.choice([1, 7, 64, 257, 900]), rnd.choice([1, 3, 17, 100])
    group, ratio = rnd.choice([1, 6, 50, 2048]), rnd.choice([0, 0, 2, 4])
    ok, elig, lists = random_call(rnd, n, slots)
    assert plan(lib, ok, elig, lists, slots, group, ratio) == model(ok, elig, lists, group, ratio)


def test_duplicates_and_group_boundaries(lib):
    """one entry per occurrence: an item that lists slot 2 twice appears twice in slot 2's list;
    groups of three eligible items, the non-eligible item 2 between them belongs to none"""
    lists = [[2, 2], [0], [5], [2, 0], [1], [0], [2]]
    ok = [1] * 7
    elig = [1, 1, 0, 1, 1, 1, 1]
    p = plan(lib, ok, elig, lists, 8, 3, 0)
    assert p["run"] == 1 and p["items"] == [0, 1, 3, 4, 5, 6] and p["gfirst"] == [0, 3, 6]
    assert p["outside"] == [2]
    assert p["goff"] == [0, 2, 5] and p["eslot"] == [2, 0, 1, 0, 2] and p["egrp"] == [0, 0, 1, 1, 1]
    assert p["coff"] == [0, 3, 5, 6, 7, 8]
    assert p["cidx"] == [0, 0, 2, 1, 2, 3, 4, 5]
    assert p["millers"] == 7 and p == model(ok, elig, lists, 3, 0)


def test_quarter_rule_drops_a_group_and_keeps_the_others(lib):
    """ratio 4: 12 items over 2 keys stay (3 * 4 <= 12), 12 items over 3 keys go (4 * 4 > 12), and
    the short last group of 4 items over one key goes too (2 * 4 > 4)"""
    lists = [[i % 2] for i in range(12)] + [[i % 3] for i in range(12)] + [[0]] * 4
    ok = elig = [1] * 28
    p = plan(lib, ok, elig, lists, 4, 12, 4)
    assert p["run"] == 1 and p["groups"] == 1 and p["items"] == list(range(12))
    assert p["outside"] == list(range(12, 28))
    assert p == model(ok, elig, lists, 12, 4)
    # every group dropped: the plan does not run and every OK item is outside
    q = plan(lib, ok, elig, lists[12:24], 4, 12, 4)
    assert q["run"] == 0 and q["groups"] == 0 and q["outside"] == list(range(12)) and q["items"] == []


def test_half_rule(lib):
    """fewer than half of the OK items eligible: the plan does not run; exactly half: it does"""
    lists = [[0]] * 10
    ok = [1] * 8 + [0, 0]
    p = plan(lib, ok, [1, 1, 1] + [0] * 7, lists, 1, 4, 0)
    assert p["run"] == 0 and p["n_ok"] == 8 and p["n_eligible"] == 3 and p["outside"] == list(range(8))
    p = plan(lib, ok, [1, 1, 1, 1] + [0] * 4 + [1, 1], lists, 1, 4, 0)  # (items 8, 9 are not OK)
    assert p["run"] == 1 and p["n_eligible"] == 4 and p["items"] == [0, 1, 2, 3] and p["outside"] == [4, 5, 6, 7]


def ranges(lib, need, gap):
    n = len(need)
    a = np.array(need + [0], dtype=u8)
    out = np.zeros(2 * n + 2, dtype=u64)
    k = int(lib.bkb_ranges(n, a.ctypes.data, gap, out.ctypes.data))
    return [(int(out[2 * j]), int(out[2 * j + 1])) for j in range(k)]


def group_loop_ranges(n, grp, gok, gap):
    """the wave batch check's re-check loop over its groups' verdicts, as the engine ran it before
    recheck_ranges served both checks: (lo, hi) per launch, and the rejected groups counted"""
    ng = (n + grp - 1) // grp
    out, rejected, g = [], 0, 0
    while g < ng:
        if gok[g] == 1:
            g += 1
            continue
        e = g + 1  # the range's end: past its last rejected group
        rejected += 1
        q = e
        while q < ng and (q - e) * grp < gap:
            if gok[q] != 1:
                e = q + 1
                rejected += 1
            q += 1
        out.append((g * grp, min(n, e * grp)))
        g = e
    return out, rejected


def test_ranges_share_launches_below_the_gap(lib):
    rnd, grnd = random.Random(5), random.Random(6)
    # group-shaped flags (every item of a rejected group marked, the last group partial): the ranges
    # of the wave batch check's former loop over the groups
    for grp in (1, 5, 7):
        for gap in (1, grp, 3 * grp, 1024):
            for n in (grp * 9 + 1 if grp > 1 else 10, grp * 40 + grp // 2 + 1, 2311):
                if grp > 1 and n % grp == 0:
                    n += 1
                ng = (n + grp - 1) // grp
                for p in (0.0, 0.1, 0.5, 1.0):
                    gok = [0 if grnd.random() < p else 1 for _ in range(ng)]
                    need = [int(gok[i // grp] != 1) for i in range(n)]
                    want, rejected = group_loop_ranges(n, grp, gok, gap)
                    assert ranges(lib, need, gap) == want, (grp, gap, n, gok)
                    assert rejected == sum(1 for v in gok if v != 1)
                    assert all(hi <= n for _, hi in want)
    for n, gap in [(1, 4), (40, 1), (200, 16), (5000, 1024)]:
        need = [int(rnd.random() < 0.03) for _ in range(n)]
        got = ranges(lib, need, gap)
        want = []
        for i in range(n):
            if need[i]:
                if want and i - want[-1][1] < gap:
                    want[-1] = (want[-1][0], i + 1)
                else:
                    want.append((i, i + 1))
        assert got == want
        assert all(need[lo] and need[hi - 1] for lo, hi in got)
        assert sum(need) == sum(sum(need[lo:hi]) for lo, hi in got)
