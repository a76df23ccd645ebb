"""The path an Ed25519 batch takes on its device (narwhal_amd/csrc/ed_plan.h) on the host, with no
HIP, through the C interface of tests/hostemu/ed_plan_stub.cpp.  The expected plans are a literal
table, not a second implementation.  tests/test_gpu_ed_paths.py runs one lane through
every path in turn inside the library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "_build", "libedplan.so")

NO_TINY, MSM_ALWAYS, MSM_NEVER = 4096, 1, 2  # include/nwv.h
TINY, COMB, MSM, EACH = "Tiny", "Comb", "Msm", "Each"
PASS = "Msm+pass"
LIM = (64, 128, 256, 1)  # tiny_max, comb_max, pass_max, msm_min


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", ROOT, "tests/_build/libedplan.so"], check=True)
    L = ctypes.CDLL(SO)
    u64, u32, i32, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p
    L.ep_plan.argtypes, L.ep_plan.restype = [u64, u32, i32, i32, i32, vp], i32
    L.ep_wants_tables.argtypes, L.ep_wants_tables.restype = [u64, u32, i32, i32, vp], i32
    L.ep_default_plan.restype = i32
    L.ep_forces_path_mask.restype = u32
    L.ep_flag.argtypes, L.ep_flag.restype = [i32], u32
    return L


def _name(code):
    path = (TINY, COMB, MSM, EACH)[code & 255]
    if code >> 8:
        assert path in (MSM, EACH)  # the pass goes with the flags' own path, never with Tiny or Comb
        return path + "+pass"
    return path


def plan(lib, n, flags=0, cached=True, tables=True, staged=False, lim=LIM):
    a = np.array(lim, dtype=np.uint64)
    return _name(lib.ep_plan(n, flags, int(cached), int(tables), int(staged), a.ctypes.data))


# (setup, keyword arguments of plan(), {n: expected})
TABLE = [
    ("keyed, cached, all tables", {}, {1: TINY, 64: TINY, 65: COMB, 128: COMB, 129: PASS, 256: PASS, 257: MSM}),
    ("keyed, one key lacks a table", {"tables": False}, {64: MSM, 65: MSM, 129: MSM}),
    ("keyed, not cached", {"cached": False, "tables": False}, {1: MSM, 64: MSM, 65: MSM, 129: MSM}),
    ("un-keyed", {"cached": False, "tables": False}, {1: MSM, 64: MSM, 65: MSM}),
    ("staged", {"staged": True}, {64: MSM, 129: MSM}),
    ("NO_TINY", {"flags": NO_TINY}, {64: MSM, 65: MSM, 129: MSM}),
    ("MSM_ALWAYS", {"flags": MSM_ALWAYS}, {64: TINY, 65: MSM, 129: MSM}),  # 64: the documented quirk
    ("MSM_NEVER", {"flags": MSM_NEVER}, {64: EACH, 65: EACH}),
    ("MSM_NEVER, un-keyed", {"flags": MSM_NEVER, "cached": False, "tables": False}, {5: EACH}),
    ("msm_min 100, un-keyed", {"cached": False, "tables": False, "lim": (64, 128, 256, 100)}, {99: EACH, 100: MSM}),
    ("msm_min 100 + MSM_ALWAYS, un-keyed",
     {"flags": MSM_ALWAYS, "cached": False, "tables": False, "lim": (64, 128, 256, 100)}, {5: MSM}),
    ("comb_max 0, pass_max 0", {"lim": (64, 0, 0, 1)}, {65: MSM}),
    ("comb_max 128, pass_max 100", {"lim": (64, 128, 100, 1)}, {100: COMB, 129: MSM}),
    ("comb_max 0 (a call that splits), pass_max 256", {"lim": (64, 0, 256, 1)}, {65: PASS}),
]


@pytest.mark.parametrize("setup,kw,want", TABLE, ids=[t[0] for t in TABLE])
def test_plan_table(lib, setup, kw, want):
    got = {n: plan(lib, n, **kw) for n in want}
    assert got == want, setup


def test_shared_mask_is_the_three_flags(lib):
    assert [lib.ep_flag(k) for k in range(3)] == [NO_TINY, MSM_ALWAYS, MSM_NEVER]
    assert lib.ep_forces_path_mask() == NO_TINY | MSM_ALWAYS | MSM_NEVER == 4099


def test_default_plan_before_any_staging(lib):
    assert _name(lib.ep_default_plan()) == MSM
    # a staged batch gets what an un-keyed one gets, whatever its keys
    for n in (1, 64, 65, 129):
        assert plan(lib, n, staged=True) == plan(lib, n, cached=False, tables=False)


def test_tables_are_looked_up_only_where_a_rule_could_hold(lib):
    def wants(n, flags=0, cached=True, staged=False, lim=LIM):
        a = np.array(lim, dtype=np.uint64)
        return bool(lib.ep_wants_tables(n, flags, int(cached), int(staged), a.ctypes.data))

    assert [wants(n) for n in (0, 1, 64, 65, 128, 129, 256, 257)] == [False] + [True] * 6 + [False]
    assert not wants(64, cached=False) and not wants(65, cached=False)
    assert not wants(64, staged=True) and not wants(129, staged=True)
    assert wants(64, MSM_ALWAYS) and not wants(65, MSM_ALWAYS) and not wants(129, MSM_ALWAYS)
    assert not any(wants(n, f) for n in (64, 65, 129) for f in (NO_TINY, MSM_NEVER))
    assert not wants(65, lim=(64, 0, 0, 1)) and wants(65, lim=(64, 0, 256, 1))
    # a plan never names a table path that the lookup was not made for
    for n in (0, 64, 65, 129, 257):
        for f in (0, NO_TINY, MSM_ALWAYS, MSM_NEVER):
            if not wants(n, f):
                assert plan(lib, n, f) in (MSM, EACH)
