"""msm_plan's entries per bucket lane (narwhal_amd/csrc/msm.h msm_bucket_seg, called through
tests/hostemu/tail_rc_hostemu.cpp): two waves per SIMD of bucket lanes with a floor of 8, two
entries for tiny batches -- and, new, ONE wave per SIMD for large batches of the lane kernel: more
than 4,096 signatures, on the chunked sort, and more than 9 x 131,072 entries (where the two-wave
rule had left its floor).  Checked at each boundary of that range, and on the plans of real sizes
(tests/zcoeff_gpu_check.plan restates msm_plan's window choice; its own seg is the rule before this
one, which every batch outside the range keeps)."""
import ctypes
import os

import pytest

import zcoeff_gpu_check as zg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "_build", "libtailrcemu.so")
TWO_WAVES = 256 * 4 * 2 * 64  # bucket lanes at two waves per SIMD
FIRST = 9 * TWO_WAVES         # the first entry count of the new range
RULE_SEG_HEADLINE = 30        # 65,536 signatures, distinct keys: 1,966,100 entries


@pytest.fixture(scope="module")
def seg():
    if not os.path.exists(LIB_PATH):
        import subprocess
        subprocess.run(["make", "-C", ROOT, "tests/_build/libtailrcemu.so"], check=True)
    so = ctypes.CDLL(LIB_PATH)
    so.he_msm_bucket_seg.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
    so.he_msm_bucket_seg.restype = ctypes.c_uint32
    return so.he_msm_bucket_seg


def before(entries):
    s = min(64, max(8, entries // TWO_WAVES))
    return 2 if entries <= 2048 else s


def test_boundaries_of_the_large_batch_range(seg):
    big = 65536
    # entries: the last count of the old rule's floor, the first of the range
    assert seg(big, FIRST - 1, 17) == before(FIRST - 1) == 8
    assert seg(big, FIRST, 17) == 18 and before(FIRST) == 9
    # signatures: 4,096 and below keep their plan (the quad bucket kernel's batches)
    assert seg(4096, FIRST, 2) == 9 and seg(4097, FIRST, 2) == 18
    # the one-chunk sort path keeps its plan
    assert seg(big, FIRST, 1) == 9 and seg(big, FIRST, 2) == 18
    # the cap: 64 entries a lane, reached at 64 x 65,536 entries
    assert seg(1 << 21, 64 * 65536 - 1, 64) == 63
    assert seg(1 << 21, 64 * 65536, 64) == 64 and seg(1 << 24, 1 << 30, 64) == 64
    # one wave per SIMD in between: entries / 65,536, rounded down
    for e in (FIRST, 1966100, 30 * 65536 - 1, 30 * 65536, 31 * 65536 - 1, 3000000):
        assert seg(big, e, 17) == min(64, e // 65536), e


def test_every_batch_outside_the_range_keeps_its_plan(seg):
    for e in (0, 1, 47, 2048, 2049, 2117, 100000, TWO_WAVES * 8, FIRST - 1):
        for n, chunks in ((4, 1), (4096, 1), (4097, 2), (16385, 5)):
            assert seg(n, e, chunks) == before(e), (n, e, chunks)
    for e in (FIRST, 1966100, 1 << 23, 1 << 30):  # large entry counts on the kept paths
        assert seg(4096, e, 2) == before(e) and seg(1 << 20, e, 1) == before(e)


@pytest.mark.parametrize("n", [2, 29, 30, 1024, 4096, 4097, 4160, 8229, 16384, 16385, 32768])
def test_real_plans_below_the_range_are_unchanged(seg, n):
    p = zg.plan(n, n, env={})
    assert p["entries"] < FIRST
    assert seg(n, p["entries"], p["chunks"]) == p["seg"]


def test_headline_plan(seg):
    p = zg.plan(65536, 65536, env={})
    assert p["entries"] == 1966100 and p["chunks"] == 17 and p["seg"] == 15  # (the rule before)
    assert seg(65536, p["entries"], p["chunks"]) == RULE_SEG_HEADLINE
    # bucket lanes: 65,537 at 30 entries against 131,074 at 15 -- 257 workgroups of 256
    assert -(-p["entries"] // RULE_SEG_HEADLINE) == 65537


def test_first_real_size_inside_the_range(seg):
    """distinct keys: the plan's entries pass 9 x 131,072 between these two sizes"""
    lo, hi = 32768, 65536
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if zg.plan(mid, mid, env={})["entries"] >= FIRST:
            hi = mid
        else:
            lo = mid
    below, above = zg.plan(lo, lo, env={}), zg.plan(hi, hi, env={})
    assert seg(lo, below["entries"], below["chunks"]) == 8
    assert seg(hi, above["entries"], above["chunks"]) == above["entries"] // 65536 >= 18
