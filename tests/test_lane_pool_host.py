"""The lease rule of a device object's lane pools (narwhal_amd/csrc/lane_pool.h) on the host, with
no HIP, through the C interface of tests/hostemu/lane_pool_stub.cpp: ordinary and reserved lanes,
the two classes of call, waiters and wake-ups, the counters.  tests/test_gpu_qos.py runs the same
rule inside the library on the GPU."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "_build", "liblanepool.so")
STUB = os.path.join(ROOT, "tests", "hostemu", "lane_pool_stub.cpp")
WAIT_MS = 20000  # upper bound on a wake-up that must come; never waited out by a passing test


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", ROOT, "tests/_build/liblanepool.so"], check=True)
    L = ctypes.CDLL(SO)
    vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    L.lp_new.argtypes, L.lp_new.restype = [u64, u64], vp
    L.lp_free.argtypes, L.lp_free.restype = [vp], None
    L.lp_fail_next_open.argtypes, L.lp_fail_next_open.restype = [vp, i32], None
    L.lp_try_lease.argtypes = [vp, i32, ctypes.POINTER(i32)]
    L.lp_release.argtypes, L.lp_release.restype = [vp, i32], None
    L.lp_counters.argtypes, L.lp_counters.restype = [vp, vp], None
    L.lp_idle.argtypes, L.lp_idle.restype = [vp], u64
    L.lp_lanes.argtypes, L.lp_lanes.restype = [vp], u64
    L.lp_first_reserved.argtypes = [vp]
    L.lp_lease_async.argtypes, L.lp_lease_async.restype = [vp, i32], vp
    L.lp_waiter_wait.argtypes = [vp, i32, ctypes.POINTER(i32)]
    L.lp_waiter_free.argtypes, L.lp_waiter_free.restype = [vp], None
    L.lp_hammer.argtypes, L.lp_hammer.restype = [vp, i32, i32], u64
    L.lp_lane_leases.argtypes, L.lp_lane_leases.restype = [vp, i32], u64
    L.lp_env_lanes.restype = u64
    L.lp_env_digest_bytes.restype = u64
    L.lp_clamp.argtypes, L.lp_clamp.restype = [u64, u64], u64
    return L


WOULD_WAIT, OPEN_FAILED = -1, -2


class Pool:
    def __init__(self, lib, ordinary, reserved):
        self.lib = lib
        self.h = lib.lp_new(ordinary, reserved)

    def close(self):
        self.lib.lp_free(self.h)

    def lease(self, latency):
        """(lane id, reserved) of a lease that does not block; (WOULD_WAIT, False) where it would"""
        r = ctypes.c_int(0)
        lane = self.lib.lp_try_lease(self.h, 1 if latency else 0, ctypes.byref(r))
        return lane, bool(r.value)

    def release(self, lane):
        self.lib.lp_release(self.h, lane)

    def counters(self):
        out = np.zeros(8, dtype=np.uint64)
        self.lib.lp_counters(self.h, out.ctypes.data)
        return [int(x) for x in out]

    def idle(self):
        return int(self.lib.lp_idle(self.h))

    def blocking(self, latency):
        return self.lib.lp_lease_async(self.h, 1 if latency else 0)

    def waited_for(self, w, ms=WAIT_MS):
        """the lane a blocking lease got, or None if it still waits after ms"""
        lane = ctypes.c_int(-9)
        return lane.value if self.lib.lp_waiter_wait(w, ms, ctypes.byref(lane)) else None


@pytest.fixture
def pool(lib):
    made = []

    def make(ordinary, reserved):
        made.append(Pool(lib, ordinary, reserved))
        return made[-1]
    yield make
    for p in made:
        p.close()


class Model:
    """The rule restated: lanes are numbered in the order they are opened; idle lanes are stacks."""

    def __init__(self, ordinary, reserved):
        self.ocap, self.rcap = ordinary, reserved
        self.ord, self.res, self.idle_ord, self.idle_res = [], [], [], []
        self.next = 0
        self.c = [0] * 5

    def _open(self, pool_list):
        pool_list.append(self.next)
        self.next += 1
        return pool_list[-1]

    def lease(self, latency):
        lane, reserved = None, False
        if latency and self.idle_res:
            lane, reserved = self.idle_res.pop(), True
        elif latency and len(self.res) < self.rcap:
            lane, reserved = self._open(self.res), True
        elif self.idle_ord:
            lane = self.idle_ord.pop()
        elif len(self.ord) < self.ocap:
            lane = self._open(self.ord)
        if lane is None:
            return WOULD_WAIT, False
        if latency:
            self.c[0] += 1
            self.c[1] += 1 if reserved else 0
        else:
            self.c[3] += 1
        return lane, reserved

    def release(self, lane):
        (self.idle_res if lane in self.res else self.idle_ord).append(lane)

    def counters(self):
        return self.c + [len(self.res), self.rcap, len(self.ord)]


@pytest.mark.parametrize("ordinary,reserved,seed", [(1, 1, 1), (4, 2, 2), (8, 4, 3), (2, 1, 4), (3, 3, 5)])
def test_random_lease_and_release_sequences_follow_the_restated_rule(pool, ordinary, reserved, seed):
    rng = random.Random(seed)
    p, m = pool(ordinary, reserved), Model(ordinary, reserved)
    held, on_ordinary = [], 0
    for _ in range(3000):
        if held and (rng.random() < 0.45 or len(held) == ordinary + reserved):
            lane = held.pop(rng.randrange(len(held)))
            p.release(lane)
            m.release(lane)
        else:
            latency = rng.random() < 0.5
            got, want = p.lease(latency), m.lease(latency)
            assert got == want, (latency, got, want, held)
            if got[0] >= 0:
                held.append(got[0])
                on_ordinary += 1 if latency and not got[1] else 0
        assert p.counters() == m.counters()
        assert p.idle() == len(m.idle_ord) + len(m.idle_res)
    c = p.counters()
    assert c[1] + on_ordinary == c[0]  # every latency-class call ran on a reserved or an ordinary lane
    assert c[2] == 0 and c[4] == 0     # (no call of this test blocks)
    assert c[5] <= reserved and c[7] <= ordinary


def test_without_latency_calls_the_order_is_idle_lane_then_new_lane_then_wait(pool):
    p = pool(3, 2)
    assert [p.lease(False) for _ in range(3)] == [(0, False), (1, False), (2, False)]  # new lanes
    assert p.lease(False) == (WOULD_WAIT, False)
    p.release(1)
    p.release(0)
    p.release(2)
    assert [p.lease(False)[0] for _ in range(3)] == [2, 0, 1]  # the most recently returned first
    assert p.lease(False) == (WOULD_WAIT, False)
    p.release(0)
    assert p.lease(False) == (0, False)
    c = p.counters()
    assert c[:6] == [0, 0, 0, 7, 0, 0] and c[7] == 3  # no reserved lane was ever opened
    assert int(p.lib.lp_first_reserved(p.h)) == -1


def test_with_every_ordinary_lane_held_latency_is_served_and_bulk_waits(pool):
    p = pool(2, 2)
    assert [p.lease(False)[0] for _ in range(2)] == [0, 1]
    assert p.lease(True) == (2, True)   # a new reserved lane, no waiting
    p.release(2)
    assert p.idle() == 1                # a reserved lane is idle ...
    assert p.lease(False) == (WOULD_WAIT, False)  # ... and a bulk call still waits
    assert p.lease(True) == (2, True)   # the idle reserved lane
    assert p.lease(True) == (3, True)   # the second reserved lane
    assert p.lease(True) == (WOULD_WAIT, False)
    c = p.counters()
    assert c[0] == 3 and c[1] == 3 and c[2] == 0 and c[3] == 2 and c[5] == 2 and c[6] == 2 and c[7] == 2


def test_with_every_reserved_lane_held_latency_falls_through_to_the_ordinary_pool(pool):
    p = pool(2, 2)
    assert [p.lease(True) for _ in range(2)] == [(0, True), (1, True)]
    assert p.lease(True) == (2, False)  # a new ordinary lane
    p.release(2)
    assert p.lease(True) == (2, False)  # the idle ordinary lane
    assert p.lease(True) == (3, False)
    assert p.lease(True) == (WOULD_WAIT, False)
    p.release(1)
    assert p.lease(True) == (1, True)   # reserved lanes first again
    c = p.counters()
    assert c[0] == 6 and c[1] == 3 and c[5] == 2 and c[7] == 2


def test_a_reserved_cap_of_one(pool):
    p = pool(1, 1)
    assert p.lease(True) == (0, True)
    assert p.lease(True) == (1, False)
    assert p.lease(True) == (WOULD_WAIT, False) and p.lease(False) == (WOULD_WAIT, False)
    p.release(0)
    assert p.lease(False) == (WOULD_WAIT, False)
    assert p.lease(True) == (0, True)
    assert p.counters()[5:] == [1, 1, 1]


def test_a_failed_open_fails_the_lease_and_counts_nothing(lib, pool):
    p = pool(1, 1)
    lib.lp_fail_next_open(p.h, 1)
    assert p.lease(True) == (OPEN_FAILED, False)
    assert p.counters() == [0, 0, 0, 0, 0, 0, 1, 0]
    assert p.lease(True) == (0, True)


def test_a_waiting_bulk_call_is_not_served_by_a_reserved_lane(pool):
    p = pool(1, 1)
    assert p.lease(False) == (0, False)
    assert p.lease(True) == (1, True)
    w = p.blocking(False)
    p.release(1)                        # the reserved lane comes back: not for the bulk waiter
    assert p.lease(True) == (1, True)   # still there for a latency-class call
    p.release(0)                        # the ordinary lane comes back: the waiter's
    assert p.waited_for(w) == 0
    p.lib.lp_waiter_free(w)
    c = p.counters()
    assert c[3] == 2 and c[4] <= 1 and c[0] == 2 and c[1] == 2


@pytest.mark.parametrize("back", ["reserved", "ordinary"])
def test_a_waiting_latency_call_takes_the_first_lane_of_either_pool(pool, back):
    p = pool(1, 1)
    assert p.lease(True) == (0, True)
    assert p.lease(False) == (1, False)
    w = p.blocking(True)
    lane = 0 if back == "reserved" else 1
    p.release(lane)
    assert p.waited_for(w) == lane
    p.lib.lp_waiter_free(w)
    c = p.counters()
    assert c[0] == 2 and c[1] == (2 if back == "reserved" else 1) and c[2] <= 1


def test_an_ordinary_lane_wakes_a_waiter_of_each_class(pool):
    """One ordinary lane returns while a bulk and a latency call wait: one of them gets it, and the
    next return serves the other (no wake-up is lost to the waiter that found the lane gone)."""
    p = pool(1, 1)
    assert p.lease(True) == (0, True)
    assert p.lease(False) == (1, False)
    wb, wl = p.blocking(False), p.blocking(True)
    p.release(1)
    first = None
    for _ in range(WAIT_MS):  # a bounded poll of both: one of them gets the lane at once
        if p.waited_for(wl, 0) is not None:
            first = (wl, wb)
        elif p.waited_for(wb, 1) is not None:
            first = (wb, wl)
        if first:
            break
    assert first is not None and p.waited_for(first[0], 0) == 1
    assert p.waited_for(first[1], 0) is None  # one lane, one holder
    p.release(1)
    assert p.waited_for(first[1]) == 1
    p.lib.lp_waiter_free(wb)
    p.lib.lp_waiter_free(wl)
    p.release(1)
    p.release(0)
    assert p.idle() == 2


def test_eight_threads_of_holders_and_waiters_end_with_every_lane_idle(lib, pool):
    threads, iters = 8, 4000
    p = pool(2, 1)
    assert lib.lp_hammer(p.h, threads, iters) == threads * iters  # 0: two holders of one lane
    c = p.counters()
    assert c[0] == c[3] == threads * iters // 2
    assert c[1] <= c[0] and c[2] <= c[0] and c[4] <= c[3]
    assert c[5] == 1 and 1 <= c[7] <= 2
    lanes = int(lib.lp_lanes(p.h))
    assert p.idle() == lanes == c[5] + c[7]
    assert sum(int(lib.lp_lane_leases(p.h, k)) for k in range(lanes)) == threads * iters
    assert int(lib.lp_lane_leases(p.h, int(lib.lp_first_reserved(p.h)))) == c[1]


def test_the_setter_clamp_stays_below_the_shard_minimum(lib):
    assert lib.lp_clamp(0, 16384) == 0 and lib.lp_clamp(64, 16384) == 64
    assert lib.lp_clamp(16383, 16384) == 16383 and lib.lp_clamp(16384, 16384) == 16383
    assert lib.lp_clamp(1 << 40, 256) == 255 and lib.lp_clamp(5, 1) == 0


def test_the_environment_is_read_with_its_defaults_and_range():
    subprocess.run(["make", "-s", "-C", ROOT, "tests/_build/liblanepool.so"], check=True)
    code = ("import ctypes; L = ctypes.CDLL(%r); L.lp_env_lanes.restype = ctypes.c_uint64; "
            "L.lp_env_digest_bytes.restype = ctypes.c_uint64; "
            "print(L.lp_env_lanes(), L.lp_env_digest_bytes(), L.lp_env_priority())" % SO)
    names = ("NWV_LATENCY_LANES", "NWV_LATENCY_DIGEST_BYTES", "NWV_LATENCY_PRIORITY")
    for vals, want in (((None, None, None), "2 1048576 1"), (("1", "4096", "0"), "1 4096 0"),
                       (("4", "0", "1"), "4 0 1"), (("9", "", ""), "4 1048576 1"), (("0", None, "x"), "1 1048576 1"),
                       (("-3", None, None), "1 1048576 1")):
        env = {k: v for k, v in os.environ.items() if k not in names}
        env.update({k: v for k, v in zip(names, vals) if v is not None})
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=60)
        assert p.returncode == 0 and p.stdout.strip() == want, (vals, p.stdout, p.stderr)


def test_the_threaded_loop_is_clean_under_the_thread_sanitizer(tmp_path):
    """lane_pool_stub.cpp as a stand-alone program (its own main), built with -fsanitize=thread and
    run on the CPU; never loaded into Python.  Sanitizer runs stay off machines with a GPU (skipped
    where the compute device node exists); also skipped where the compiler cannot link the
    sanitizer's runtime or the runtime cannot map its shadow memory on this kernel."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer runs are for CPU-only machines")
    exe = str(tmp_path / "lane_pool_tsan")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=thread", "-DLANE_POOL_STUB_MAIN",
                        "-o", exe, STUB], capture_output=True, text=True, timeout=300)
    if b.returncode != 0:
        pytest.skip("cannot build with -fsanitize=thread here: " + b.stderr[-300:])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if "unexpected memory mapping" in p.stderr:
        pytest.skip("the thread sanitizer's runtime cannot start on this kernel")
    print(p.stdout.strip())
    assert p.returncode == 0 and "WARNING: ThreadSanitizer" not in p.stderr, p.stdout + p.stderr[-3000:]
    assert "32000 leases, ok" in p.stdout
