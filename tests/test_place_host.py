"""The placement policy of a multi-device context (narwhal_amd/csrc/place.h) on the host, with no
HIP: the load table, the tickets a call holds and the rotation of calls that split, through the C
interface of tests/hostemu/place_stub.cpp.  tests/test_gpu_place.py runs the same policy inside the
library, over device replicas on the GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "_build", "libplace.so")
STUB = os.path.join(ROOT, "tests", "hostemu", "place_stub.cpp")


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", ROOT, "tests/_build/libplace.so"], check=True)
    L = ctypes.CDLL(SO)
    vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    L.pl_new.argtypes, L.pl_new.restype = [u64, i32], vp
    L.pl_free.argtypes, L.pl_free.restype = [vp], None
    L.pl_pick.argtypes, L.pl_pick.restype = [vp, u64, i32], vp
    L.pl_acquire.argtypes, L.pl_acquire.restype = [vp, u64, u64, i32], vp
    L.pl_ticket_dev.argtypes = [vp]
    L.pl_release.argtypes, L.pl_release.restype = [vp], None
    L.pl_call_ranges.argtypes = [vp, i32, u64, i32, vp]
    L.pl_failing_call.argtypes = [vp, u64, i32, vp]
    L.pl_get.argtypes, L.pl_get.restype = [vp, u64, vp], None
    L.pl_hammer.argtypes, L.pl_hammer.restype = [vp, i32, i32, vp], u64
    return L


class Table:
    def __init__(self, lib, ndev, first=False):
        self.lib, self.ndev = lib, ndev
        self.h = lib.pl_new(ndev, 1 if first else 0)

    def close(self):
        self.lib.pl_free(self.h)

    def pick(self, items=1, engine=0):
        t = self.lib.pl_pick(self.h, items, engine)
        return t, self.lib.pl_ticket_dev(t)

    def hold(self, dev, items=1, engine=0):
        return self.lib.pl_acquire(self.h, dev, items, engine)

    def release(self, t):
        self.lib.pl_release(t)

    def call(self, k, per=64, engine=0):
        devs = np.full(max(k, 1), -1, dtype=np.int32)
        n = self.lib.pl_call_ranges(self.h, k, per, engine, devs.ctypes.data)
        return devs[:n].tolist()

    def get(self, dev):
        out = np.zeros(7, dtype=np.uint64)
        self.lib.pl_get(self.h, dev, out.ctypes.data)
        return dict(zip(("out_ranges", "out_items", "peak", "ranges0", "items0", "ranges1", "items1"),
                        (int(x) for x in out)))


@pytest.fixture
def table(lib):
    made = []

    def make(ndev, first=False):
        made.append(Table(lib, ndev, first))
        return made[-1]
    yield make
    for t in made:
        t.close()


def test_an_idle_table_picks_index_0_every_time(table):
    t = table(3)
    for _ in range(20):
        tk, d = t.pick(5)
        assert d == 0
        t.release(tk)
    assert t.get(0)["ranges0"] == 20 and t.get(0)["items0"] == 100 and t.get(0)["peak"] == 1
    assert all(t.get(d)["ranges0"] == 0 for d in (1, 2))


def test_the_fewest_outstanding_ranges_win(table):
    t = table(3)
    t.hold(0)  # loads (1, 0, 0)
    tk, d = t.pick()
    assert d == 1
    t.release(tk)
    t.hold(1)  # loads (1, 1, 0)
    tk, d = t.pick()
    assert d == 2
    t.release(tk)
    t.hold(2)  # loads (1, 1, 1): the lowest index again
    assert t.pick()[1] == 0


def test_equal_ranges_go_to_the_fewest_outstanding_items(table):
    t = table(3)
    t.hold(0, items=100)
    t.hold(1, items=7)
    t.hold(2, items=50)
    assert t.pick(1000)[1] == 1  # (100, 7, 50) items -> device 1, now 2 ranges there
    assert t.pick(1)[1] == 2     # ranges (1, 2, 1): items 100 against 50
    assert t.pick(1)[1] == 0     # ranges (1, 2, 2)


def test_a_released_ticket_restores_the_entry(table):
    t = table(2)
    tk, d = t.pick(9)
    assert d == 0 and t.get(0)["out_ranges"] == 1 and t.get(0)["out_items"] == 9
    t.release(tk)
    e = t.get(0)
    assert e["out_ranges"] == 0 and e["out_items"] == 0 and e["ranges0"] == 1 and e["items0"] == 9 and e["peak"] == 1
    assert t.pick()[1] == 0


@pytest.mark.parametrize("fail", [0, 7])
def test_a_call_releases_its_ticket_on_the_error_path_too(lib, table, fail):
    t = table(3)
    t.hold(0)
    dev = ctypes.c_int(-1)
    assert lib.pl_failing_call(t.h, 11, fail, ctypes.byref(dev)) == fail
    assert dev.value == 1
    e = t.get(1)
    assert e["out_ranges"] == 0 and e["out_items"] == 0 and e["ranges0"] == 1 and e["items0"] == 11
    assert t.pick()[1] == 1  # device 0 is still held, device 1 is free again


@pytest.mark.parametrize("ndev", range(1, 9))
def test_ndev_consecutive_split_calls_put_k_ranges_on_every_device(table, ndev):
    for k in range(2, ndev + 1):
        t = table(ndev)
        seen = []
        for _ in range(ndev):
            devs = t.call(k)
            assert len(devs) == k and len(set(devs)) == k  # a call's ranges on k different devices
            assert all(devs[j + 1] == (devs[j] + 1) % ndev for j in range(k - 1))
            seen.append(devs[0])
        assert sorted(seen) == list(range(ndev))  # the base rotates
        for d in range(ndev):
            e = t.get(d)
            assert e["ranges0"] == k and e["items0"] == 64 * k and e["out_ranges"] == 0 and e["peak"] == 1


def test_a_split_call_does_not_move_the_single_range_rule(table):
    t = table(4)
    assert t.call(2) == [0, 1] and t.call(3) == [1, 2, 3]
    assert t.call(1) == [0]  # the tickets of the split calls are back: idle table, index 0
    t.hold(0)
    assert t.call(1) == [1] and t.call(2) == [2, 3]


def test_first_mode_reproduces_device_0_and_device_k(table):
    t = table(4, first=True)
    t.hold(0, items=1000)
    t.hold(0, items=1000)
    for _ in range(3):
        tk, d = t.pick()
        assert d == 0  # whatever the load
        t.release(tk)
    for _ in range(3):
        assert t.call(3) == [0, 1, 2] and t.call(4) == [0, 1, 2, 3]
    assert t.get(0)["ranges0"] == 2 + 3 + 6 and t.get(3)["ranges0"] == 3  # the counters are kept


def test_nwv_place_is_read_from_the_environment():
    code = ("import ctypes; L = ctypes.CDLL(%r); print(L.pl_env_first())" % SO)
    for val, want in (("first", "1"), ("load", "0"), ("", "0"), (None, "0")):
        env = {k: v for k, v in os.environ.items() if k != "NWV_PLACE"}
        if val is not None:
            env["NWV_PLACE"] = val
        subprocess.run(["make", "-s", "-C", ROOT, "tests/_build/libplace.so"], check=True)
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=60)
        assert p.returncode == 0 and p.stdout.strip() == want, (val, p.stdout, p.stderr)


def test_the_engines_share_the_load_and_keep_their_own_totals(table):
    t = table(2)
    t.hold(0, items=4, engine=1)  # a BLS call in flight on device 0
    tk, d = t.pick(3, engine=0)   # pushes an Ed25519 call to device 1
    assert d == 1
    assert t.get(0)["ranges1"] == 1 and t.get(0)["ranges0"] == 0 and t.get(0)["items1"] == 4
    assert t.get(1)["ranges0"] == 1 and t.get(1)["ranges1"] == 0 and t.get(1)["items0"] == 3


def test_eight_threads_of_pick_and_release_pairs_leave_a_consistent_table(lib, table):
    threads, iters = 8, 10000
    t = table(3)
    per = np.zeros(3, dtype=np.uint64)
    picks = lib.pl_hammer(t.h, threads, iters, per.ctypes.data)
    assert picks == threads * iters
    es = [t.get(d) for d in range(3)]
    assert sum(e["ranges0"] for e in es) == picks
    assert [e["ranges0"] for e in es] == per.tolist()
    assert all(e["out_ranges"] == 0 and e["out_items"] == 0 for e in es)
    assert all(e["peak"] <= threads for e in es) and es[0]["peak"] >= 1


def test_the_threaded_loop_is_clean_under_the_thread_sanitizer(tmp_path):
    """place_stub.cpp as a stand-alone program (its own main), built with -fsanitize=thread and run
    on the CPU; never loaded into Python.  Sanitizer runs stay off machines with a GPU (skipped where
    the compute device node exists); also skipped where the compiler cannot link the sanitizer's
    runtime or the runtime cannot map its shadow memory on this kernel."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer runs are for CPU-only machines")
    exe = str(tmp_path / "place_tsan")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=thread", "-DPLACE_STUB_MAIN",
                        "-o", exe, STUB], capture_output=True, text=True, timeout=300)
    if b.returncode != 0:
        pytest.skip("cannot build with -fsanitize=thread here: " + b.stderr[-300:])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if "unexpected memory mapping" in p.stderr:
        pytest.skip("the thread sanitizer's runtime cannot start on this kernel")
    print(p.stdout.strip())
    assert p.returncode == 0 and "WARNING: ThreadSanitizer" not in p.stderr, p.stdout + p.stderr[-3000:]
    assert "80000 picks, ok" in p.stdout
