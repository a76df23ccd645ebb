"""The digest stream's host side (narwhal_amd/csrc/digest_stream.h: chunk pool, hold-back rule, tick
plan, bincode walk, pump thread, backpressure, callbacks) with no GPU, through the C interface of
tests/hostemu/digest_stream_stub.cpp.  The stub device copies what a tick uploads into a pool of
its own and runs the tick's work records there with blake2b.h's compression, as k_blake2b_slice
does, so planner, padding, last_len and state carry are checked end to end against
hashlib.blake2b(digest_size=32).  tests/test_gpu_digest_stream.py runs the same stream on the GPU."""
import ctypes
import hashlib
import json
import os
import random
import subprocess
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "_build", "libdstream.so")
STUB = os.path.join(ROOT, "tests", "hostemu", "digest_stream_stub.cpp")
ERR_ARG, ERR_REENTRANT = -1, -7
STATS = ("messages", "ticks", "compressions", "uploaded", "tick_messages", "chunks", "chunks_peak", "waited")
DEVICE = ("violations", "copies", "copy_bytes", "busy_on", "busy_off", "rec_blocks", "tick_recs", "dup_slots")


def b2(m):
    return hashlib.blake2b(m, digest_size=32).digest()


def nblocks(n):
    return max(1, -(-n // 128))


def edge_lengths(s):
    return [0, 1, 127, 128, 129, 255, 256, 257, s * 128 - 1, s * 128, s * 128 + 1, 2 * s * 128, 3 * s * 128 + 5]


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", ROOT, "tests/_build/libdstream.so"], check=True)
    L = ctypes.CDLL(SO)
    vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    L.dsx_new.argtypes, L.dsx_new.restype = [u64, u64, u64, u64], vp
    L.dsx_free.argtypes, L.dsx_free.restype = [vp], None
    L.dsx_set_mode.argtypes, L.dsx_set_mode.restype = [vp, u64, i32], None
    L.dsx_submit.argtypes = [vp, ctypes.c_char_p, u64, u64]
    L.dsx_submit_serialized.argtypes = [vp, ctypes.c_char_p, u64, u64, ctypes.POINTER(ctypes.c_int64)]
    L.dsx_begin.argtypes = [vp, u64, ctypes.POINTER(u64)]
    L.dsx_update.argtypes = [vp, u64, ctypes.c_char_p, u64]
    L.dsx_finish.argtypes = [vp, u64]
    L.dsx_flush.argtypes = [vp]
    L.dsx_close.argtypes = [vp]
    L.dsx_stats.argtypes, L.dsx_stats.restype = [vp, vp], None
    L.dsx_result.argtypes = [vp, u64, ctypes.POINTER(ctypes.c_int32), vp]
    L.dsx_device.argtypes, L.dsx_device.restype = [vp, vp], None
    L.dsx_set_chained.argtypes = [vp, ctypes.c_char_p, u64]
    L.dsx_chain_rc.argtypes = [vp]
    L.dsx_reentrant.argtypes, L.dsx_reentrant.restype = [vp, vp], None
    L.dsx_walk.argtypes, L.dsx_walk.restype = [ctypes.c_char_p, u64, ctypes.POINTER(u64)], ctypes.c_int64
    return L


class Stream:
    def __init__(self, lib, slice_blocks, chunks, messages, tags):
        self.lib = lib
        self.h = lib.dsx_new(slice_blocks, chunks, messages, tags)
        assert self.h

    def free(self):
        if self.h:
            self.lib.dsx_free(self.h)
            self.h = None

    def submit(self, data, tag):
        return self.lib.dsx_submit(self.h, data, len(data), tag)

    def submit_serialized(self, buf, tag):
        err = ctypes.c_int64(-99)
        rc = self.lib.dsx_submit_serialized(self.h, buf, len(buf), tag, ctypes.byref(err))
        return rc, err.value

    def begin(self, tag):
        i = ctypes.c_uint64(0)
        assert self.lib.dsx_begin(self.h, tag, ctypes.byref(i)) == 0
        return i.value

    def update(self, mid, data):
        return self.lib.dsx_update(self.h, mid, data, len(data))

    def finish(self, mid):
        return self.lib.dsx_finish(self.h, mid)

    def flush(self):
        return self.lib.dsx_flush(self.h)

    def close(self):
        return self.lib.dsx_close(self.h)

    def result(self, tag):
        """(times the callback fired, its result, the digest)"""
        res = ctypes.c_int32(0)
        d = np.zeros(32, dtype=np.uint8)
        n = self.lib.dsx_result(self.h, tag, ctypes.byref(res), d.ctypes.data)
        return n, res.value, d.tobytes()

    def _u64s(self, fn, names):
        out = np.zeros(8, dtype=np.uint64)
        fn(self.h, out.ctypes.data)
        return dict(zip(names, (int(x) for x in out)))

    def stats(self):
        return self._u64s(self.lib.dsx_stats, STATS)

    def device(self):
        return self._u64s(self.lib.dsx_device, DEVICE)


@pytest.fixture
def stream(lib):
    made = []

    def make(slice_blocks, chunks, messages, tags):
        made.append(Stream(lib, slice_blocks, chunks, messages, tags))
        return made[-1]
    yield make
    for s in made:
        s.free()


def check_clean(s, total_len_blocks, n_messages):
    """after a flush: every block uploaded once and consumed once, nothing left in the pool"""
    st, dv = s.stats(), s.device()
    assert dv["violations"] == 0 and dv["dup_slots"] == 0
    assert st["messages"] == n_messages
    assert st["compressions"] == total_len_blocks
    assert st["uploaded"] == 128 * total_len_blocks == dv["copy_bytes"]
    assert st["chunks"] == 0
    return st, dv


@pytest.mark.parametrize("s_blocks", [1, 2, 3])
def test_whole_messages_at_the_block_and_chunk_edges(stream, s_blocks):
    lens = edge_lengths(s_blocks)
    rnd = random.Random(100 + s_blocks)
    msgs = [rnd.randbytes(n) for n in lens]
    s = stream(s_blocks, 16, 8, len(msgs))
    for i, m in enumerate(msgs):
        assert s.submit(m, i) == 0
    assert s.flush() == 0
    for i, m in enumerate(msgs):
        assert s.result(i) == (1, 0, b2(m)), lens[i]
    st, dv = check_clean(s, sum(nblocks(n) for n in lens), len(msgs))
    assert dv["rec_blocks"] <= s_blocks  # a record is never longer than the slice
    # the longest message needs at least ceil(nb / S) ticks: slicing really happened
    assert st["ticks"] >= -(-nblocks(max(lens)) // s_blocks)
    assert s.close() == 0


@pytest.mark.parametrize("s_blocks", [1, 2, 3])
@pytest.mark.parametrize("piece", [0, 1, 127, 128, 129])
def test_piecewise_updates_of_one_size(stream, s_blocks, piece):
    """updates of `piece` bytes (0: every message is built from empty updates plus one whole one):
    exactly max(1, ceil(L / 128)) compressions a message, the last of them only after finish"""
    lens = [n for n in edge_lengths(s_blocks) if piece or n <= 257]
    rnd = random.Random(7 * s_blocks + piece)
    s = stream(s_blocks, 16, 4, len(lens))
    total = 0
    for i, n in enumerate(lens):
        m = rnd.randbytes(n)
        mid = s.begin(i)
        if piece == 0:
            assert s.update(mid, b"") == 0 and s.update(mid, m) == 0 and s.update(mid, b"") == 0
        else:
            for o in range(0, n, piece):
                assert s.update(mid, m[o:o + piece]) == 0
        before = s.stats()["compressions"]
        assert s.finish(mid) == 0
        assert s.flush() == 0
        assert s.result(i) == (1, 0, b2(m)), (n, piece)
        total += nblocks(n)
        # exactly max(1, ceil(L / 128)) compressions, and at least the last one waited for finish
        assert s.stats()["compressions"] == total and before < total
        assert s.update(mid, b"x") == ERR_ARG and s.finish(mid) == ERR_ARG  # the id is spent
    check_clean(s, total, len(lens))


def test_hold_back_releases_all_but_the_last_buffered_block(stream):
    """an unfinished message of B buffered bytes has had floor((B - 1) / 128) blocks run, never its
    last buffered block, even a full one; finish right after an exact multiple adds one compression"""
    s = stream(2, 16, 4, 20)
    mid = s.begin(0)
    m = random.Random(3).randbytes(5 * 128)
    fed = barriers = 0
    for step in (1, 127, 1, 127, 128, 256):  # buffered: 1, 128, 129, 256, 384, 640
        assert s.update(mid, m[fed:fed + step]) == 0
        fed += step
        # A flush does not wait for an unfinished message, so empty messages serve as barriers: the
        # tick that runs one was planned after the update, and a tick takes blocks of every message
        # that has some (to the end of a chunk, so the 2 blocks of the last step may need 2 ticks).
        for _ in range(3):
            barriers += 1
            assert s.submit(b"", barriers) == 0 and s.flush() == 0
        assert s.stats()["compressions"] - barriers == (fed - 1) // 128, fed
    assert s.finish(mid) == 0 and s.flush() == 0
    assert s.stats()["compressions"] - barriers == 5
    assert s.result(0) == (1, 0, b2(m))


def test_seeded_random_pieces_two_messages_interleaved(stream):
    rnd = random.Random(11)
    s = stream(3, 16, 4, 40)
    total = 0
    for k in range(20):
        a, b = rnd.randbytes(rnd.randrange(0, 3000)), rnd.randbytes(rnd.randrange(0, 3000))
        ia, ib = s.begin(2 * k), s.begin(2 * k + 1)
        oa = ob = 0
        while oa < len(a) or ob < len(b):
            na, nb_ = rnd.randrange(0, 400), rnd.randrange(0, 400)
            assert s.update(ia, a[oa:oa + na]) == 0 and s.update(ib, b[ob:ob + nb_]) == 0
            oa, ob = oa + na, ob + nb_
        assert s.finish(ib) == 0 and s.finish(ia) == 0
        total += nblocks(len(a)) + nblocks(len(b))
        assert s.flush() == 0
        assert s.result(2 * k) == (1, 0, b2(a)) and s.result(2 * k + 1) == (1, 0, b2(b))
    check_clean(s, total, 40)


def test_finish_with_no_data(stream):
    s = stream(2, 16, 4, 3)
    ids = [s.begin(i) for i in range(3)]
    for i in ids:
        assert s.finish(i) == 0
    assert s.flush() == 0
    assert [s.result(i) for i in range(3)] == [(1, 0, b2(b""))] * 3
    check_clean(s, 3, 3)


def test_slot_and_chunk_reuse_with_a_message_larger_than_the_pool(stream):
    """64 messages through 4 slots and 8 chunks of 2 blocks (a 2 KiB pool); one message is 5 KiB"""
    rnd = random.Random(64)
    lens = [rnd.randrange(0, 900) for _ in range(64)]
    lens[17] = 5 * 1024 + 3
    lens[40] = 8 * 2 * 128  # exactly the pool
    msgs = [rnd.randbytes(n) for n in lens]
    s = stream(2, 8, 4, 64)
    for i, m in enumerate(msgs):
        assert s.submit(m, i) == 0
    assert s.flush() == 0
    assert [s.result(i) for i in range(64)] == [(1, 0, b2(m)) for m in msgs]
    st, dv = check_clean(s, sum(nblocks(n) for n in lens), 64)
    assert st["chunks_peak"] <= 8 and st["tick_messages"] <= 4 and dv["tick_recs"] <= 4
    # (the 5 KiB message took 21 chunks' worth of an 8-chunk pool: chunks came back as ticks ran)
    assert dv["busy_on"] == dv["busy_off"] >= 1  # in flight / idle, as the load table is told
    assert dv["copies"] <= st["compressions"]  # adjacent ranges merge: never more copies than blocks


def test_concurrent_submitters(stream):
    rnd = random.Random(5)
    msgs = [rnd.randbytes(rnd.choice([0, 1, 128, 511, 512, 513, 1024, rnd.randrange(0, 3000)])) for _ in range(200)]
    s = stream(4, 16, 8, 200)
    rcs = []

    def work(k):
        for i in range(k, 200, 4):
            rcs.append(s.submit(msgs[i], i))
    th = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert s.flush() == 0 and rcs == [0] * 200
    assert [s.result(i) for i in range(200)] == [(1, 0, b2(m)) for m in msgs]
    st, _ = check_clean(s, sum(nblocks(len(m)) for m in msgs), 200)
    assert st["chunks_peak"] <= 16


def test_bincode_batches_and_malformed_buffers(stream, lib):
    with open(os.path.join(ROOT, "tests", "golden", "worker_batches.json")) as f:
        g = json.load(f)
    good = [(bytes.fromhex(b["serialized"]), b["digest"]) for b in g["batches"] if "serialized" in b]
    bad = [(bytes.fromhex(m["hex"]), int(m["err_offset"])) for m in g["malformed"]]
    assert good and bad
    s = stream(2, 64, 8, len(good) + len(bad))
    for i, (buf, _) in enumerate(good):
        assert s.submit_serialized(buf, i) == (0, -1)
    for j, (buf, off) in enumerate(bad):
        # accepted; the offset is known at once, the callback reports the error
        assert s.submit_serialized(buf, len(good) + j) == (0, off)
    assert s.flush() == 0
    for i, (_, dig) in enumerate(good):
        n, res, d = s.result(i)
        assert (n, res, d.hex()) == (1, 0, dig)
    for j in range(len(bad)):
        # as nwv_batch_digest_serialized: the digest slot holds the digest of no bytes
        assert s.result(len(good) + j) == (1, ERR_ARG, b2(b""))
    assert s.device()["violations"] == 0
    # the walk alone: a count that promises more transactions than the buffer holds, a length that
    # runs past the end, trailing bytes (ignored, as k_batch_compact ignores them)
    import struct
    tx = [b"ab", b"", b"cdefg"]
    ok = struct.pack("<IQ", 0, 3) + b"".join(struct.pack("<Q", len(t)) + t for t in tx)
    pay = ctypes.c_uint64(0)
    assert lib.dsx_walk(ok, len(ok), ctypes.byref(pay)) == -1 and pay.value == 7
    assert lib.dsx_walk(ok + b"zz", len(ok) + 2, ctypes.byref(pay)) == -1 and pay.value == 7
    assert lib.dsx_walk(ok, len(ok) - 1, ctypes.byref(pay)) == 12 + 8 + 2 + 8
    more = struct.pack("<IQ", 0, 4) + ok[12:]
    assert lib.dsx_walk(more, len(more), ctypes.byref(pay)) == len(more)
    assert lib.dsx_walk(ok, 11, ctypes.byref(pay)) == 4


def test_close_fails_never_finished_messages_and_completes_finished_ones(stream):
    s = stream(2, 16, 4, 3)
    a, b = s.begin(0), s.begin(1)
    m = random.Random(8).randbytes(700)
    assert s.update(a, m) == 0 and s.update(b, m) == 0
    assert s.finish(b) == 0
    assert s.submit(m[:300], 2) == 0
    assert s.close() == 0
    assert s.result(0)[:2] == (1, ERR_ARG)  # never finished
    assert s.result(1) == (1, 0, b2(m)) and s.result(2) == (1, 0, b2(m[:300]))
    # the stream is closed: every call fails, nothing fires twice
    assert s.submit(b"x", 2) == ERR_ARG and s.flush() == ERR_ARG and s.close() == ERR_ARG
    assert s.update(a, b"x") == ERR_ARG and s.finish(a) == ERR_ARG
    assert [s.result(i)[0] for i in range(3)] == [1, 1, 1]
    assert s.stats()["chunks"] == 0 and s.device()["busy_on"] == s.device()["busy_off"]


def test_waiting_calls_from_inside_a_callback_return_reentrant(stream, lib):
    s = stream(2, 8, 4, 4)
    lib.dsx_set_mode(s.h, 0, 1)  # tag 0's callback calls flush, close and an over-the-pool submit
    assert s.submit(b"abc", 0) == 0 and s.flush() == 0
    out = np.zeros(3, dtype=np.int32)
    lib.dsx_reentrant(s.h, out.ctypes.data)
    assert out.tolist() == [ERR_REENTRANT] * 3
    # a submission that fits goes through from a callback, and completes
    lib.dsx_set_mode(s.h, 1, 2)
    chained = random.Random(2).randbytes(600)
    lib.dsx_set_chained(s.h, chained, len(chained))
    assert s.submit(b"first", 1) == 0
    assert s.flush() == 0  # (tag 1 only: tag 2 was submitted after the call began)
    assert s.result(1) == (1, 0, b2(b"first"))
    assert s.flush() == 0 and lib.dsx_chain_rc(s.h) == 0
    assert s.result(2) == (1, 0, b2(chained))
    assert s.device()["violations"] == 0 and s.close() == 0


def test_config_needs_two_chunks_a_message(lib):
    assert not lib.dsx_new(2, 7, 4, 0) and not lib.dsx_new(0, 8, 4, 0) and not lib.dsx_new(2, 8, 0, 0)
    h = lib.dsx_new(2, 8, 4, 0)
    assert h
    lib.dsx_free(h)


def test_the_threaded_stream_is_clean_under_the_thread_sanitizer(tmp_path):
    """digest_stream_stub.cpp as a stand-alone program (its own main: four submitting threads, whole
    and piecewise, over 8 slots and 16 chunks), built with -fsanitize=thread and run on the CPU; never
    loaded into Python.  Sanitizer runs stay off machines with a GPU (skipped where the compute
    device node exists); also skipped where the compiler cannot link the sanitizer's runtime or the
    runtime cannot map its shadow memory on this kernel."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer runs are for CPU-only machines")
    exe = str(tmp_path / "dstream_tsan")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    b = subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "--offload-host-only", "-x", "hip", "-pthread",
                        "-fsanitize=thread", "-DDSTREAM_STUB_MAIN", "-o", exe, STUB],
                       capture_output=True, text=True, timeout=300)
    if b.returncode != 0:
        pytest.skip("cannot build with -fsanitize=thread here: " + b.stderr[-300:])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if "unexpected memory mapping" in p.stderr:
        pytest.skip("the thread sanitizer's runtime cannot start on this kernel")
    print(p.stdout.strip())
    assert p.returncode == 0 and "WARNING: ThreadSanitizer" not in p.stderr, p.stdout + p.stderr[-3000:]
    assert "800 messages, ok" in p.stdout
