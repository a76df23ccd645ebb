"""The digest stream on the GPU (include/nwv_digest_stream.h, k_blake2b_slice): digests against
hashlib and against the one-call forms on the same inputs, slicing shown by the tick count,
piecewise and concurrent submission, the bincode walk against nwv_batch_digest_serialized, the
config-5 batch and round, verification beside a busy stream, reentrancy and id reuse.
tests/test_digest_stream_host.py checks the stream's host side alone."""
import hashlib
import random
import struct
import threading

import pytest

import oracle_ffi as of

pytestmark = pytest.mark.gpu


def b2(m):
    return hashlib.blake2b(m, digest_size=32).digest()


def nblocks(n):
    return max(1, -(-n // 128))


def edge_lengths(s):
    return [0, 1, 127, 128, 129, 255, 256, 257, s * 128 - 1, s * 128, s * 128 + 1, 2 * s * 128, 3 * s * 128 + 5]


@pytest.fixture(scope="module")
def eng():
    import narwhal_amd
    e = narwhal_amd.Engine(device=0)
    yield e
    e.close()


def worker_batch(rnd, b=1):
    """a config-5 worker batch: 977 x 512 B (node/src/benchmark_client.rs:153-168 layout), serialized"""
    txs = [(bytes([b % 2]) + struct.pack(">Q", rnd.getrandbits(64))).ljust(512, b"\0") for _ in range(977)]
    ser = struct.pack("<IQ", 0, len(txs)) + b"".join(struct.pack("<Q", len(t)) + t for t in txs)
    return ser, b2(b"".join(txs))


def test_slicing_really_happens(eng):
    from narwhal_amd import DigestStream
    rnd = random.Random(9)
    lens = edge_lengths(2) + [rnd.randrange(0, 3000) for _ in range(40)]
    msgs = [rnd.randbytes(n) for n in lens]
    want = [b2(m) for m in msgs]
    with DigestStream(eng, device_index=0, slice_blocks=2, pool_chunks=64, max_messages=16) as ds:
        ps = [ds.submit(m) for m in msgs]
        ds.flush()
        assert [p.digest(0) for p in ps] == want
        assert [p.fired for p in ps] == [1] * len(ps)
        st = ds.stats()
    assert eng.blake2b256_many(msgs) == want
    assert st["ticks"] >= -(-nblocks(max(lens)) // 2)
    assert st["messages"] == len(msgs) and st["chunks"] == 0
    assert st["compressions"] == sum(nblocks(n) for n in lens) and st["uploaded"] == 128 * st["compressions"]
    assert st["tick_messages"] <= 16 and st["chunks_peak"] <= 64


@pytest.mark.parametrize("piece", [0, 1, 127, 128, 129])
def test_piecewise_updates_two_messages_interleaved(eng, piece):
    from narwhal_amd import DigestStream
    rnd = random.Random(20 + piece)
    lens = [n for n in edge_lengths(3) if piece > 1 or n <= 257]
    with DigestStream(eng, device_index=0, slice_blocks=3, pool_chunks=16, max_messages=4) as ds:
        for n in lens:
            a, b = rnd.randbytes(n), rnd.randbytes(max(0, n - 1))
            pa, pb = ds.begin(), ds.begin()
            if piece == 0:
                pa.update(b"").update(a).update(b"")
                pb.update(b).update(b"")
            else:
                for o in range(0, n, piece):
                    pa.update(a[o:o + piece])
                    pb.update(b[o:o + piece])
            pb.finish()
            pa.finish()
            assert (pa.digest(30), pb.digest(30)) == (b2(a), b2(b)), (n, piece)
        st = ds.stats()
    assert st["compressions"] == sum(nblocks(n) + nblocks(max(0, n - 1)) for n in lens)


def test_seeded_random_pieces(eng):
    from narwhal_amd import DigestStream
    rnd = random.Random(31)
    with DigestStream(eng, device_index=0, slice_blocks=4, pool_chunks=16, max_messages=4) as ds:
        for _ in range(12):
            a, b = rnd.randbytes(rnd.randrange(0, 4000)), rnd.randbytes(rnd.randrange(0, 4000))
            pa, pb = ds.begin(), ds.begin()
            oa = ob = 0
            while oa < len(a) or ob < len(b):
                na, nb_ = rnd.randrange(0, 500), rnd.randrange(0, 500)
                pa.update(a[oa:oa + na])
                pb.update(b[ob:ob + nb_])
                oa, ob = oa + na, ob + nb_
            pa.finish()
            pb.finish()
            assert (pa.digest(30), pb.digest(30)) == (b2(a), b2(b))


def test_concurrent_submitters(eng):
    from narwhal_amd import DigestStream
    rnd = random.Random(5)
    msgs = [rnd.randbytes(rnd.choice([0, 1, 128, 511, 512, 513, 1024, rnd.randrange(0, 3000)])) for _ in range(200)]
    msgs[77] = rnd.randbytes(16 * 4 * 128 + 77)  # larger than the whole pool
    fired = []
    ps = [None] * 200
    with DigestStream(eng, device_index=0, slice_blocks=4, pool_chunks=16, max_messages=8) as ds:
        def work(k):
            for i in range(k, 200, 4):
                ps[i] = ds.submit(msgs[i], callback=lambda p, i=i: fired.append(i))
        th = [threading.Thread(target=work, args=(k,)) for k in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        ds.flush()
        st = ds.stats()
    assert sorted(fired) == list(range(200)) and [p.fired for p in ps] == [1] * 200
    assert [p.digest(0) for p in ps] == [b2(m) for m in msgs]
    assert st["chunks_peak"] <= 16 and st["chunks"] == 0 and st["messages"] == 200


def test_serialized_batches_match_the_one_call_form(eng):
    from narwhal_amd import DigestStream
    from narwhal_amd.digest_stream import digest_results
    g = of.load_golden("worker_batches.json")
    bufs = [bytes.fromhex(b["serialized"]) for b in g["batches"] if "serialized" in b]
    bufs += [bytes.fromhex(m["hex"]) for m in g["malformed"]]
    with DigestStream(eng, device_index=0, slice_blocks=3, pool_chunks=32, max_messages=8) as ds:
        ps = [ds.submit_serialized(b) for b in bufs]
        ds.flush()
        got = digest_results(ps)
    assert got == eng.batch_digest_serialized(bufs)
    assert [d.hex() for d, e in got if e < 0] == [b["digest"] for b in g["batches"] if "serialized" in b]
    assert [e for _, e in got if e >= 0] == [int(m["err_offset"]) for m in g["malformed"]]
    assert [p.result for p in ps] == [0 if e < 0 else -1 for _, e in got]


def test_config5_batch_at_the_default_slice(eng):
    from narwhal_amd import DigestStream
    ser, want = worker_batch(random.Random(5))
    with DigestStream(eng) as ds:
        p = ds.submit_serialized(ser)
        assert p.digest(60) == want and p.err_offset == -1
        st = ds.stats()
    nb = nblocks(977 * 512)
    assert st["compressions"] == nb and st["ticks"] >= -(-nb // 1024)  # (the default slice: 1,024 blocks)


def test_hundred_worker_batches_round_submitted_at_once(eng):
    """the inputs and expectations of test_gpu_blake2b.py::test_hundred_worker_batches_dag_round"""
    from narwhal_amd import DigestStream
    rnd = random.Random(55)
    bufs, want = [], []
    for b in range(100):
        ser, d = worker_batch(rnd, b)
        bufs.append(ser)
        want.append(d)
    with DigestStream(eng) as ds:
        ps = [ds.submit_serialized(b) for b in bufs]
        ds.flush()
        assert [p.digest(0) for p in ps] == want
        assert ds.stats()["messages"] == 100


def test_a_busy_stream_beside_verify_batch(eng):
    """one thread keeps a stream busy, one runs verify_batch on the same context: both right"""
    from narwhal_amd import DigestStream
    g = of.load_golden("ed25519_vectors.json")
    items = [(bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"])) for v in g["vectors"]]
    expect = [v["expect"] for v in g["vectors"]]
    alone = eng.verify_batch(items, seed=b"\x07" * 32)  # before the stream exists
    assert list(alone[1]) == expect and alone[0] == all(expect)
    rnd = random.Random(12)
    msgs = [rnd.randbytes(rnd.randrange(20000, 60000)) for _ in range(24)]
    out = {}
    with DigestStream(eng, device_index=0, slice_blocks=16, pool_chunks=64, max_messages=8) as ds:
        def digests():
            out["ps"] = [ds.submit(m) for m in msgs]
            ds.flush()

        def verify():
            out["v"] = [eng.verify_batch(items, seed=bytes([k]) * 32) for k in range(6)]
        th = [threading.Thread(target=digests), threading.Thread(target=verify)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert [p.digest(0) for p in out["ps"]] == [b2(m) for m in msgs]
    for allv, bits in out["v"]:
        assert (allv, list(bits)) == (alone[0], expect)


def test_a_stream_with_messages_in_flight_is_one_outstanding_range(eng):
    """place.h's load table: from the first message begun until the last has completed"""
    from narwhal_amd import DigestStream
    base = eng.device_counters(0, 0)["outstanding"]
    with DigestStream(eng, device_index=0, slice_blocks=2, pool_chunks=8, max_messages=4) as ds:
        assert eng.device_counters(0, 0)["outstanding"] == base  # open and idle: no load
        p, q = ds.begin(), ds.begin()
        assert eng.device_counters(0, 0)["outstanding"] == base + 1  # one range, however many messages
        p.update(b"abc").finish()
        assert p.digest(30) == b2(b"abc")
        assert eng.device_counters(0, 0)["outstanding"] == base + 1  # q is still open
        q.finish()
        ds.flush()
        assert q.digest(0) == b2(b"") and eng.device_counters(0, 0)["outstanding"] == base


def test_reentrancy_and_id_reuse(eng):
    from narwhal_amd import DigestStream, NwvError
    seen = []
    ds = DigestStream(eng, device_index=0, slice_blocks=2, pool_chunks=8, max_messages=4)
    sid = ds.id

    def cb(p):
        try:
            ds.flush()
            seen.append(0)
        except NwvError as e:
            seen.append(e.code)
        try:
            ds.close()
            seen.append(0)
        except NwvError as e:
            seen.append(e.code)
    p = ds.submit(b"abc", callback=cb)
    assert p.digest(30) == b2(b"abc")
    assert seen == [-7, -7]  # NWV_ERR_REENTRANT
    # a never-finished message completes with NWV_ERR_ARG at close
    q = ds.begin().update(b"x" * 300)
    ds.close()
    assert (q.wait(30), q.fired, q.digest()) == (-1, 1, None)
    ds2 = DigestStream(eng, device_index=0, slice_blocks=2, pool_chunks=8, max_messages=4)
    assert ds2.id == sid
    assert ds2.submit(b"").digest(30) == b2(b"")
    ds2.close()
    assert eng.lib.nwv_dstream_flush(eng._h, sid) == -1  # NWV_ERR_ARG: the id is closed
