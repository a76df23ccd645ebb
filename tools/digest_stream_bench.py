#!/usr/bin/env python3
"""The digest stream (include/nwv_digest_stream.h) against the one-call digests and the host, on
config 5's worker batches (977 x 512 B transactions, 500,224 payload bytes, serialized).

  digest_stream_bench.py worker --cases a,b,... [--slice S] [--rounds R] [--reps N]
      one process, one JSON line; the library is the one NWV_LIB names (narwhal_amd/lib/), so the
      parent commit's build runs the one-call cases through the same script.
        onecall1 / onecall4   nwv_batch_digest_serialized of the 100 batches in one call, R rounds from
                              one thread / split over four threads calling at once -> ms a round
        stream1 / stream4     the same 100 batches a round submitted to one stream continuously from one
                              / four threads, no waiting between rounds, flush at the end -> ms a round
        host16                hashlib.blake2b of the 100 payloads on 16 host threads (bench.py's C5 host
                              figure) -> ms a round
        processor             k in {1, 4, 16} threads in a closed loop, one batch each: submit and wait
                              for its callback, against nwv_batch_digest_serialized(n = 1) -> batches/s
                              (the stream half only where the library has one)
        lone                  one batch alone: stream submit-and-wait against the direct call -> ms
        beside                C1 certificate and 1,024-signature verify_batch p50 / p99 beside four
                              threads of one-call digests, and beside a stream that four threads keep
                              saturated (tools/qos_lat.py's foreground and pacing)
      Every shape is warmed first; the host clock brackets work that ends in a flush, a completed
      callback or a returned blocking call; every digest is checked against hashlib.
  digest_stream_bench.py all --parent libnwv_parent.so [--runs 3] [--out profiles/digest_stream_sweep.json]
      fresh worker processes, the parent's library and this one alternating, `runs` times; then the
      slice sweep (64 .. 1024) on this library, `runs` processes a value; medians, the parent's own
      run-to-run spread, the default-slice rule and the recommendation rule are
      worked out into "summary".  Every worker runs under its own time limit and the script stops at
      the first failure.
  digest_stream_bench.py headline --parent libnwv_parent.so [--runs 3] [--out profiles/digest_stream_headline_ab.json]
      plain bench.py with --dump-outputs, parent and new alternating; compares the dumped outputs."""
import argparse
import ctypes
import hashlib
import json
import os
import struct
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
N_BATCH, N_TX, TX = 100, 977, 512
SLICES = (64, 128, 256, 512, 1024)


def make_batches():
    """100 serialized config-5 batches (seeded) and their digests"""
    import numpy as np
    rng = np.random.default_rng(55)
    bufs, want = [], []
    for _ in range(N_BATCH):
        tx = rng.integers(0, 256, size=(N_TX, TX), dtype=np.uint8)
        rec = np.zeros((N_TX, 8 + TX), dtype=np.uint8)
        rec[:, :8] = np.frombuffer(struct.pack("<Q", TX), dtype=np.uint8)
        rec[:, 8:] = tx
        bufs.append(struct.pack("<IQ", 0, N_TX) + rec.tobytes())
        want.append(hashlib.blake2b(tx.tobytes(), digest_size=32).digest())
    return bufs, want


class Bench:
    def __init__(self, a):
        import numpy as np
        import narwhal_amd
        from narwhal_amd import _lib
        self.np, self._lib, self.a = np, _lib, a
        self.eng = narwhal_amd.Engine(device=0)
        self.lib, self.h = self.eng.lib, self.eng._h
        self.bufs, self.want = make_batches()
        self.has_stream = hasattr(self.lib, "nwv_dstream_open")
        lens = np.array([len(b) for b in self.bufs], dtype=np.uint64)
        self.arena = np.frombuffer(b"".join(self.bufs) + b"\0" * 16, dtype=np.uint8)
        self.offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
        self.lens = lens

    # ---- the one-call form ----
    def onecall(self, lo=0, n=N_BATCH, check=False):
        np, p = self.np, self._lib._ptr
        out = np.zeros(32 * n, dtype=np.uint8)
        err = np.zeros(n, dtype=np.int64)
        self._lib._check(self.lib.nwv_batch_digest_serialized(self.h, n, p(self.arena), self.offs[lo:].ctypes.data,
                                                              self.lens[lo:].ctypes.data, p(out), p(err)))
        if check:
            assert [out[32 * i:32 * i + 32].tobytes() for i in range(n)] == self.want[lo:lo + n]

    def onecall_rounds(self, threads):
        R = self.a.rounds
        for _ in range(2):
            self.onecall(check=True)
        per = [R // threads + (1 if k < R % threads else 0) for k in range(threads)]

        def work(k):
            for _ in range(per[k]):
                self.onecall()
        th = [threading.Thread(target=work, args=(k,)) for k in range(threads)]
        t = time.perf_counter()
        for x in th:
            x.start()
        for x in th:
            x.join()
        return {"ms_per_round": (time.perf_counter() - t) * 1e3 / R, "rounds": R, "threads": threads}

    # ---- the stream, callbacks off: completion is the flush ----
    def open_stream(self):
        sid = self.lib.nwv_dstream_open(self.h, 0, self.a.slice, self.a.pool_chunks, self.a.max_messages)
        if sid < 0:
            self._lib._check(sid)
        return sid

    def submit_raw(self, sid, i, out, slot):
        err = ctypes.c_int64(0)
        b = self.bufs[i]
        rc = self.lib.nwv_dstream_submit_serialized(self.h, sid, b, len(b), out[slot].ctypes.data, ctypes.byref(err),
                                                    None, None)
        assert rc == 0 and err.value == -1, (rc, err.value)

    def stream_rounds(self, threads):
        np, R, warm = self.np, self.a.rounds, 3
        sid = self.open_stream()
        out = np.zeros((R + warm, N_BATCH, 32), dtype=np.uint8)

        def work(k, r0, r1):
            for r in range(r0, r1):
                for i in range(k, N_BATCH, threads):
                    self.submit_raw(sid, i, out[r], i)

        def run(r0, r1):
            th = [threading.Thread(target=work, args=(k, r0, r1)) for k in range(threads)]
            for x in th:
                x.start()
            for x in th:
                x.join()
            self._lib._check(self.lib.nwv_dstream_flush(self.h, sid))
        run(0, warm)
        t = time.perf_counter()
        run(warm, warm + R)
        dt = time.perf_counter() - t
        for r in (0, warm, warm + R - 1):
            assert [out[r, i].tobytes() for i in range(N_BATCH)] == self.want, r
        st = np.zeros(8, dtype=np.uint64)
        self._lib._check(self.lib.nwv_dstream_stats(self.h, sid, st.ctypes.data))
        self._lib._check(self.lib.nwv_dstream_close(self.h, sid))
        return {"ms_per_round": dt * 1e3 / R, "rounds": R, "threads": threads, "slice": self.a.slice,
                "ticks": int(st[1]), "most_messages_in_a_tick": int(st[4]), "peak_chunks": int(st[6]),
                "submissions_that_waited": int(st[7])}

    def host16(self):
        from concurrent.futures import ThreadPoolExecutor
        pay = [self.np.frombuffer(b[12:], dtype=self.np.uint8).reshape(N_TX, 8 + TX)[:, 8:].tobytes() for b in self.bufs]
        with ThreadPoolExecutor(16) as ex:
            f = lambda: list(ex.map(lambda m: hashlib.blake2b(m, digest_size=32).digest(), pay))  # noqa: E731
            assert f() == self.want
            ts = []
            for _ in range(5):
                t = time.perf_counter()
                f()
                ts.append(time.perf_counter() - t)
        return {"ms_per_round": sorted(ts)[len(ts) // 2] * 1e3, "threads": 16, "kind": "port",
                "what": "hashlib.blake2b(digest_size=32) of the 100 payloads on a 16-thread pool, median of 5"}

    # ---- the Processor pattern: k threads, one batch each, closed loop ----
    def closed_loop(self, k, one):
        stop = time.perf_counter() + self.a.seconds
        done = [0] * k

        def work(j):
            i = j
            while time.perf_counter() < stop:
                one(i % N_BATCH)
                i += k
                done[j] += 1
        th = [threading.Thread(target=work, args=(j,)) for j in range(k)]
        t = time.perf_counter()
        for x in th:
            x.start()
        for x in th:
            x.join()
        return sum(done) / (time.perf_counter() - t)

    def processor(self):
        from narwhal_amd.digest_stream import DigestStream
        out = {}
        ds = DigestStream(self.eng, 0, self.a.slice, self.a.pool_chunks, self.a.max_messages) if self.has_stream else None

        def via_stream(i):
            assert ds.submit_serialized(self.bufs[i]).digest(60) == self.want[i]
        for k in (1, 4, 16):
            for _ in range(3):
                self.onecall(0, 1, check=True)
            out[f"k{k}"] = {"onecall_batches_per_s": self.closed_loop(k, lambda i: self.onecall(i, 1))}
            if ds:
                for i in range(3):
                    via_stream(i)
                out[f"k{k}"]["stream_batches_per_s"] = self.closed_loop(k, via_stream)
        if ds:
            ds.close()
        return out

    def lone(self):
        from narwhal_amd.digest_stream import DigestStream
        np = self.np

        def med(f, reps=self.a.reps):
            for _ in range(5):
                f()
            ts = []
            for _ in range(reps):
                t = time.perf_counter()
                f()
                ts.append(time.perf_counter() - t)
            return float(np.median(ts) * 1e3)
        out = {"onecall_ms": med(lambda: self.onecall(0, 1))}
        if self.has_stream:
            with DigestStream(self.eng, 0, self.a.slice, self.a.pool_chunks, self.a.max_messages) as ds:
                out["stream_ms"] = med(lambda: ds.submit_serialized(self.bufs[0]).wait(60))
                assert ds.submit_serialized(self.bufs[0]).digest(60) == self.want[0]
                out["slice"] = self.a.slice
        return out

    def beside(self):
        import qos_lat as Q
        np = self.np
        c = Q.Calls(self.eng, ["ed_digest"])
        reps = self.a.reps
        fg = {"certificate": (c.certificate, reps), "batch_1024": (lambda: c.verify_batch(c.b1k), reps)}
        out = {"beside_four_threads_of_onecall_digests": Q.loaded(fg, c.digests, 4, N_BATCH)}
        if self.has_stream:
            sid = self.open_stream()
            sink = np.zeros((4, N_BATCH, 32), dtype=np.uint8)
            tl = threading.local()
            ids = iter(range(4))

            def load():  # 25 batches a call; the pool's backpressure paces the four threads
                if not hasattr(tl, "k"):
                    tl.k = next(ids)
                for i in range(tl.k, N_BATCH, 4):
                    self.submit_raw(sid, i, sink[tl.k], i)
            out["beside_a_saturated_stream"] = Q.loaded(fg, load, 4, N_BATCH // 4)
            self._lib._check(self.lib.nwv_dstream_flush(self.h, sid))
            assert [sink[i % 4, i].tobytes() for i in range(N_BATCH)] == self.want
            self._lib._check(self.lib.nwv_dstream_close(self.h, sid))
        return out


def worker(a):
    b = Bench(a)
    out = {"lib": os.environ.get("NWV_LIB", "libnwv.so"), "has_stream": b.has_stream}
    for case in a.cases.split(","):
        if case in ("stream1", "stream4") and not b.has_stream:
            continue
        out[case] = {"onecall1": lambda: b.onecall_rounds(1), "onecall4": lambda: b.onecall_rounds(4),
                     "stream1": lambda: b.stream_rounds(1), "stream4": lambda: b.stream_rounds(4), "host16": b.host16,
                     "processor": b.processor, "lone": b.lone, "beside": b.beside}[case]()
    b.eng.close()
    print(json.dumps(out), flush=True)


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def summarize(res):
    par, new, sw = res["runs"]["parent"], res["runs"]["new"], res["sweep"]
    s = {}
    p1 = [r["onecall1"]["ms_per_round"] for r in par]
    s["parent_onecall1_ms"] = {"runs": p1, "median": _median(p1)}
    spread = (max(p1) - min(p1)) / _median(p1)
    s["spread"] = spread
    s["spread_source"] = "(max - min) / median of the parent library's own onecall1 runs"
    for key in ("onecall1", "onecall4", "stream1", "stream4", "host16"):
        v = [r[key]["ms_per_round"] for r in new if key in r]
        if v:
            s["new_" + key + "_ms"] = {"runs": v, "median": _median(v)}
    p4 = [r["onecall4"]["ms_per_round"] for r in par]
    s["parent_onecall4_ms"] = {"runs": p4, "median": _median(p4)}
    # the slice sweep: the smallest slice whose steady round rate is within the spread of the best
    rounds = {S: _median([r["stream1"]["ms_per_round"] for r in sw[str(S)]]) for S in SLICES if sw.get(str(S))}
    lone = {S: _median([r["lone"]["stream_ms"] for r in sw[str(S)]]) for S in SLICES if sw.get(str(S))}
    s["sweep_stream1_ms_per_round"], s["sweep_lone_stream_ms"] = rounds, lone
    if rounds:
        best = min(rounds.values())
        s["default_slice_by_rule"] = min(S for S, v in rounds.items() if v <= best * (1 + spread))
    # the recommendation rule: new <= parent x (1 - max(0.10, 2 spread)), against the one-call form and the host
    margin = max(0.10, 2 * spread)
    s["margin"] = margin
    host = s.get("new_host16_ms", {}).get("median")
    rec = {}
    for shape, mine, theirs in (("rounds_from_one_thread", "new_stream1_ms", "parent_onecall1_ms"),
                                ("rounds_from_four_threads", "new_stream4_ms", "parent_onecall4_ms")):
        if mine in s and host is not None:
            m = s[mine]["median"]
            rec[shape] = {"stream_ms": m, "onecall_ms": s[theirs]["median"], "host16_ms": host,
                          "recommend_stream": bool(m <= s[theirs]["median"] * (1 - margin) and m <= host * (1 - margin))}
    proc = {}
    for k in ("k1", "k4", "k16"):
        a = [r["processor"][k]["stream_batches_per_s"] for r in new if "processor" in r]
        o = [r["processor"][k]["onecall_batches_per_s"] for r in par if "processor" in r]
        if a and o:
            proc[k] = {"stream_batches_per_s": _median(a), "parent_onecall_batches_per_s": _median(o),
                       "recommend_stream_over_onecall": bool(_median(a) >= _median(o) / (1 - margin))}
    s["recommendation"], s["processor"] = rec, proc
    ln = [r["lone"] for r in new if "lone" in r]
    if ln:
        s["lone_ms"] = {"stream": _median([x["stream_ms"] for x in ln]), "onecall": _median([x["onecall_ms"] for x in ln]),
                        "parent_onecall": _median([r["lone"]["onecall_ms"] for r in par if "lone" in r])}
    bs = [r["beside"] for r in new if "beside" in r]
    if bs:
        s["beside_p50_ms"] = {
            load: {fg: _median([x[load][fg]["p50_ms"] for x in bs]) for fg in ("certificate", "batch_1024")}
            for load in ("beside_four_threads_of_onecall_digests", "beside_a_saturated_stream")}
        s["beside_load_batches_per_s"] = {
            load: _median([x[load]["load_items_per_s"] for x in bs])
            for load in ("beside_four_threads_of_onecall_digests", "beside_a_saturated_stream")}
    return s


def run_all(a):
    import qos_lat as Q
    me = os.path.abspath(__file__)
    res = {"what": __doc__.split("\n\n")[0] + "  Fresh worker processes, the parent commit's library and this one "
           "alternating in one session on one MI355X (tools/digest_stream_bench.py all).",
           "rounds": a.rounds, "reps": a.reps, "seconds": a.seconds, "runs": {"parent": [], "new": []}, "sweep": {}}

    def child(lib, cases, slice_blocks, limit):
        env = dict(os.environ, NWV_LIB=lib)
        args = [sys.executable, me, "worker", "--cases", cases, "--slice", str(slice_blocks), "--rounds", str(a.rounds),
                "--reps", str(a.reps), "--seconds", str(a.seconds)]
        t = time.time()
        out = Q._child(args, env, limit)
        print(f"{lib} {cases} slice {slice_blocks}: {time.time() - t:.1f} s", flush=True)
        return out

    def save():
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    for r in range(a.runs):
        res["runs"]["parent"].append(child(a.parent, "onecall1,onecall4,processor,lone", 0, 240))
        save()
        res["runs"]["new"].append(child("libnwv.so", "onecall1,onecall4,stream1,stream4,host16,processor,lone,beside",
                                        0, 400))
        save()
    for S in SLICES:
        res["sweep"][str(S)] = [child("libnwv.so", "stream1,lone", S, 200) for _ in range(a.runs)]
        save()
    res["summary"] = summarize(res)
    save()
    print(json.dumps({"written": a.out, "summary": res["summary"]}), flush=True)


def headline(a):
    import numpy as np
    import qos_lat as Q
    res = {"what": "plain bench.py (--gpus 1, its default steps and warm-up) with --dump-outputs, the parent commit's "
           "library and this one alternating in one session on one MI355X, value in sigs/s "
           "(tools/digest_stream_bench.py headline).  bench.py never opens a digest stream.",
           "order_in_each_pair": "new, parent" if a.new_first else "parent, new", "runs": {"parent": [], "new": []}}
    dumps = {}
    for r in range(a.runs):
        sides = (("parent", a.parent), ("new", "libnwv.so"))
        for name, lib in (sides[::-1] if a.new_first else sides):
            d = os.path.join(ROOT, "bench_outputs", f"dstream_dump_{name}_{r}")
            line = Q._child([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", d],
                            dict(os.environ, NWV_LIB=lib), 400)
            res["runs"][name].append({"value": line["value"]})
            res.setdefault("metric", line.get("metric"))
            dumps[(name, r)] = d
            print(f"run {r} {name}: {line['value']:.4g}", flush=True)
    same, ref = True, dumps[("parent", 0)]
    for d in dumps.values():
        for fn in sorted(os.listdir(ref)):
            x, y = np.load(os.path.join(ref, fn), allow_pickle=False), np.load(os.path.join(d, fn), allow_pickle=False)
            same = same and x.shape == y.shape and bool((x == y).all())
    for name in ("parent", "new"):
        v = [x["value"] for x in res["runs"][name]]
        res[name + "_median"] = float(np.median(v))
        res[name + "_range"] = [min(v), max(v)]
    res["new_median_inside_parent_range"] = res["parent_range"][0] <= res["new_median"] <= res["parent_range"][1]
    res["dumped_outputs_identical"] = same
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out, "identical": same, "inside": res["new_median_inside_parent_range"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    w = sub.add_parser("worker")
    w.add_argument("--cases", required=True)
    for p in (w, sub.add_parser("all")):
        p.add_argument("--slice", type=int, default=0)
        p.add_argument("--pool-chunks", type=int, default=0)
        p.add_argument("--max-messages", type=int, default=0)
        p.add_argument("--rounds", type=int, default=50)
        p.add_argument("--reps", type=int, default=100)
        p.add_argument("--seconds", type=float, default=1.5)
        if p is not w:
            p.add_argument("--parent", required=True)
            p.add_argument("--runs", type=int, default=3)
            p.add_argument("--out", default=os.path.join(ROOT, "profiles", "digest_stream_sweep.json"))
    h = sub.add_parser("headline")
    h.add_argument("--parent", required=True)
    h.add_argument("--runs", type=int, default=3)
    h.add_argument("--new-first", action="store_true", help="each pair runs this library first, then the parent's")
    h.add_argument("--out", default=os.path.join(ROOT, "profiles", "digest_stream_headline_ab.json"))
    a = ap.parse_args()
    if a.cmd == "worker":
        worker(a)
    elif a.cmd == "all":
        run_all(a)
    else:
        headline(a)


if __name__ == "__main__":
    main()
