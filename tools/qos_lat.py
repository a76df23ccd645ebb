#!/usr/bin/env python3
"""Latency of protocol-sized calls alone and beside bulk callers, with and without the latency
class (nwv_set_latency_max, narwhal_amd/csrc/lane_pool.h).

  qos_lat.py worker [--on] [--hwq 16] [--reps N] [--legs unloaded,ed_batch,ed_digest,bls]
      one process, one JSON line.  The library is the one NWV_LIB names (narwhal_amd/lib/), so the
      parent commit's build runs through the same script (it has no setter: never with --on).
      --on sets the bounds (Ed25519 1,024: the foreground's largest call; BLS 2).  --hwq 16 sets
      GPU_MAX_HW_QUEUES=16 for this process before HIP starts, as bench.py does; without it the
      machine's default holds.
        unloaded   C1 certificate verify, verify_batch of 1,024, BLS single verify, one thread
        ed_batch   certificate and 1,024-batch beside four threads looping a host-to-host
                   65,536 x 32 B verify_batch
        ed_digest  the same beside four threads looping nwv_blake2b256_many of 100 x 500,224 B
        bls        BLS single verify beside two threads looping a 4,096-item call
      In the loaded legs the foreground rests 1 ms between calls (the same offered load in every
      state); they also report the load threads' aggregate rate (items/s) while the foreground ran.
  qos_lat.py ab --parent libnwv_parent.so [--runs 3] [--out profiles/qos_latency_ab.json]
      alternates fresh worker processes: parent, new with the bound off, new with it on, new with
      it on and NWV_LATENCY_PRIORITY=0 (reserved lanes at default priority), `runs` times, at the
      default hardware-queue count and at 16.  Every worker runs under its own time limit and the
      script stops at the first failure.
  qos_lat.py headline --parent libnwv_parent.so [--runs 3] [--out profiles/qos_headline_ab.json]
      plain bench.py with --dump-outputs, parent and new alternating; compares the dumped outputs."""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ED, BLS = 0, 1
R_BLS = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
PACE = 0.001  # the loaded legs' foreground rests this long between calls


def _pcts(xs):
    import numpy as np
    a = np.array(xs) * 1e3
    return {"p50_ms": float(np.percentile(a, 50)), "p99_ms": float(np.percentile(a, 99)), "reps": len(xs)}


class Calls:
    """the foreground and load calls, inputs packed once; every call asserts its result"""

    def __init__(self, eng, legs):
        import numpy as np
        import config_legs as CL
        from narwhal_amd import _lib
        from narwhal_amd import types as T
        from narwhal_amd.bls import Bls
        self.eng, self.lib, self._lib, self.np = eng, eng.lib, _lib, np
        seeds, keys, com = CL.committee_fixture(eng, 4, b"nwv-qos-c1")
        _, _, certs = CL.dag_round(eng, seeds, keys, com)
        T.verify(eng, com, certs[-1])
        self.keep = T._Keep()
        self.cc = com._c(self.keep)
        self.carr = (T._Certificate * 1)(certs[-1]._c(self.keep))
        self.tlib = T.lib()
        self.b1k = self.batch(1024, 11)
        if "ed_batch" in legs:
            self.b64k = self.batch(65536, 12)
        if "ed_digest" in legs:
            n, sz = 100, 500224
            self.dg = (np.frombuffer(np.random.default_rng(5).bytes(n * sz + 16), dtype=np.uint8),
                       np.arange(n, dtype=np.uint64) * sz, np.full(n, sz, dtype=np.uint64))
        if "bls" in legs or "unloaded" in legs:
            self.bls = Bls(eng)
            rng = np.random.default_rng(3)
            sks = [(int.from_bytes(rng.bytes(32), "big") % (R_BLS - 1) + 1).to_bytes(32, "big") for _ in range(4)]
            self.bpk = self.bls.keygen(sks)
            self.bmsg = hashlib.sha256(b"qos-lat").digest()
            self.bsig = self.bls.sign(sks, [self.bmsg] * 4)
            self.bls.register_keys(self.bpk)
            if "bls" in legs:
                n = 4096
                self.bb = (self.bpk, [self.bsig[i % 4] for i in range(n)], [[i % 4] for i in range(n)],
                           [self.bmsg] * n)

    def batch(self, n, seed):
        np, _lib = self.np, self._lib
        rng = np.random.default_rng(seed)
        seeds = [rng.bytes(32) for _ in range(n)]
        msgs = [rng.bytes(32) for _ in range(n)]
        pk, sg = self.eng.sign_many(seeds, msgs)
        items = [(pk[32 * i:32 * i + 32].tobytes(), sg[64 * i:64 * i + 64].tobytes(), msgs[i]) for i in range(n)]
        return (n,) + tuple(_lib.soa(items))

    def certificate(self):
        res = (ctypes.c_int32 * 1)()
        rc = self.tlib.nwv_certificate_verify_many(self.eng._h, ctypes.byref(self.cc), 1, self.carr, res)
        assert rc == 0 and res[0] == 0

    def verify_batch(self, b, r=0):
        n, pk, sg, arena, offs, lens = b
        p = self._lib._ptr
        allv = self._lib._i32(0)
        self._lib._check(self.lib.nwv_ed25519_verify_batch(self.eng._h, n, p(pk), p(sg), p(arena), p(offs), p(lens),
                                                           bytes([r % 256]) * 32, ctypes.byref(allv), None))
        assert allv.value == 1

    def digests(self):
        arena, offs, lens = self.dg
        p = self._lib._ptr
        out = self.np.zeros(32 * len(offs), dtype=self.np.uint8)
        self._lib._check(self.lib.nwv_blake2b256_many(self.eng._h, len(offs), p(arena), p(offs), p(lens), p(out)))

    def bls_single(self):
        assert self.bls.verify(self.bpk[0], self.bmsg, self.bsig[0]) == 0

    def bls_bulk(self):
        st = self.bls.verify_many(*self.bb)
        assert not any(st)


def timed(call, reps, warm=5, pace=0.0):
    """p50 / p99 of `reps` calls after `warm`; pace: seconds slept between calls (a caller that
    issues its calls at a fixed rest, not back to back, so every state is offered the same load)"""
    lat = []
    for r in range(reps + warm):
        t = time.perf_counter()
        call()
        if r >= warm:
            lat.append(time.perf_counter() - t)
        if pace:
            time.sleep(pace)
    return _pcts(lat)


def loaded(fg, load, n_threads, items_per_call):
    """fg: {name: (call, reps)} timed in turn while n_threads threads loop load() -> results, and the
    load threads' aggregate rate while the foreground ran"""
    stop = threading.Event()
    done = [0] * n_threads
    errs = []

    def work(k):
        try:
            while not stop.is_set():
                load()
                done[k] += 1
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))
            stop.set()

    th = [threading.Thread(target=work, args=(k,)) for k in range(n_threads)]
    for x in th:
        x.start()
    out = {}
    try:
        while sum(done) < n_threads and not stop.is_set():  # every load thread in its stride
            time.sleep(0.001)
        c0, t0 = sum(done), time.perf_counter()
        for name, (call, reps) in fg.items():
            out[name] = timed(call, reps, pace=PACE)
        c1, t1 = sum(done), time.perf_counter()
    finally:
        stop.set()
        for x in th:
            x.join()
    assert not errs, errs
    out["load_calls"] = c1 - c0
    out["load_items_per_s"] = (c1 - c0) * items_per_call / (t1 - t0)
    return out


def worker(a):
    if a.hwq:
        os.environ["GPU_MAX_HW_QUEUES"] = str(min(int(a.hwq), 32))  # before HIP starts
    import narwhal_amd
    legs = a.legs.split(",")
    eng = narwhal_amd.Engine(device=0)
    c = Calls(eng, legs)
    out = {"lib": os.environ.get("NWV_LIB", "libnwv.so"), "on": bool(a.on), "hwq": a.hwq or "default",
           "priority_env": os.environ.get("NWV_LATENCY_PRIORITY", "")}
    if a.on:
        eng.set_latency_max(ED, 1024)
        eng.set_latency_max(BLS, 2)
    reps = a.reps
    if "unloaded" in legs:
        out["unloaded"] = {"certificate": timed(c.certificate, 3 * reps), "batch_1024": timed(lambda: c.verify_batch(c.b1k), reps),
                           "bls_single": timed(c.bls_single, reps)}
    ed_fg = {"certificate": (c.certificate, reps), "batch_1024": (lambda: c.verify_batch(c.b1k), reps)}
    if "ed_batch" in legs:
        out["ed_batch"] = loaded(ed_fg, lambda: c.verify_batch(c.b64k), 4, 65536)
    if "ed_digest" in legs:
        out["ed_digest"] = loaded(ed_fg, c.digests, 4, 100)
    if "bls" in legs:
        out["bls"] = loaded({"bls_single": (c.bls_single, max(reps // 3, 20))}, c.bls_bulk, 2, 4096)
    if a.on:
        out["qos"] = {"ed25519": eng.diag_qos(ED), "bls": eng.diag_qos(BLS),
                      "priority": [list(eng.diag_qos_priority(ED)), list(eng.diag_qos_priority(BLS))]}
    eng.close()
    print(json.dumps(out), flush=True)


def _child(args, env, limit):
    """one worker under its own time limit -> its JSON line; raises on any failure (the driver stops)"""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + args, env=env, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(f"stopped: {' '.join(args)} ended with {p.returncode}\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def ab(a):
    sides = [("parent", a.parent, False, None), ("new_off", "libnwv.so", False, None), ("new_on", "libnwv.so", True, None),
             ("new_on_default_priority", "libnwv.so", True, "0")]
    res = {"what": __doc__.split("\n\n")[0] + "  Fresh worker processes alternating in one session on one MI355X "
           "(tools/qos_lat.py ab): the parent commit's library, this one with the bound off, with it on (Ed25519 "
           "1,024, BLS 2), and with it on over default-priority reserved lanes (NWV_LATENCY_PRIORITY=0).",
           "reps": a.reps, "runs": {}}
    for hwq in ("", "16"):
        key = "hwq_" + (hwq or "default")
        res["runs"][key] = {s[0]: [] for s in sides}
        for r in range(a.runs):
            for name, lib, on, prio in sides:
                env = {k: v for k, v in os.environ.items() if k not in ("NWV_LATENCY_PRIORITY", "NWV_LIB")}
                env["NWV_LIB"] = lib
                if prio is not None:
                    env["NWV_LATENCY_PRIORITY"] = prio
                args = [sys.executable, os.path.abspath(__file__), "worker", "--reps", str(a.reps), "--legs", a.legs]
                args += ["--on"] if on else []
                args += ["--hwq", hwq] if hwq else []
                t = time.time()
                res["runs"][key][name].append(_child(args, env, 300))
                print(f"{key} run {r} {name}: {time.time() - t:.1f} s", flush=True)
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out}), flush=True)


def headline(a):
    import numpy as np
    res = {"what": "plain bench.py (--gpus 1, its default steps and warm-up, the headline alone) with --dump-outputs, the "
           "parent commit's library and this one alternating in one session on one MI355X, value in sigs/s "
           "(tools/qos_lat.py headline).  Staged batches lease no lane and are untouched.",
           "runs": {"parent": [], "new": []}}
    dumps = {}
    for r in range(a.runs):
        for name, lib in (("parent", a.parent), ("new", "libnwv.so")):
            env = dict(os.environ, NWV_LIB=lib)
            d = os.path.join(ROOT, "bench_outputs", f"qos_dump_{name}_{r}")
            line = _child([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", d], env, 400)
            res["runs"][name].append({"value": line["value"]})
            res.setdefault("metric", line.get("metric"))
            dumps[(name, r)] = d
            print(f"run {r} {name}: {line['value']:.4g}", flush=True)
    same = True
    ref = dumps[("parent", 0)]
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
    print(json.dumps({"written": a.out, "identical": same}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    w = sub.add_parser("worker")
    w.add_argument("--on", action="store_true")
    w.add_argument("--hwq", default="")
    w.add_argument("--reps", type=int, default=200)
    w.add_argument("--legs", default="unloaded,ed_batch,ed_digest,bls")
    b = sub.add_parser("ab")
    b.add_argument("--parent", required=True)
    b.add_argument("--runs", type=int, default=3)
    b.add_argument("--reps", type=int, default=200)
    b.add_argument("--legs", default="unloaded,ed_batch,ed_digest,bls")
    b.add_argument("--out", default=os.path.join(ROOT, "profiles", "qos_latency_ab.json"))
    h = sub.add_parser("headline")
    h.add_argument("--parent", required=True)
    h.add_argument("--runs", type=int, default=3)
    h.add_argument("--out", default=os.path.join(ROOT, "profiles", "qos_headline_ab.json"))
    a = ap.parse_args()
    {"worker": worker, "ab": ab, "headline": headline}[a.cmd](a)


if __name__ == "__main__":
    main()
