#!/usr/bin/env python3
"""Sweep that sets the default of nwv_set_comb_batch_max.

Keyed batches over a registered 100-key committee with 32-byte messages, host -> host p50 of
nwv_ed25519_verify_batch_keyed (batch verdict only, valid batches) at each size, for
  new      this build, comb path offered at every size
  parent   the parent commit's library, built in the same tree (--parent-lib; batch MSM above 64)
  parent2  the parent again: the difference to `parent` is the measurement's spread
  notiny   this build opened with NWV_FLAG_NO_TINY (batch MSM): should match the parent
Each configuration runs in a child process of its own, the configurations alternate, --rounds times.
The default is the largest swept n such that at n and at every smaller swept n
  new p50 <= parent p50 * (1 - max(0.10, 2 * spread)),
or 0 when no size qualifies.  Second metric (reported, not gating): a rejected batch with 1 % forgeries
and the verdict bits requested, at 1,024 and 7,000 signatures.

  python tools/comb_sweep.py --parent-lib narwhal_amd/lib/libnwv_parent.so --out profiles/comb_batch_sweep.json
  python tools/comb_sweep.py --child narwhal_amd/lib/libnwv.so --config new --sizes 1024,7000   (one process, e.g. under a profiler)
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [65, 128, 256, 512, 1024, 2048, 4096, 7000, 8192, 16383]
REJECT_SIZES = [1024, 7000]
NWV_FLAG_NO_TINY = 4096
vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


def ptr(a):
    return a.ctypes.data


def child(args):
    lib = ctypes.CDLL(os.path.abspath(args.child))
    lib.nwv_init_device.argtypes = [ctypes.POINTER(vp), i32, ctypes.c_uint32]
    lib.nwv_free.argtypes = [vp]
    lib.nwv_keycache_register.argtypes = [vp, sz, vp]
    lib.nwv_ed25519_sign_many.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    lib.nwv_ed25519_verify_batch_keyed.argtypes = [vp, sz, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.nwv_last_error.restype = ctypes.c_char_p
    h = vp()

    def check(rc):
        if rc != 0:
            raise RuntimeError(f"nwv error {rc}: {lib.nwv_last_error().decode(errors='replace')}")

    check(lib.nwv_init_device(ctypes.byref(h), 0, NWV_FLAG_NO_TINY if args.config == "notiny" else 0))
    comb = args.config == "new"
    if comb:
        lib.nwv_set_comb_batch_max.argtypes = [vp, sz]
        lib.nwv_diag_counters_ex.argtypes = [vp, vp, i32]
        check(lib.nwv_set_comb_batch_max(h, 1 << 30))  # clamped below the shard minimum: every swept size

    def comb_count():
        out = np.zeros(4, dtype=np.uint64)
        lib.nwv_diag_counters_ex(h, ptr(out), 4)
        return int(out[3])

    rnd = random.Random(100)
    nk = 100
    seeds = np.frombuffer(rnd.randbytes(32 * nk), dtype=np.uint8)
    zero_off, zero_len = np.zeros(nk, dtype=np.uint64), np.zeros(nk, dtype=np.uint32)
    keys = np.zeros(32 * nk, dtype=np.uint8)
    tmp = np.zeros(64 * nk, dtype=np.uint8)
    check(lib.nwv_ed25519_sign_many(h, nk, ptr(seeds), ptr(np.zeros(16, dtype=np.uint8)), ptr(zero_off), ptr(zero_len),
                                    ptr(keys), ptr(tmp)))
    check(lib.nwv_keycache_register(h, nk, ptr(keys)))
    res = {"config": args.config, "sizes": {}, "rejected": {}}
    for n in args.sizes:
        kidx = np.array([rnd.randrange(nk) for _ in range(n)], dtype=np.uint32)
        arena = np.frombuffer(rnd.randbytes(32 * n) + bytes(64), dtype=np.uint8).copy()
        offs = (32 * np.arange(n)).astype(np.uint64)
        lens = np.full(n, 32, dtype=np.uint32)
        sd = np.ascontiguousarray(seeds.reshape(nk, 32)[kidx]).reshape(-1)
        pk = np.zeros(32 * n, dtype=np.uint8)
        sg = np.zeros(64 * n + 16, dtype=np.uint8)
        check(lib.nwv_ed25519_sign_many(h, n, ptr(sd), ptr(arena), ptr(offs), ptr(lens), ptr(pk), ptr(sg)))
        allv = i32(0)
        bits = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)

        def call(want_bits):
            check(lib.nwv_ed25519_verify_batch_keyed(h, nk, ptr(keys), n, ptr(kidx), ptr(sg), ptr(arena), ptr(offs),
                                                     ptr(lens), None, ctypes.byref(allv), ptr(bits) if want_bits else None))
            return allv.value

        def timed(reps, want_bits, expect):
            for _ in range(args.warmup):
                assert call(want_bits) == expect
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                v = call(want_bits)
                ts.append(time.perf_counter() - t0)
                assert v == expect
            ts.sort()
            return {"p50_ms": 1e3 * ts[len(ts) // 2], "p10_ms": 1e3 * ts[len(ts) // 10], "p90_ms": 1e3 * ts[9 * len(ts) // 10],
                    "calls": reps}

        c0 = comb_count() if comb else 0
        r = timed(args.reps, False, 1)
        if comb:
            r["comb_launches"] = comb_count() - c0
            assert r["comb_launches"] == args.reps + args.warmup, "the comb path did not run"
        res["sizes"][str(n)] = r
        if n in REJECT_SIZES and not args.no_reject:
            bad = rnd.sample(range(n), n // 100)
            for i in bad:
                sg[64 * i + 40] ^= 1
            r = timed(max(50, args.reps // 3), True, 0)
            got = np.unpackbits(bits.view(np.uint8), bitorder="little")[:n]
            assert sorted(np.flatnonzero(got == 0).tolist()) == sorted(bad)
            res["rejected"][str(n)] = r
    lib.nwv_free(h)
    print("SWEEP " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--config", default="new", choices=["new", "parent", "parent2", "notiny"])
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=SIZES)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-reject", action="store_true")
    ap.add_argument("--new-lib", default=os.path.join(ROOT, "narwhal_amd", "lib", "libnwv.so"))
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib:
        ap.error("--parent-lib: the parent commit's libnwv.so, built in this tree")
    libs = {"parent": args.parent_lib, "new": args.new_lib, "parent2": args.parent_lib, "notiny": args.new_lib}
    runs = {c: [] for c in libs}
    for _ in range(args.rounds):
        for cfg, lib in libs.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--child", lib, "--config", cfg, "--reps", str(args.reps),
                   "--warmup", str(args.warmup), "--sizes", ",".join(map(str, args.sizes))]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:  # nothing more starts on the device after a failed child
                sys.exit(f"child {cfg} failed with {p.returncode}")
            line = [x for x in p.stdout.splitlines() if x.startswith("SWEEP ")][-1]
            runs[cfg].append(json.loads(line[6:]))
            print(cfg, {n: round(v["p50_ms"], 4) for n, v in runs[cfg][-1]["sizes"].items()}, flush=True)

    def p50(cfg, n, kind="sizes"):
        return statistics.mean(r[kind][str(n)]["p50_ms"] for r in runs[cfg])

    table, default, still = [], 0, True
    for n in args.sizes:
        pa, pb, nw, nt = p50("parent", n), p50("parent2", n), p50("new", n), p50("notiny", n)
        spread = abs(pa - pb) / min(pa, pb)
        margin = max(0.10, 2 * spread)
        ok = nw <= pa * (1 - margin)
        still = still and ok
        if still:
            default = n
        table.append({"n": n, "new_p50_ms": nw, "parent_p50_ms": pa, "parent2_p50_ms": pb, "notiny_p50_ms": nt,
                      "spread": spread, "margin": margin, "qualifies": ok})
    rej = [{"n": n, "new_p50_ms": p50("new", n, "rejected"), "parent_p50_ms": p50("parent", n, "rejected"),
            "notiny_p50_ms": p50("notiny", n, "rejected")} for n in REJECT_SIZES if n in args.sizes and not args.no_reject]
    out = {"workload": "keyed batch, 100 registered keys, 32-byte messages, batch verdict only, host->host p50",
           "reps": args.reps, "warmup": args.warmup, "rounds": args.rounds, "table": table,
           "rejected_1pct_bits_requested": rej, "derived_default_comb_batch_max": default, "runs": runs}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps({"table": table, "rejected": rej, "default": default}, indent=1))


if __name__ == "__main__":
    main()
