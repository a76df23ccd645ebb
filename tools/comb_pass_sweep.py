#!/usr/bin/env python3
"""Sweep that derives the value of nwv_set_comb_pass_max.

Keyed batches over a registered 100-key committee with 32-byte messages, 1 % forgeries that decode
(a flipped bit of s; at least one a batch), verdict bits requested: the batch MSM rejects and the
per-signature pass names the bad set.  Host -> host p50 and p99 of nwv_ed25519_verify_batch_keyed
at each size, for
  new4     this build, nwv_set_comb_pass_max at every size, four lanes a signature (k_ed_comb_pass4)
  new16    the same with sixteen lanes a signature (k_ed_comb_pass16, NWV_COMB_PASS_L=16)
  off      this build with the limit at 0: should match the parent
  parent   the parent commit's library, built in the same tree (--parent-lib)
  parent2  the parent again: the difference to `parent` is the measurement's spread
  comb     this build with nwv_set_comb_batch_max above n: k_ed_comb in place of the MSM, as it
           stands (what the new kernel adds over the old one; reported, not gating)
and, for `off`, `parent` and `parent2`, the clean batch of the same size (batch verdict only): the
accepting path, which the limit must leave alone.  Each configuration runs in a child process of its
own, the configurations alternate, --rounds times (at least three).  The parent's run-to-run spread
at a size is (max - min) / min of the p50s of all its runs.  The value is, per form, the largest
swept n such that at n and at every smaller swept n
  new p50 <= parent p50 * (1 - max(0.10, 2 * spread)),
or 0 when no size qualifies.

  python tools/comb_pass_sweep.py --parent-lib narwhal_amd/lib/libnwv_parent.so --out profiles/comb_pass_sweep.json
  python tools/comb_pass_sweep.py --child narwhal_amd/lib/libnwv.so --config new4 --sizes 7000 --reps 50
      (one process, e.g. under a profiler)
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
SIZES = [2049, 4096, 7000, 8192, 16383]
CONFIGS = ("parent", "new4", "off", "parent2", "new16", "comb")
CLEAN = ("off", "parent", "parent2")
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

    check(lib.nwv_init_device(ctypes.byref(h), 0, 0))
    new = args.config in ("new4", "new16")
    if args.config in ("new4", "new16", "off", "comb"):
        lib.nwv_set_comb_pass_max.argtypes = [vp, sz]
        lib.nwv_diag_comb_pass.argtypes = [vp, vp]
        check(lib.nwv_set_comb_pass_max(h, (1 << 30) if new else 0))  # clamped below the shard minimum
    if args.config == "comb":
        lib.nwv_set_comb_batch_max.argtypes = [vp, sz]
        check(lib.nwv_set_comb_batch_max(h, 1 << 30))

    def passes():
        out = np.zeros(2, dtype=np.uint64)
        lib.nwv_diag_comb_pass(h, ptr(out))
        return int(out[0])

    rnd = random.Random(100)
    nk = 100
    seeds = np.frombuffer(rnd.randbytes(32 * nk), dtype=np.uint8)
    zero_off, zero_len = np.zeros(nk, dtype=np.uint64), np.zeros(nk, dtype=np.uint32)
    keys = np.zeros(32 * nk, dtype=np.uint8)
    tmp = np.zeros(64 * nk, dtype=np.uint8)
    check(lib.nwv_ed25519_sign_many(h, nk, ptr(seeds), ptr(np.zeros(16, dtype=np.uint8)), ptr(zero_off), ptr(zero_len),
                                    ptr(keys), ptr(tmp)))
    check(lib.nwv_keycache_register(h, nk, ptr(keys)))
    res = {"config": args.config, "reject": {}, "clean": {}}
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
            return {"p50_ms": 1e3 * ts[len(ts) // 2], "p10_ms": 1e3 * ts[len(ts) // 10],
                    "p99_ms": 1e3 * ts[min(len(ts) - 1, 99 * len(ts) // 100)], "calls": reps}

        if args.config in CLEAN:
            res["clean"][str(n)] = timed(args.reps, False, 1)
        bad = rnd.sample(range(n), max(1, n // 100))
        for i in bad:
            sg[64 * i + 40] ^= 1
        c0 = passes() if new else 0
        r = timed(args.reps, True, 0)
        got = np.unpackbits(bits.view(np.uint8), bitorder="little")[:n]
        assert sorted(np.flatnonzero(got == 0).tolist()) == sorted(bad), "wrong verdict bits"
        if new:
            r["comb_passes"] = passes() - c0
            assert r["comb_passes"] == args.reps + args.warmup, "the comb pass did not run"
        elif args.config in ("off", "comb"):
            assert passes() == 0
        res["reject"][str(n)] = r
    lib.nwv_free(h)
    print("SWEEP " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--config", default="new4", choices=list(CONFIGS))
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=SIZES)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new-lib", default=os.path.join(ROOT, "narwhal_amd", "lib", "libnwv.so"))
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib:
        ap.error("--parent-lib: the parent commit's libnwv.so, built in this tree")
    if args.rounds < 3:
        ap.error("--rounds: at least three runs a side")
    runs = {c: [] for c in CONFIGS}
    for _ in range(args.rounds):
        for cfg in CONFIGS:
            lib = args.parent_lib if cfg.startswith("parent") else args.new_lib
            env = {k: v for k, v in os.environ.items() if k != "NWV_COMB_PASS_L"}
            if cfg in ("new4", "new16"):
                env["NWV_COMB_PASS_L"] = cfg[3:]
            cmd = [sys.executable, os.path.abspath(__file__), "--child", lib, "--config", cfg, "--reps", str(args.reps),
                   "--warmup", str(args.warmup), "--sizes", ",".join(map(str, args.sizes))]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=300, env=env)
            if p.returncode != 0:  # nothing more starts on the device after a failed child
                sys.exit(f"child {cfg} failed with {p.returncode}")
            line = [x for x in p.stdout.splitlines() if x.startswith("SWEEP ")][-1]
            runs[cfg].append(json.loads(line[6:]))
            print(cfg, {n: round(v["p50_ms"], 4) for n, v in runs[cfg][-1]["reject"].items()}, flush=True)

    def stat(cfg, n, key="p50_ms", shape="reject"):
        return [r[shape][str(n)][key] for r in runs[cfg]]

    med = statistics.median
    table, derived, still = [], {"new4": 0, "new16": 0}, {"new4": True, "new16": True}
    for n in args.sizes:
        pa = stat("parent", n) + stat("parent2", n)
        spread = (max(pa) - min(pa)) / min(pa)
        margin = max(0.10, 2 * spread)
        row = {"n": n, "parent_p50_ms": med(pa), "parent_p99_ms": med(stat("parent", n, "p99_ms") + stat("parent2", n, "p99_ms")),
               "parent_p50_runs_ms": pa, "spread": spread, "margin": margin,
               "off_p50_ms": med(stat("off", n)), "off_p50_runs_ms": stat("off", n),
               "k_ed_comb_p50_ms": med(stat("comb", n)), "k_ed_comb_p50_runs_ms": stat("comb", n)}
        for cfg in ("new4", "new16"):
            nw = stat(cfg, n)
            ok = med(nw) <= med(pa) * (1 - margin)
            still[cfg] = still[cfg] and ok
            if still[cfg]:
                derived[cfg] = n
            row.update({cfg + "_p50_ms": med(nw), cfg + "_p99_ms": med(stat(cfg, n, "p99_ms")), cfg + "_p50_runs_ms": nw,
                        cfg + "_qualifies": ok})
        pc = stat("parent", n, shape="clean") + stat("parent2", n, shape="clean")
        oc = stat("off", n, shape="clean")
        row.update({"clean_parent_p50_runs_ms": pc, "clean_off_p50_runs_ms": oc, "clean_parent_p50_ms": med(pc),
                    "clean_off_p50_ms": med(oc), "clean_off_inside_parent_range": min(pc) <= med(oc) <= max(pc)})
        table.append(row)
    out = {"workload": "registered 100-key committee, 32-byte messages, 1 % decodable forgeries, verdict bits requested, "
                       "host->host; clean: the same batch before the forgeries, batch verdict only",
           "reps": args.reps, "warmup": args.warmup, "rounds": args.rounds, "table": table,
           "derived_comb_pass_max": derived, "runs": runs}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps({"table": table, "derived": derived}, indent=1))


if __name__ == "__main__":
    main()
