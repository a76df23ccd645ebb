#!/usr/bin/env python3
"""Sweep that sets the default of nwv_set_each_row_max.

Unregistered random keys (16 of them), 32-byte messages, host -> host p50 and p99 at each size of
  each     nwv_ed25519_verify_each on valid input
  reject   nwv_ed25519_verify_batch with the verdict bits requested and 1 % forgeries that decode
           (a flipped bit of s; at least one a batch): the MSM rejects, the per-signature pass names them
for
  new      this build, the row kernel (k_ed_each_row) offered at every size
  parent   the parent commit's library, built in the same tree (--parent-lib): the lane pipeline
  plain    this build opened with NWV_FLAG_NO_MSM_REUSE: the pass after a rejected MSM runs the plain
           form of the kernel (k_ed_each_row) instead of the reuse form (k_ed_each_row_msm); the A/B
           of the two forms is `new` against `plain` on the reject shape (reported, not gating)
Each run is a child process of its own, the two alternate, --rounds times (at least three).  The
parent's run-to-run spread at a size is (max - min) / min of its runs' p50s.  The default is, for
each call shape, the largest swept n such that at n and at every smaller swept n
  new p50 <= parent p50 * (1 - max(0.10, 2 * spread)),
and the smaller of the two shapes' values (0 when no size qualifies).

  python tools/each_row_sweep.py --parent-lib narwhal_amd/lib/libnwv_parent.so --out profiles/each_row_sweep.json
  python tools/each_row_sweep.py --child narwhal_amd/lib/libnwv.so --config new --sizes 64,1024,4096 --reps 20
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
SIZES = [1, 4, 16, 64, 128, 256, 512, 1024, 2048, 4096]
SHAPES = ("each", "reject")
NWV_FLAG_NO_MSM_REUSE = 32
vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


def ptr(a):
    return a.ctypes.data


def child(args):
    lib = ctypes.CDLL(os.path.abspath(args.child))
    lib.nwv_init_device.argtypes = [ctypes.POINTER(vp), i32, ctypes.c_uint32]
    lib.nwv_free.argtypes = [vp]
    lib.nwv_ed25519_sign_many.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    lib.nwv_ed25519_verify_each.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    lib.nwv_ed25519_verify_batch.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.nwv_last_error.restype = ctypes.c_char_p
    h = vp()

    def check(rc):
        if rc != 0:
            raise RuntimeError(f"nwv error {rc}: {lib.nwv_last_error().decode(errors='replace')}")

    check(lib.nwv_init_device(ctypes.byref(h), 0, NWV_FLAG_NO_MSM_REUSE if args.config == "plain" else 0))
    new = args.config in ("new", "plain")
    if new:
        lib.nwv_set_each_row_max.argtypes = [vp, sz]
        lib.nwv_diag_each_row.argtypes = [vp, vp]
        check(lib.nwv_set_each_row_max(h, 1 << 30))  # clamped below the shard minimum: every swept size

    def row_passes():
        out = np.zeros(2, dtype=np.uint64)
        lib.nwv_diag_each_row(h, ptr(out))
        return int(out[0])

    rnd = random.Random(100)
    nk = 16
    seeds = np.frombuffer(rnd.randbytes(32 * nk), dtype=np.uint8)
    res = {"config": args.config, "each": {}, "reject": {}}
    for n in args.sizes:
        arena = np.frombuffer(rnd.randbytes(32 * n) + bytes(64), dtype=np.uint8).copy()
        offs = (32 * np.arange(n)).astype(np.uint64)
        lens = np.full(n, 32, dtype=np.uint32)
        kidx = np.array([rnd.randrange(nk) for _ in range(n)], dtype=np.uint32)
        sd = np.ascontiguousarray(seeds.reshape(nk, 32)[kidx]).reshape(-1)
        pk = np.zeros(32 * n + 16, dtype=np.uint8)
        sg = np.zeros(64 * n + 16, dtype=np.uint8)
        check(lib.nwv_ed25519_sign_many(h, n, ptr(sd), ptr(arena), ptr(offs), ptr(lens), ptr(pk), ptr(sg)))
        allv = i32(0)
        bits = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)

        def call_each():
            check(lib.nwv_ed25519_verify_each(h, n, ptr(pk), ptr(sg), ptr(arena), ptr(offs), ptr(lens), ptr(bits)))

        def call_batch():
            check(lib.nwv_ed25519_verify_batch(h, n, ptr(pk), ptr(sg), ptr(arena), ptr(offs), ptr(lens), None,
                                               ctypes.byref(allv), ptr(bits)))

        def timed(fn, reps, bad):
            for _ in range(args.warmup):
                fn()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            got = np.unpackbits(bits.view(np.uint8), bitorder="little")[:n]
            assert sorted(np.flatnonzero(got == 0).tolist()) == sorted(bad), "wrong verdict bits"
            ts.sort()
            return {"p50_ms": 1e3 * ts[len(ts) // 2], "p99_ms": 1e3 * ts[min(len(ts) - 1, 99 * len(ts) // 100)],
                    "p10_ms": 1e3 * ts[len(ts) // 10], "calls": reps}

        for shape in SHAPES:
            bad = []
            if shape == "reject":
                bad = rnd.sample(range(n), max(1, n // 100))
                for i in bad:
                    sg[64 * i + 40] ^= 1
            c0 = row_passes() if new else 0
            r = timed(call_each if shape == "each" else call_batch, args.reps, bad)
            if new:
                r["row_passes"] = row_passes() - c0
                assert r["row_passes"] == args.reps + args.warmup, "the row kernel did not run"
            res[shape][str(n)] = r
    lib.nwv_free(h)
    print("SWEEP " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--config", default="new", choices=["new", "parent", "plain"])
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=SIZES)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
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
    libs = {"parent": args.parent_lib, "new": args.new_lib, "plain": args.new_lib}
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
            for shape in SHAPES:
                print(cfg, shape, {n: round(v["p50_ms"], 4) for n, v in runs[cfg][-1][shape].items()}, flush=True)

    def stat(cfg, shape, n, key="p50_ms"):
        return [r[shape][str(n)][key] for r in runs[cfg]]

    tables, defaults = {}, {}
    for shape in SHAPES:
        table, default, still = [], 0, True
        for n in args.sizes:
            pa, nw = stat("parent", shape, n), stat("new", shape, n)
            spread = (max(pa) - min(pa)) / min(pa)
            margin = max(0.10, 2 * spread)
            ok = statistics.median(nw) <= statistics.median(pa) * (1 - margin)
            still = still and ok
            if still:
                default = n
            table.append({"n": n, "new_p50_ms": statistics.median(nw), "parent_p50_ms": statistics.median(pa),
                          "new_p99_ms": statistics.median(stat("new", shape, n, "p99_ms")),
                          "parent_p99_ms": statistics.median(stat("parent", shape, n, "p99_ms")),
                          "plain_form_p50_ms": statistics.median(stat("plain", shape, n)),
                          "parent_p50_runs_ms": pa, "new_p50_runs_ms": nw,
                          "plain_form_p50_runs_ms": stat("plain", shape, n), "spread": spread, "margin": margin,
                          "qualifies": ok})
        tables[shape], defaults[shape] = table, default
    out = {"workload": "16 unregistered keys, 32-byte messages, host->host; each: verify_each on valid input; "
                       "reject: verify_batch, verdict bits requested, 1 % decodable forgeries",
           "reps": args.reps, "warmup": args.warmup, "rounds": args.rounds, "tables": tables,
           "derived_default_by_shape": defaults, "derived_default_each_row_max": min(defaults.values()), "runs": runs}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps({"tables": tables, "defaults": defaults, "default": out["derived_default_each_row_max"]}, indent=1))


if __name__ == "__main__":
    main()
