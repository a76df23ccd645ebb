#!/usr/bin/env python3
"""Sweep behind nwv_bls_set_apk_dense_min and NWV_BLS_APK_LANES.

Items over a registered 100-key committee with 32-byte messages, all valid:
  onekey   one-key items (headers, votes): the dense stage leaves every one to the per-item kernel
  certs    67-of-100 certificates, signers ascending as a bitmap lists them (the signature is by
           the sum of the signers' secret keys, which is what the aggregate of their signatures is)
  mixed    both in turn (kernel statistics only: all three kernels of the stage launch)
host -> host p50 of nwv_bls_verify_many at each size, for
  new      this build with nwv_bls_set_apk_dense_min(1), lanes by the build's rule
  new_lN   `new` with NWV_BLS_APK_LANES=N (certs only)
  off      this build with the setting at its default 0: should match the parent
  parent   the parent commit's library, built in the same tree (--parent-lib)
  parent2  the parent again: the difference to `parent` is the measurement's spread
each with the key-transposed check off and on (nwv_bls_set_key_batch_min(1); --key-batch 0,1).
Each configuration runs in a child process of its own, the configurations alternate, --rounds
times.  The value to give nwv_bls_set_apk_dense_min is, per kind and key-batch setting, the smallest
swept n such that at n and at every larger swept n
  new p50 <= parent p50 * (1 - max(0.10, 2 * spread)),
or none when no size qualifies.

  python tools/bls_apk_dense_sweep.py --parent-lib _prev/libnwv_parent.so --out profiles/bls_apk_dense_sweep.json
  python tools/bls_apk_dense_sweep.py --child narwhal_amd/lib/libnwv.so --config new --kind certs --sizes 16384   (one process, e.g. under a profiler)
  python tools/bls_apk_dense_sweep.py --kernel-stats DIR --what "..." --out FILE   (a profiler's kernel statistics, CSV, as JSON)
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import random
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1100, 2048, 4096, 16384]
KINDS = ["onekey", "certs"]
LANES = [4, 8, 16]
R_ORD = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


def ptr(a):
    return a.ctypes.data


def child(args):
    lib = ctypes.CDLL(os.path.abspath(args.child))
    lib.nwv_init_device.argtypes = [ctypes.POINTER(vp), i32, ctypes.c_uint32]
    lib.nwv_free.argtypes = [vp]
    lib.nwv_bls_keygen_many.argtypes = [vp, sz, vp, vp]
    lib.nwv_bls_sign_many.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, vp]
    lib.nwv_bls_keycache_register.argtypes = [vp, sz, vp]
    lib.nwv_bls_verify_many.argtypes = [vp, sz, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.nwv_bls_last_kernel_ms.argtypes = [vp, vp]
    lib.nwv_bls_last_path.argtypes = [vp]
    lib.nwv_bls_set_key_batch_min.argtypes = [vp, sz]
    lib.nwv_last_error.restype = ctypes.c_char_p
    h = vp()

    def check(rc):
        if rc != 0:
            raise RuntimeError(f"nwv error {rc}: {lib.nwv_last_error().decode(errors='replace')}")

    check(lib.nwv_init_device(ctypes.byref(h), 0, 0))
    dense = args.config.startswith("new")
    if dense:
        lib.nwv_bls_set_apk_dense_min.argtypes = [vp, sz]
        lib.nwv_bls_last_apk_dense.argtypes = [vp, vp]
        check(lib.nwv_bls_set_apk_dense_min(h, 1))
    if args.key_batch_on:
        check(lib.nwv_bls_set_key_batch_min(h, 1))
    rnd = random.Random(300)
    nk, signers = 100, 67
    sk_int = [rnd.randrange(1, R_ORD) for _ in range(nk)]
    sks = np.frombuffer(b"".join(s.to_bytes(32, "big") for s in sk_int), dtype=np.uint8)
    keys = np.zeros(96 * nk, dtype=np.uint8)
    check(lib.nwv_bls_keygen_many(h, nk, ptr(sks), ptr(keys)))
    check(lib.nwv_bls_keycache_register(h, nk, ptr(keys)))
    res = {"config": args.config, "kind": args.kind, "key_batch": int(args.key_batch_on),
           "lanes_env": os.environ.get("NWV_BLS_APK_LANES"), "sizes": {}}
    for n in args.sizes:
        who = []
        for i in range(n):
            if args.kind == "certs" or (args.kind == "mixed" and i % 2):
                who.append(sorted(rnd.sample(range(nk), signers)))
            else:
                who.append([rnd.randrange(nk)])
        kidx = np.array([k for ks in who for k in ks], dtype=np.uint32)
        pk_cnt = np.array([len(ks) for ks in who], dtype=np.uint32)
        pk_off = (np.cumsum(pk_cnt) - pk_cnt).astype(np.uint32)
        sk_n = np.frombuffer(b"".join((sum(sk_int[k] for k in ks) % R_ORD).to_bytes(32, "big") for ks in who),
                             dtype=np.uint8)
        arena = np.frombuffer(rnd.randbytes(32 * n) + bytes(64), dtype=np.uint8).copy()
        offs = (32 * np.arange(n)).astype(np.uint64)
        lens = np.full(n, 32, dtype=np.uint32)
        sg = np.zeros(48 * n + 16, dtype=np.uint8)
        check(lib.nwv_bls_sign_many(h, n, ptr(sk_n), ptr(arena), ptr(offs), ptr(lens), None, 0, ptr(sg)))
        st = np.zeros(n, dtype=np.int32)
        ms = np.zeros(5, dtype=np.float64)

        def call():
            check(lib.nwv_bls_verify_many(h, nk, ptr(keys), n, ptr(sg), ptr(pk_off), ptr(pk_cnt), ptr(kidx), ptr(arena),
                                          ptr(offs), ptr(lens), None, 0, ptr(st)))

        for _ in range(args.warmup):
            call()
            assert (st == 0).all()
        ts, stages = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
            assert (st == 0).all()
            lib.nwv_bls_last_kernel_ms(h, ptr(ms))
            stages.append([float(x) for x in ms])
        ts.sort()
        out = {"p50_ms": 1e3 * ts[len(ts) // 2], "p10_ms": 1e3 * ts[len(ts) // 10], "p90_ms": 1e3 * ts[9 * len(ts) // 10],
               "pairing_stage_p50_ms": statistics.median(s[4] for s in stages),
               "key_sums_stage_p50_ms": statistics.median(s[3] for s in stages), "path": int(lib.nwv_bls_last_path(h)),
               "calls": args.reps}
        if dense:
            b = np.zeros(4, dtype=np.uint64)
            lib.nwv_bls_last_apk_dense(h, ptr(b))
            out["direct_complement_rest_lanes"] = [int(x) for x in b]
        res["sizes"][str(n)] = out
    lib.nwv_free(h)
    print("SWEEP " + json.dumps(res), flush=True)


def kernel_stats(args):
    """a profiler's per-kernel statistics (CSV files with Name, Calls and an average in ns) as JSON:
    average ms per launch of every kernel"""
    kernels = {}
    for path in sorted(glob.glob(os.path.join(args.kernel_stats, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row["Name"].split("(")[0].split(" ")[-1]
                avg = float(row.get("AverageNs") or row.get("Average") or 0.0)
                kernels[name] = {"calls": int(row["Calls"]), "avg_ms": round(avg / 1e6, 4)}
    out = {"what": args.what, "kernels": dict(sorted(kernels.items(), key=lambda kv: -kv[1]["avg_ms"]))}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--config", default="new")
    ap.add_argument("--kind", default="certs", choices=KINDS + ["mixed"])
    ap.add_argument("--key-batch-on", type=int, default=0)
    ap.add_argument("--kinds", type=lambda s: s.split(","), default=KINDS)
    ap.add_argument("--key-batch", type=lambda s: [int(x) for x in s.split(",")], default=[0, 1])
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=SIZES)
    ap.add_argument("--lanes", type=lambda s: [int(x) for x in s.split(",") if x], default=LANES)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--new-lib", default=os.path.join(ROOT, "narwhal_amd", "lib", "libnwv.so"))
    ap.add_argument("--parent-lib")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--what", default="")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.kernel_stats:
        return kernel_stats(args)
    if not args.parent_lib:
        ap.error("--parent-lib: the parent commit's libnwv.so, built in this tree")
    result = {"workload": "100 registered keys, 32-byte messages, all valid, host->host p50; onekey: one-key items, "
                          "certs: 67-of-100 certificates with ascending signer lists",
              "reps": args.reps, "warmup": args.warmup, "rounds": args.rounds, "results": {}}
    for kind in args.kinds:
        for kb in args.key_batch:
            # (library, NWV_BLS_APK_LANES or None: the build's rule)
            cfgs = {"parent": (args.parent_lib, None), "new": (args.new_lib, None),
                    "parent2": (args.parent_lib, None), "off": (args.new_lib, None)}
            if kind == "certs":
                for l in args.lanes:
                    cfgs[f"new_l{l}"] = (args.new_lib, l)
            runs = {c: [] for c in cfgs}
            for _ in range(args.rounds):
                for cfg, (lib, lanes) in cfgs.items():
                    cmd = [sys.executable, os.path.abspath(__file__), "--child", lib, "--config", cfg, "--kind", kind,
                           "--key-batch-on", str(kb), "--reps", str(args.reps), "--warmup", str(args.warmup),
                           "--sizes", ",".join(map(str, args.sizes))]
                    env = dict(os.environ)
                    env.pop("NWV_BLS_APK_LANES", None)
                    if lanes is not None:
                        env["NWV_BLS_APK_LANES"] = str(lanes)
                    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600, env=env)
                    if p.returncode != 0:  # nothing more starts on the device after a failed child
                        sys.exit(f"child {kind} kb={kb} {cfg} failed with {p.returncode}")
                    line = [x for x in p.stdout.splitlines() if x.startswith("SWEEP ")][-1]
                    runs[cfg].append(json.loads(line[6:]))
                    print(kind, f"kb={kb}", cfg, {n: round(v["p50_ms"], 3) for n, v in runs[cfg][-1]["sizes"].items()},
                          flush=True)

            def p50(cfg, n, field="p50_ms"):
                return statistics.mean(r["sizes"][str(n)][field] for r in runs[cfg])

            table, qual = [], {}
            news = [c for c in cfgs if c.startswith("new")]
            for n in args.sizes:
                pa, pb, off = p50("parent", n), p50("parent2", n), p50("off", n)
                spread = abs(pa - pb) / min(pa, pb)
                margin = max(0.10, 2 * spread)
                nw = p50("new", n)
                qual[n] = nw <= pa * (1 - margin)
                lo, hi = min(pa, pb), max(pa, pb)
                row = {"n": n, "parent_p50_ms": pa, "parent2_p50_ms": pb, "off_p50_ms": off,
                       "off_inside_parent_spread": lo * (1 - spread) <= off <= hi * (1 + spread),
                       "off_minus_parent_ms": off - (pa + pb) / 2,
                       "parent_key_sums_stage_ms": p50("parent", n, "key_sums_stage_p50_ms"),
                       "spread": spread, "margin": margin, "qualifies": qual[n]}
                for c in news:
                    row[c + "_p50_ms"] = p50(c, n)
                    row[c + "_key_sums_stage_ms"] = p50(c, n, "key_sums_stage_p50_ms")
                    row[c + "_counts"] = runs[c][-1]["sizes"][str(n)].get("direct_complement_rest_lanes")
                table.append(row)
            recommended = None
            for n in sorted(args.sizes, reverse=True):
                if not qual[n]:
                    break
                recommended = n
            key = f"{kind}_key_batch_{kb}"
            result["results"][key] = {"table": table,
                                      "recommended_apk_dense_min": recommended if recommended is not None else "none",
                                      "runs": runs}
            print(json.dumps({"key": key, "table": table,
                              "recommended_apk_dense_min": result["results"][key]["recommended_apk_dense_min"]}, indent=1),
                  flush=True)
            if args.out:  # (after every kind: a later child's failure keeps what was measured)
                with open(args.out, "w") as f:
                    json.dump(result, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()
