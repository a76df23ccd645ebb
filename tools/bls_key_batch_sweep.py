#!/usr/bin/env python3
"""Sweep behind nwv_bls_set_key_batch_min and the default of NWV_BLS_KEY_GROUP.

Two kinds of item over a registered 100-key committee with 32-byte messages, all valid:
  onekey   one-key items (headers, votes)
  certs    67-of-100 certificates (the signature is by the sum of the signers' secret keys, which
           is what the aggregate of their signatures is)
host -> host p50 of nwv_bls_verify_many at each size, for
  new      this build with nwv_bls_set_key_batch_min(1): the key-transposed batch check
  off      this build with the setting at its default 0: should match the parent
  parent   the parent commit's library, built in the same tree (--parent-lib)
  parent2  the parent again: the difference to `parent` is the measurement's spread
  new_gN   `new` with NWV_BLS_KEY_GROUP=N, at the largest size only (--groups)
Each configuration runs in a child process of its own, the configurations alternate, --rounds
times.  The value to give nwv_bls_set_key_batch_min is, per kind, the smallest swept n such that
at n and at every larger swept n
  new p50 <= parent p50 * (1 - max(0.10, 2 * spread)),
or none when no size qualifies.  Second metric (reported, not gating): 1 % of the items signed
over another message, at 4,096 and 16,384 items.

  python tools/bls_key_batch_sweep.py --parent-lib narwhal_amd/lib/libnwv_parent.so --out profiles/bls_key_batch_sweep.json
  python tools/bls_key_batch_sweep.py --child narwhal_amd/lib/libnwv.so --config new --kind certs --sizes 16384   (one process, e.g. under a profiler)
  python tools/bls_key_batch_sweep.py --kernel-stats DIR --out profiles/bls_key_batch_kernel_ms.json   (a profiler's kernel statistics, CSV, into the committed form)
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
FORGED_SIZES = [4096, 16384]
GROUPS = [512, 2048, 8192]
KINDS = ["onekey", "certs"]
VERIFY_FAIL = 5
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
    lib.nwv_last_error.restype = ctypes.c_char_p
    h = vp()

    def check(rc):
        if rc != 0:
            raise RuntimeError(f"nwv error {rc}: {lib.nwv_last_error().decode(errors='replace')}")

    check(lib.nwv_init_device(ctypes.byref(h), 0, 0))
    batch = args.config.startswith("new")
    if batch:
        lib.nwv_bls_set_key_batch_min.argtypes = [vp, sz]
        lib.nwv_bls_last_key_batch.argtypes = [vp, vp]
        check(lib.nwv_bls_set_key_batch_min(h, 1))
    rnd = random.Random(300)
    nk, signers = 100, 67
    sk_int = [rnd.randrange(1, R_ORD) for _ in range(nk)]
    sks = np.frombuffer(b"".join(s.to_bytes(32, "big") for s in sk_int), dtype=np.uint8)
    keys = np.zeros(96 * nk, dtype=np.uint8)
    check(lib.nwv_bls_keygen_many(h, nk, ptr(sks), ptr(keys)))
    check(lib.nwv_bls_keycache_register(h, nk, ptr(keys)))
    res = {"config": args.config, "kind": args.kind, "group": os.environ.get("NWV_BLS_KEY_GROUP"), "sizes": {},
           "forged": {}}
    for n in args.sizes:
        if args.kind == "certs":
            who = [rnd.sample(range(nk), signers) for _ in range(n)]
        else:
            who = [[rnd.randrange(nk)] for _ in range(n)]
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

        def timed(reps, want, path):
            for _ in range(args.warmup):
                call()
                assert (st == want).all()
            ts, stages = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                call()
                ts.append(time.perf_counter() - t0)
                assert (st == want).all()
                lib.nwv_bls_last_kernel_ms(h, ptr(ms))
                stages.append([float(x) for x in ms])
            assert lib.nwv_bls_last_path(h) == path, (lib.nwv_bls_last_path(h), path)
            ts.sort()
            out = {"p50_ms": 1e3 * ts[len(ts) // 2], "p10_ms": 1e3 * ts[len(ts) // 10], "p90_ms": 1e3 * ts[9 * len(ts) // 10],
                   "pairing_stage_p50_ms": statistics.median(s[4] for s in stages),
                   "key_sums_stage_p50_ms": statistics.median(s[3] for s in stages), "calls": reps}
            if batch:
                b = np.zeros(5, dtype=np.uint64)
                lib.nwv_bls_last_key_batch(h, ptr(b))
                out["groups_rejected_rechecked_millers_items"] = [int(x) for x in b]
            return out

        res["sizes"][str(n)] = timed(args.reps, np.zeros(n, dtype=np.int32), 6 if batch else 3)
        if n in FORGED_SIZES and not args.no_forged:
            bad = rnd.sample(range(n), n // 100)
            want = np.zeros(n, dtype=np.int32)
            for i in bad:
                arena[32 * i] ^= 1
                want[i] = VERIFY_FAIL
            res["forged"][str(n)] = timed(max(5, args.reps // 2), want, 7 if batch else 3)
    lib.nwv_free(h)
    print("SWEEP " + json.dumps(res), flush=True)


def kernel_stats(args):
    """a profiler's per-kernel statistics (CSV files with Name, Calls and an average in ns) as the
    committed JSON: average ms per launch of every BLS kernel"""
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
    ap.add_argument("--kind", default="onekey", choices=KINDS)
    ap.add_argument("--kinds", type=lambda s: s.split(","), default=KINDS)
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=SIZES)
    ap.add_argument("--groups", type=lambda s: [int(x) for x in s.split(",")], default=GROUPS)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-forged", action="store_true")
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
    top = max(args.sizes)
    # (library, sizes, NWV_BLS_KEY_GROUP or None: the build's default)
    cfgs = {"parent": (args.parent_lib, args.sizes, None), "new": (args.new_lib, args.sizes, None),
            "parent2": (args.parent_lib, args.sizes, None), "off": (args.new_lib, args.sizes, None)}
    for g in args.groups:
        cfgs[f"new_g{g}"] = (args.new_lib, [top], g)
    result = {"workload": "100 registered keys, 32-byte messages, all valid, host->host p50; onekey: one-key items, "
                          "certs: 67-of-100 certificates", "reps": args.reps, "warmup": args.warmup,
              "rounds": args.rounds, "kinds": {}}
    for kind in args.kinds:
        runs = {c: [] for c in cfgs}
        for _ in range(args.rounds):
            for cfg, (lib, sizes, grp) in cfgs.items():
                cmd = [sys.executable, os.path.abspath(__file__), "--child", lib, "--config", cfg, "--kind", kind,
                       "--reps", str(args.reps), "--warmup", str(args.warmup), "--sizes", ",".join(map(str, sizes))]
                if grp is not None or args.no_forged:
                    cmd.append("--no-forged")
                env = dict(os.environ)
                env.pop("NWV_BLS_KEY_GROUP", None)
                if grp is not None:
                    env["NWV_BLS_KEY_GROUP"] = str(grp)
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600, env=env)
                if p.returncode != 0:  # nothing more starts on the device after a failed child
                    sys.exit(f"child {kind} {cfg} failed with {p.returncode}")
                line = [x for x in p.stdout.splitlines() if x.startswith("SWEEP ")][-1]
                runs[cfg].append(json.loads(line[6:]))
                print(kind, cfg, {n: round(v["p50_ms"], 3) for n, v in runs[cfg][-1]["sizes"].items()}, flush=True)

        def p50(cfg, n, part="sizes", field="p50_ms"):
            return statistics.mean(r[part][str(n)][field] for r in runs[cfg])

        table, qual = [], {}
        for n in args.sizes:
            pa, pb, nw, off = p50("parent", n), p50("parent2", n), p50("new", n), p50("off", n)
            spread = abs(pa - pb) / min(pa, pb)
            margin = max(0.10, 2 * spread)
            qual[n] = nw <= pa * (1 - margin)
            lo, hi = min(pa, pb), max(pa, pb)
            table.append({"n": n, "new_p50_ms": nw, "parent_p50_ms": pa, "parent2_p50_ms": pb, "off_p50_ms": off,
                          "off_inside_parent_spread": lo * (1 - spread) <= off <= hi * (1 + spread),
                          "new_pairing_stage_ms": p50("new", n, field="pairing_stage_p50_ms"),
                          "parent_pairing_stage_ms": p50("parent", n, field="pairing_stage_p50_ms"),
                          "new_key_sums_stage_ms": p50("new", n, field="key_sums_stage_p50_ms"),
                          "parent_key_sums_stage_ms": p50("parent", n, field="key_sums_stage_p50_ms"),
                          "new_counts": runs["new"][-1]["sizes"][str(n)].get("groups_rejected_rechecked_millers_items"),
                          "spread": spread, "margin": margin, "qualifies": qual[n]})
        recommended = None
        for n in sorted(args.sizes, reverse=True):
            if not qual[n]:
                break
            recommended = n
        top_spread = next(t["spread"] for t in table if t["n"] == top)
        groups = [{"group": g, "p50_ms": p50(f"new_g{g}", top),
                   "pairing_stage_ms": p50(f"new_g{g}", top, field="pairing_stage_p50_ms")} for g in args.groups]
        best = min(g["p50_ms"] for g in groups) if groups else None
        chosen = next((g["group"] for g in sorted(groups, key=lambda g: g["group"])
                       if g["p50_ms"] <= best * (1 + top_spread)), None)
        forged = [{"n": n, "new_p50_ms": p50("new", n, "forged"), "parent_p50_ms": p50("parent", n, "forged"),
                   "new_counts": runs["new"][-1]["forged"][str(n)].get("groups_rejected_rechecked_millers_items")}
                  for n in FORGED_SIZES if n in args.sizes and not args.no_forged]
        result["kinds"][kind] = {"table": table, "group_sizes_at_largest_n": groups, "group_within_spread_of_best": chosen,
                                 "forged_1pct": forged,
                                 "recommended_key_batch_min": recommended if recommended is not None else "none",
                                 "runs": runs}
        print(json.dumps({"kind": kind, "table": table, "groups": groups, "forged": forged,
                          "recommended_key_batch_min": result["kinds"][kind]["recommended_key_batch_min"]}, indent=1),
              flush=True)
        if args.out:  # (after every kind: a later child's failure keeps what was measured)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
