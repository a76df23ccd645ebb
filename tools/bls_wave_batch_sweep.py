#!/usr/bin/env python3
"""Sweep behind nwv_bls_set_wave_batch_min and the default of NWV_BLS_BATCH_GROUP.

One-key items over a registered 100-key committee with 32-byte messages, all valid, host -> host
p50 of nwv_bls_verify_many at each size, for
  new      this build with nwv_bls_set_wave_batch_min(1): the wave batch check
  off      this build with the setting at its default 0: should match the parent
  parent   the parent commit's library, built in the same tree (--parent-lib)
  parent2  the parent again: the difference to `parent` is the measurement's spread
  new_gN   `new` with NWV_BLS_BATCH_GROUP=N, at the largest size only (--groups)
Each configuration runs in a child process of its own, the configurations alternate, --rounds
times.  The value to give nwv_bls_set_wave_batch_min is the smallest swept n such that at n and at
every larger swept n
  new p50 <= parent p50 * (1 - max(0.10, 2 * spread)),
or none when no size qualifies.  The group size is the smallest swept one whose p50 at the largest
size is within the measured spread of the best.  Second metric (reported, not gating): 1 % of the
items signed over another message, at 4,096 and 16,384 items.

  python tools/bls_wave_batch_sweep.py --parent-lib narwhal_amd/lib/libnwv_parent.so --out profiles/bls_wave_batch_sweep.json
  python tools/bls_wave_batch_sweep.py --child narwhal_amd/lib/libnwv.so --config new --sizes 16384   (one process, e.g. under a profiler)
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
SIZES = [1100, 2048, 4096, 16384]
FORGED_SIZES = [4096, 16384]
GROUPS = [16, 64, 256]
VERIFY_FAIL = 5
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
        lib.nwv_bls_set_wave_batch_min.argtypes = [vp, sz]
        lib.nwv_bls_last_batch.argtypes = [vp, vp]
        check(lib.nwv_bls_set_wave_batch_min(h, 1))
    r_ord = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
    rnd = random.Random(200)
    nk = 100
    sks = np.frombuffer(b"".join(rnd.randrange(1, r_ord).to_bytes(32, "big") for _ in range(nk)), dtype=np.uint8)
    keys = np.zeros(96 * nk, dtype=np.uint8)
    check(lib.nwv_bls_keygen_many(h, nk, ptr(sks), ptr(keys)))
    check(lib.nwv_bls_keycache_register(h, nk, ptr(keys)))
    res = {"config": args.config, "group": os.environ.get("NWV_BLS_BATCH_GROUP"), "sizes": {}, "forged": {}}
    for n in args.sizes:
        kidx = np.array([rnd.randrange(nk) for _ in range(n)], dtype=np.uint32)
        arena = np.frombuffer(rnd.randbytes(32 * n) + bytes(64), dtype=np.uint8).copy()
        offs = (32 * np.arange(n)).astype(np.uint64)
        lens = np.full(n, 32, dtype=np.uint32)
        sk_n = np.ascontiguousarray(sks.reshape(nk, 32)[kidx]).reshape(-1)
        sg = np.zeros(48 * n + 16, dtype=np.uint8)
        check(lib.nwv_bls_sign_many(h, n, ptr(sk_n), ptr(arena), ptr(offs), ptr(lens), None, 0, ptr(sg)))
        pk_off = np.arange(n, dtype=np.uint32)
        pk_cnt = np.ones(n, dtype=np.uint32)
        st = np.zeros(n, dtype=np.int32)
        ms = np.zeros(5, dtype=np.float64)

        def call():
            check(lib.nwv_bls_verify_many(h, nk, ptr(keys), n, ptr(sg), ptr(pk_off), ptr(pk_cnt), ptr(kidx), ptr(arena),
                                          ptr(offs), ptr(lens), None, 0, ptr(st)))

        def timed(reps, want, path):
            for _ in range(args.warmup):
                call()
                assert (st == want).all()
            ts, pair = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                call()
                ts.append(time.perf_counter() - t0)
                assert (st == want).all()
                lib.nwv_bls_last_kernel_ms(h, ptr(ms))
                pair.append(float(ms[4]))
            assert lib.nwv_bls_last_path(h) == path, (lib.nwv_bls_last_path(h), path)
            ts.sort()
            out = {"p50_ms": 1e3 * ts[len(ts) // 2], "p10_ms": 1e3 * ts[len(ts) // 10], "p90_ms": 1e3 * ts[9 * len(ts) // 10],
                   "pairing_stage_p50_ms": statistics.median(pair), "calls": reps}
            if batch:
                b = np.zeros(3, dtype=np.uint64)
                lib.nwv_bls_last_batch(h, ptr(b))
                out["groups_rejected_rechecked"] = [int(x) for x in b]
            return out

        res["sizes"][str(n)] = timed(args.reps, np.zeros(n, dtype=np.int32), 4 if batch else 3)
        if n in FORGED_SIZES and not args.no_forged:
            bad = rnd.sample(range(n), n // 100)
            want = np.zeros(n, dtype=np.int32)
            for i in bad:
                arena[32 * i] ^= 1
                want[i] = VERIFY_FAIL
            res["forged"][str(n)] = timed(max(5, args.reps // 2), want, 5 if batch else 3)
    lib.nwv_free(h)
    print("SWEEP " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--config", default="new")
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=SIZES)
    ap.add_argument("--groups", type=lambda s: [int(x) for x in s.split(",")], default=GROUPS)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-forged", action="store_true")
    ap.add_argument("--new-lib", default=os.path.join(ROOT, "narwhal_amd", "lib", "libnwv.so"))
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib:
        ap.error("--parent-lib: the parent commit's libnwv.so, built in this tree")
    top = max(args.sizes)
    # (library, sizes, NWV_BLS_BATCH_GROUP or None: the build's default)
    cfgs = {"parent": (args.parent_lib, args.sizes, None), "new": (args.new_lib, args.sizes, None),
            "parent2": (args.parent_lib, args.sizes, None), "off": (args.new_lib, args.sizes, None)}
    for g in args.groups:
        cfgs[f"new_g{g}"] = (args.new_lib, [top], g)
    runs = {c: [] for c in cfgs}
    for _ in range(args.rounds):
        for cfg, (lib, sizes, grp) in cfgs.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--child", lib, "--config", cfg, "--reps", str(args.reps),
                   "--warmup", str(args.warmup), "--sizes", ",".join(map(str, sizes))]
            if grp is not None:
                cmd.append("--no-forged")
            env = dict(os.environ)
            env.pop("NWV_BLS_BATCH_GROUP", None)
            if grp is not None:
                env["NWV_BLS_BATCH_GROUP"] = str(grp)
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600, env=env)
            if p.returncode != 0:  # nothing more starts on the device after a failed child
                sys.exit(f"child {cfg} failed with {p.returncode}")
            line = [x for x in p.stdout.splitlines() if x.startswith("SWEEP ")][-1]
            runs[cfg].append(json.loads(line[6:]))
            print(cfg, {n: round(v["p50_ms"], 3) for n, v in runs[cfg][-1]["sizes"].items()}, flush=True)

    def p50(cfg, n, kind="sizes", field="p50_ms"):
        return statistics.mean(r[kind][str(n)][field] for r in runs[cfg])

    table, qual = [], {}
    for n in args.sizes:
        pa, pb, nw, off = p50("parent", n), p50("parent2", n), p50("new", n), p50("off", n)
        spread = abs(pa - pb) / min(pa, pb)
        margin = max(0.10, 2 * spread)
        qual[n] = nw <= pa * (1 - margin)
        table.append({"n": n, "new_p50_ms": nw, "parent_p50_ms": pa, "parent2_p50_ms": pb, "off_p50_ms": off,
                      "new_pairing_stage_ms": p50("new", n, field="pairing_stage_p50_ms"),
                      "parent_pairing_stage_ms": p50("parent", n, field="pairing_stage_p50_ms"),
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
    chosen = next((g["group"] for g in sorted(groups, key=lambda g: g["group"]) if g["p50_ms"] <= best * (1 + top_spread)),
                  None)
    forged = [{"n": n, "new_p50_ms": p50("new", n, "forged"), "parent_p50_ms": p50("parent", n, "forged"),
               "new_groups_rejected_rechecked": runs["new"][-1]["forged"][str(n)].get("groups_rejected_rechecked")}
              for n in FORGED_SIZES if n in args.sizes and not args.no_forged]
    out = {"workload": "one-key items, 100 registered keys, 32-byte messages, all valid, host->host p50",
           "reps": args.reps, "warmup": args.warmup, "rounds": args.rounds, "table": table,
           "group_sizes_at_largest_n": groups, "chosen_group": chosen, "forged_1pct": forged,
           "recommended_wave_batch_min": recommended if recommended is not None else "none", "runs": runs}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps({"table": table, "groups": groups, "chosen_group": chosen, "forged": forged,
                      "recommended_wave_batch_min": out["recommended_wave_batch_min"]}, indent=1))


if __name__ == "__main__":
    main()
