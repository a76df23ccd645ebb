#!/usr/bin/env python3
"""Sweep behind nwv_set_typed_fused: the typed per-call paths host to host, on the
parent commit's library and on this build with the setting off and on.

  tools/typed_fused_sweep.py --parent-lib libnwv_parent.so [--runs 3] [--reps 1000] [--out FILE]

The parent's library is a build of the parent commit placed beside this one in narwhal_amd/lib
(NWV_LIB selects it).  Every measurement is a fresh process (this script with --one); the three
columns alternate, `runs` times each.  Cases: nwv_certificate_verify, nwv_header_verify and
nwv_vote_verify of a 4-key committee (C1: 3 + 1 signatures), the certificate of a 34-key committee
(23 + 1) and of a 100-key committee (67 + 1, the comb kernel).  p50 / p99 over `reps` calls.
Qualification: the setting qualifies for a case when its median p50 is at most
the parent's median p50 x (1 - max(0.10, 2 x spread)), spread = (max - min) / min of the parent's
p50s; the setting-off column is neutral when its median p50 lies inside the parent's own range."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = ("certificate_verify_n4", "header_verify_n4", "vote_verify_n4", "certificate_verify_n34",
         "certificate_verify_n100")


def one(mode, reps):
    import narwhal_amd
    import config_legs as CL
    from narwhal_amd import types as T
    eng = narwhal_amd.Engine(device=0)
    if mode != "parent":
        eng.set_typed_fused(mode == "on")
    lib = T.lib()
    out = {"mode": mode, "lib": os.environ.get("NWV_LIB", "libnwv.so")}

    def timed(fn, cc, arr, res):
        lat = []
        for r in range(reps + 20):
            t = time.perf_counter()
            rc = fn(eng._h, ctypes.byref(cc), 1, arr, res)
            if r >= 20:
                lat.append(time.perf_counter() - t)
            assert rc == 0 and res[0] == 0
        return CL._pcts(lat)

    for n in (4, 34, 100):
        seeds, keys, com = CL.committee_fixture(eng, n, b"nwv-typed-fused-%d" % n)
        headers, votes, certs = CL.dag_round(eng, seeds, keys, com)
        keep = T._Keep()
        cc = com._c(keep)
        res = (ctypes.c_int32 * 1)()
        carr = (T._Certificate * 1)(certs[-1]._c(keep))
        out[f"certificate_verify_n{n}"] = timed(lib.nwv_certificate_verify_many, cc, carr, res)
        if n == 4:
            harr = (T._Header * 1)(headers[0]._c(keep))
            out["header_verify_n4"] = timed(lib.nwv_header_verify_many, cc, harr, res)
            varr = (T._Vote * 1)(votes[0]._c(keep))
            out["vote_verify_n4"] = timed(lib.nwv_vote_verify_many, cc, varr, res)
    out["diag_counters"] = eng.diag_counters_ex()
    out["diag_typed_fused"] = list(eng.diag_typed_fused()) if mode != "parent" else None
    eng.close()
    print(json.dumps(out), flush=True)


def sweep(a):
    runs = {"parent": [], "off": [], "on": []}
    for r in range(a.runs):
        for mode in ("parent", "off", "on"):
            env = dict(os.environ)
            env.pop("NWV_LIB", None)
            if mode == "parent":
                env["NWV_LIB"] = a.parent_lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", mode, "--reps", str(a.reps)],
                               env=env, capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-2000:])
                return p.returncode or 1
            runs[mode].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f"run {r} {mode}: " + " ".join(f"{c}={runs[mode][-1][c]['p50_ms']:.4f}" for c in CASES), flush=True)
    summary = {}
    for c in CASES:
        p50 = {m: [x[c]["p50_ms"] for x in runs[m]] for m in runs}
        p99 = {m: [x[c]["p99_ms"] for x in runs[m]] for m in runs}
        par = p50["parent"]
        spread = (max(par) - min(par)) / min(par)
        margin = max(0.10, 2 * spread)
        med = {m: statistics.median(p50[m]) for m in runs}
        summary[c] = {
            "p50_ms": p50, "p99_ms": p99, "median_p50_ms": med,
            "median_p99_ms": {m: statistics.median(p99[m]) for m in runs},
            "parent_spread": spread, "margin": margin,
            "on_vs_parent": med["on"] / med["parent"] - 1.0,
            "qualifies": med["on"] <= med["parent"] * (1.0 - margin),
            "off_inside_parent_range": min(par) <= med["off"] <= max(par),
        }
    doc = {"tool": "tools/typed_fused_sweep.py", "runs": a.runs, "reps": a.reps, "parent_lib": a.parent_lib,
           "rule": "on median p50 <= parent median p50 * (1 - max(0.10, 2 * parent spread))",
           "default": "off", "summary": summary, "raw": runs}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps({c: {k: summary[c][k] for k in ("median_p50_ms", "parent_spread", "qualifies",
                                                     "off_inside_parent_range")} for c in CASES}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=["parent", "off", "on"])
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-lib", default="libnwv_parent.so")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=float, default=240.0)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.reps)
        return 0
    return sweep(a)


if __name__ == "__main__":
    sys.exit(main())
