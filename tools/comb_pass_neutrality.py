#!/usr/bin/env python3
"""What the comb pass costs a context that leaves it off: the device sources
changed, so the parent commit's library (built in the same tree, narwhal_amd/lib/<--parent-lib>)
and this build run the same three measurements in fresh processes, alternating, --rounds times:
  headline   the plain bench.py --gpus 1: sigs/s and ms per step
  c1         tools/c1_times.py: Certificate::verify of a 4-node committee, p50
  clean7000  tools/comb_pass_sweep.py --child: the clean 7,000-signature keyed call, p50
With the limit at its default 0 the new medians should lie inside the parent's own run-to-run range.

  python tools/comb_pass_neutrality.py --parent-lib libnwv_parent.so --out profiles/comb_pass_neutrality.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cmd, env, prefix=None):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=400, env=env, cwd=ROOT)
    if p.returncode != 0:  # nothing more starts on the device after a failed child
        sys.exit(f"{cmd} failed with {p.returncode}")
    lines = [x for x in p.stdout.splitlines() if x.startswith(prefix or "{")]
    return json.loads(lines[-1][len(prefix or ""):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="file name under narwhal_amd/lib (NWV_LIB)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=192)
    ap.add_argument("--warmup", type=int, default=48)
    ap.add_argument("--out")
    a = ap.parse_args()
    libs = {"parent": a.parent_lib, "new": "libnwv.so"}
    runs = {s: {"headline_sigs_per_s": [], "headline_ms_per_step": [], "c1_certificate_p50_ms": [],
                "clean7000_p50_ms": []} for s in libs}
    py = sys.executable
    for _ in range(a.rounds):
        for side, lib in libs.items():
            env = dict(os.environ, NWV_LIB=lib)
            b = run([py, "bench.py", "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)], env)
            runs[side]["headline_sigs_per_s"].append(b["value"])
            runs[side]["headline_ms_per_step"].append(b["ms_per_step"])
            c = run([py, os.path.join("tools", "c1_times.py"), "300"], env)
            runs[side]["c1_certificate_p50_ms"].append(c["certificate_verify_n4"]["p50_ms"])
            s = run([py, os.path.join("tools", "comb_pass_sweep.py"), "--child",
                     os.path.join("narwhal_amd", "lib", lib), "--config", "parent" if side == "parent" else "off",
                     "--sizes", "7000", "--reps", "200", "--warmup", "20"], env, "SWEEP ")
            runs[side]["clean7000_p50_ms"].append(s["clean"]["7000"]["p50_ms"])
            print(side, {k: v[-1] for k, v in runs[side].items()}, flush=True)
    summary = {}
    for k in runs["parent"]:
        pa, nw = runs["parent"][k], runs["new"][k]
        if not all(isinstance(x, (int, float)) for x in pa + nw):
            continue
        summary[k] = {"parent_runs": pa, "new_runs": nw, "parent_median": statistics.median(pa),
                      "new_median": statistics.median(nw),
                      "new_median_inside_parent_range": min(pa) <= statistics.median(nw) <= max(pa)}
    out = {"protocol": f"fresh processes, parent and new alternating, {a.rounds} runs a side; "
                       f"bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup}; c1_times.py 300; "
                       "the clean 7,000-signature keyed call of comb_pass_sweep.py, 200 calls",
           "comb_pass_max": 0, "summary": summary, "runs": runs}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
