"""Child process of tests/test_gpu_tail_rc.py: the smallest batches that take the lane bucket kernel
(k_msm_bucket, above 4,096 signatures) with the tail's chunk sums lane-local, under the environment
the parent sets (the library reads its knobs once per process).  Per size:

  clean      the valid batch accepts, every bit set, no per-signature pass;
  forged     one signature's s changed: rejected, and the bits are the oracle's (bad set exact,
             through the per-signature fallback);
  pair       a cancelling forgery pair (tests/zcoeff.py) far enough apart to sit in different
             buckets and bucket lanes: accepted under the construction's seed, rejected under
             another (zcoeff_gpu_check.three_checks);
  keyed      the same three over 100 keys in the key cache (the split form's z-only layout).

Prints one JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import zcoeff_gpu_check as zg  # noqa: E402

SIZES = [4160, 8229]
KEYS = 100


def chunk_sizes(widths, tail_s):
    """C of every window's chunks"""
    return sorted({(1 << (w - 1)) // min(tail_s, 1 << (w - 1)) for w in widths})


def forged_one(eng, run, oracle_items, sigs, at):
    bad = list(sigs)
    s = bytearray(bad[at])
    s[40] ^= 4  # in s
    bad[at] = bytes(s)
    want = zg.oracle_bits(oracle_items(bad))
    c0 = eng.diag_counters_ex()
    ok_nb, _ = run(bad, zg.S, False)
    ok, bits = run(bad, zg.S, True)
    c1 = eng.diag_counters_ex()
    return {"oracle_bad_set": [i for i, b in enumerate(want) if not b], "rejects_nobits": not ok_nb,
            "rejects_bits": not ok, "bits_are_the_oracles": list(bits) == want,
            "fallback_ran": c1["each"] > c0["each"], "msm_runs": c1["msm"] - c0["msm"]}


def cases(eng, run, oracle_items, sigs, tag):
    n = len(sigs)
    r = {"forged": forged_one(eng, run, oracle_items, sigs, (2 * n) // 3)}
    # the pair's three checks start with the clean batch (valid_accepts)
    r["pair"] = zg.three_checks(eng, run, oracle_items, sigs, P=(n // 5, n - 7), tag=tag)
    return r


def main():
    import narwhal_amd
    from narwhal_amd import _lib
    out = {}
    eng = narwhal_amd.Engine(device=0, flags=_lib.NWV_FLAG_MSM_ALWAYS)
    keys, _, sigs, msgs = zg.signed(eng, max(SIZES), max(SIZES), 21)
    kkeys, kidx, ksigs, kmsgs = zg.signed(eng, max(SIZES), KEYS, 22)
    for n in SIZES:
        def plain(n=n):
            pk, sg, ms = keys[:n], sigs[:n], msgs[:n]
            r = cases(eng, zg.batch_run(eng, pk, ms), lambda f: list(zip(pk, f, ms)), sg, n)
            p = zg.plan(n, n)
            r["plan"] = {k: p[k] for k in ("widths", "seg", "tail_S", "chunks", "entries", "buckets")}
            r["chunk_sizes"] = chunk_sizes(p["widths"], p["tail_S"])
            r["plan_matches_engine"] = zg.plan_matches(zg.staged_stats(eng, pk, sg, ms), p)
            return r
        zg.guarded(out, f"plain_{n}", plain)

        def keyed(n=n):
            ki, sg, ms = kidx[:n], ksigs[:n], kmsgs[:n]
            r = cases(eng, zg.keyed_run(eng, kkeys, ki, ms), lambda f: [(kkeys[ki[i]], f[i], ms[i]) for i in range(n)],
                      sg, n + 1)
            p = zg.plan(n, 2 * KEYS + 1, split=True)
            r["chunk_sizes"] = chunk_sizes(p["widths"], p["tail_S"])
            return r
        zg.guarded(out, f"keyed_{n}", keyed)
    eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
