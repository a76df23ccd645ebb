#!/usr/bin/env python3
"""p50 / p99 of the C call nwv_ed25519_verify_batch_keyed alone, over inputs packed once: 1,024
signatures by a registered 100-key committee (k_ed_comb) and 8 signatures by 4 of its keys
(k_ed_tiny), argv[1] calls each (default 1,000).  Both calls take and release the key cache's hold
(keycache_alloc.h).  With argv[1] = "epoch": the host wall time of nwv_keycache_retain and of the
nwv_keycache_register after it for fully rotated 100-key committees, medians and maxima of 10
epochs.  One JSON line (profiles/retain_latency_ab.json)."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def committee(eng, m, seed):
    rng = np.random.default_rng(seed)
    seeds = [rng.bytes(32) for _ in range(m)]
    pk, _ = eng.sign_many(seeds, [b"k"] * m)
    return seeds, [pk[32 * i:32 * i + 32].tobytes() for i in range(m)]


def epochs(eng):
    ts = {"retain_ms": [], "register_ms": [], "both_ms": []}
    for k in range(12):
        new = committee(eng, 100, 9100 + k)[1]
        t0 = time.perf_counter()
        out = eng.keycache_retain(new)
        t1 = time.perf_counter()
        eng.keycache_register(new)
        t2 = time.perf_counter()
        assert out["slots_retired"] == 100 and out["combs_retired"] == 100, out
        if k >= 2:
            for nm, v in (("retain_ms", t1 - t0), ("register_ms", t2 - t1), ("both_ms", t2 - t0)):
                ts[nm].append(v * 1e3)
    r = {"epochs": 10, "committee": 100, "stats_end": eng.keycache_stats()}
    r.update({k: float(np.median(v)) for k, v in ts.items()})
    r.update({k.replace("_ms", "_max_ms"): float(max(v)) for k, v in ts.items()})
    return r


def latencies(eng, com, reps):
    from narwhal_amd import _lib
    rng = np.random.default_rng(7)
    out = {}
    for n, nk in ((1024, 100), (8, 4)):
        kidx = [int(x) for x in rng.integers(0, nk, n)]
        msgs = [rng.bytes(32) for _ in range(n)]
        _, sg = eng.sign_many([com[0][k] for k in kidx], msgs)
        sg = np.ascontiguousarray(sg[:64 * n])
        arena, offs, lens = _lib.pack_messages(msgs)
        kb = np.frombuffer(b"".join(com[1][:nk]), dtype=np.uint8)
        ki = np.asarray(kidx, dtype=np.uint32)
        allv = _lib._i32(0)
        c0 = eng.diag_counters_ex()
        lat = []
        for r in range(reps + 20):
            t = time.perf_counter()
            rc = eng.lib.nwv_ed25519_verify_batch_keyed(eng._h, nk, _lib._ptr(kb), n, _lib._ptr(ki), _lib._ptr(sg),
                                                        _lib._ptr(arena), _lib._ptr(offs), _lib._ptr(lens),
                                                        bytes([r % 256]) * 32, ctypes.byref(allv), None)
            dt = time.perf_counter() - t
            assert rc == 0 and allv.value == 1
            if r >= 20:
                lat.append(dt)
        c1 = eng.diag_counters_ex()
        out["n%d" % n] = {"p50_ms": float(np.median(lat)) * 1e3, "p99_ms": float(np.percentile(lat, 99)) * 1e3,
                          "runs": {k: c1[k] - c0[k] for k in c1}}
    return out


def main():
    import narwhal_amd
    eng = narwhal_amd.Engine(device=0)
    com = committee(eng, 100, 9000)
    eng.keycache_register(com[1])
    if len(sys.argv) > 1 and sys.argv[1] == "epoch":
        r = epochs(eng)
    else:
        r = latencies(eng, com, int(sys.argv[1]) if len(sys.argv) > 1 else 1000)
    eng.close()
    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
