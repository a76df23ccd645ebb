#!/usr/bin/env python3
"""Host-to-host latency of the fastcrypto trait-surface calls, p50 / p99 over --reps calls each
(default 1,000) on inputs packed once (profiles/trait_grouped.json):

  cert4     nwv_ed25519_aggregate_verify, 3 signatures by a registered 4-key committee
  cert100   nwv_ed25519_aggregate_verify, 67 signatures by a registered 100-key committee
  round100  nwv_ed25519_aggregate_batch_verify, 100 aggregates x 67 signatures, the same committee
  strangers nwv_ed25519_verify_batch_empty_fail, 1,024 distinct unregistered keys (where the
            grouping pass cannot help)

The library is loaded by path (--lib, default narwhal_amd/lib/libnwv.so) with only the entry
points that every build since the trait surface has, so the same driver measures an earlier
commit's library for the A/B.  --helper times the grouping helper alone on the CPU
(tests/_build/libgroupkeys.so; no GPU).  One JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def load(path):
    L = ctypes.CDLL(path)
    vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.nwv_init_device.argtypes, L.nwv_init_device.restype = [ctypes.POINTER(vp), i32, ctypes.c_uint32], i32
    L.nwv_free.argtypes, L.nwv_free.restype = [vp], None
    L.nwv_keycache_register.argtypes, L.nwv_keycache_register.restype = [vp, sz, vp], i32
    L.nwv_diag_counters_ex.argtypes, L.nwv_diag_counters_ex.restype = [vp, vp, i32], i32
    L.nwv_ed25519_sign_many.argtypes, L.nwv_ed25519_sign_many.restype = [vp, sz, vp, vp, vp, vp, vp, vp], i32
    L.nwv_ed25519_verify_batch_empty_fail.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp]
    L.nwv_ed25519_aggregate_verify.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp]
    L.nwv_ed25519_aggregate_batch_verify.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, sz, vp]
    return L


def counters(L, h):
    out = np.zeros(4, dtype=np.uint64)
    assert L.nwv_diag_counters_ex(h, out.ctypes.data, 4) == 4
    return dict(zip(("tiny", "msm", "each", "comb"), (int(x) for x in out)))


def sign(L, h, seeds, msgs):
    n = len(seeds)
    lens = np.fromiter((len(m) for m in msgs), dtype=np.uint32, count=n)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    arena = np.frombuffer(b"".join(msgs) + bytes(16), dtype=np.uint8)
    sd = np.frombuffer(b"".join(seeds), dtype=np.uint8)
    pk, sg = np.zeros(32 * n, dtype=np.uint8), np.zeros(64 * n, dtype=np.uint8)
    rc = L.nwv_ed25519_sign_many(h, n, sd.ctypes.data, arena.ctypes.data, offs.ctypes.data, lens.ctypes.data,
                                 pk.ctypes.data, sg.ctypes.data)
    assert rc == 0
    return ([pk[32 * i:32 * i + 32].tobytes() for i in range(n)], [sg[64 * i:64 * i + 64].tobytes() for i in range(n)])


def timed(L, h, call, reps):
    c0 = counters(L, h)
    lat = []
    for r in range(reps + 50):
        seed = bytes([r % 256]) * 32
        t = time.perf_counter()
        rc = call(seed)
        dt = time.perf_counter() - t
        assert rc == 0, rc
        if r >= 50:
            lat.append(dt)
    c1 = counters(L, h)
    return {"p50_ms": float(np.median(lat)) * 1e3, "p99_ms": float(np.percentile(lat, 99)) * 1e3,
            "mean_ms": float(np.mean(lat)) * 1e3, "reps": reps, "runs": {k: c1[k] - c0[k] for k in c1}}


def gpu(a):
    L = load(a.lib)
    h = ctypes.c_void_p()
    assert L.nwv_init_device(ctypes.byref(h), 0, 0) == 0
    rng = np.random.default_rng(2024)
    cases = [c for c in a.cases.split(",") if c]
    out = {"lib": os.path.basename(a.lib), "note": a.note}
    seeds100 = [rng.bytes(32) for _ in range(100)]
    keys100, _ = sign(L, h, seeds100, [b"k"] * 100)
    seeds4 = [rng.bytes(32) for _ in range(4)]
    keys4, _ = sign(L, h, seeds4, [b"k"] * 4)
    reg = np.frombuffer(b"".join(keys100 + keys4), dtype=np.uint8)
    assert L.nwv_keycache_register(h, 104, reg.ctypes.data) == 0
    if "cert4" in cases:
        d = rng.bytes(32)
        _, sg = sign(L, h, seeds4[:3], [d] * 3)
        pk, sg = b"".join(keys4[:3]), b"".join(sg)
        out["cert4"] = timed(L, h, lambda s: L.nwv_ed25519_aggregate_verify(h, sg, 3, pk, 3, d, 32, s), a.reps)
    if "cert100" in cases:
        d = rng.bytes(32)
        who = sorted(int(x) for x in rng.permutation(100)[:67])
        _, sg = sign(L, h, [seeds100[k] for k in who], [d] * 67)
        pk1, sg1 = b"".join(keys100[k] for k in who), b"".join(sg)
        out["cert100"] = timed(L, h, lambda s: L.nwv_ed25519_aggregate_verify(h, sg1, 67, pk1, 67, d, 32, s), a.reps)
    if "round100" in cases:
        ds, pks, sgs = [], [], []
        for _ in range(100):
            d = rng.bytes(32)
            who = sorted(int(x) for x in rng.permutation(100)[:67])
            _, sg = sign(L, h, [seeds100[k] for k in who], [d] * 67)
            ds.append(d)
            pks.append(b"".join(keys100[k] for k in who))
            sgs.append(b"".join(sg))
        arr = lambda xs: (ctypes.c_char_p * len(xs))(*xs)  # noqa: E731
        ap, asg, am = arr(pks), arr(sgs), arr(ds)
        n67, n32 = (ctypes.c_size_t * 100)(*[67] * 100), (ctypes.c_size_t * 100)(*[32] * 100)
        out["round100"] = timed(
            L, h, lambda s: L.nwv_ed25519_aggregate_batch_verify(h, 100, asg, n67, ap, n67, am, n32, 100, s), a.reps)
    if "strangers" in cases:
        d = rng.bytes(32)
        sd = [rng.bytes(32) for _ in range(1024)]
        ks, sg = sign(L, h, sd, [d] * 1024)
        pk2, sg2 = b"".join(ks), b"".join(sg)
        out["strangers"] = timed(
            L, h, lambda s: L.nwv_ed25519_verify_batch_empty_fail(h, d, 32, pk2, 1024, sg2, 1024, s), a.reps)
    L.nwv_free(h)
    print(json.dumps(out), flush=True)


def helper(a):
    """the grouping pass alone: nanoseconds per call, medians of 9 runs of --reps groupings"""
    G = ctypes.CDLL(os.path.join(ROOT, "tests", "_build", "libgroupkeys.so"))
    G.gk_new.restype = ctypes.c_void_p
    G.gk_time_ns.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
    G.gk_time_ns.restype = ctypes.c_double
    rng = np.random.default_rng(5)
    g = ctypes.c_void_p(G.gk_new())
    out = {"note": a.note}
    k1024 = np.frombuffer(rng.bytes(32 * 1024), dtype=np.uint8)
    com = [rng.bytes(32) for _ in range(100)]
    k6800 = np.frombuffer(b"".join(com * 68), dtype=np.uint8)
    for name, kb, n, lim in (("n1024_distinct_full_pass", k1024, 1024, 0),
                             ("n1024_distinct_stops_past_half", k1024, 1024, 512),
                             ("n6800_over_100_keys", k6800, 6800, 0)):
        runs = sorted(G.gk_time_ns(g, kb.ctypes.data, n, lim, a.reps) for _ in range(9))
        out[name] = {"median_us": runs[4] / 1e3, "min_us": runs[0] / 1e3, "max_us": runs[-1] / 1e3, "reps": a.reps}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "narwhal_amd", "lib", "libnwv.so"))
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--cases", default="cert4,cert100,round100,strangers")
    ap.add_argument("--note", default="")
    ap.add_argument("--helper", action="store_true")
    a = ap.parse_args()
    (helper if a.helper else gpu)(a)


if __name__ == "__main__":
    main()
