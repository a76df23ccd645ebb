"""Child process of tests/test_gpu_comb_pass.py, for the cases whose environment the library reads
once per process.  --part epoch (NWV_COMB_KEYS=8): the key cache across an epoch change, the comb
pass (nwv_set_comb_pass_max) over tables that changed hands.  --part replicas
(NWV_DEVICE_REPLICAS=3): three overlapping threads on an all-devices context.  Verdict bits against
the oracle's.  Prints one JSON line."""
import argparse
import json
import os
import random
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import oracle_ffi as of  # noqa: E402  (checker)

ED = 0


def _engine(**kw):
    import narwhal_amd
    e = narwhal_amd.Engine(**kw)
    e.set_comb_batch_max(0)
    e.set_comb_pass_max(4096)
    return e


def _signed(seeds, kidx, seed):
    rnd = random.Random(seed)
    msgs = [rnd.randbytes(32) for _ in kidx]
    return [of.sign(seeds[k], m) for k, m in zip(kidx, msgs)], msgs


def _spoil(sigs, idx):
    for i in idx:
        s = bytearray(sigs[i])
        s[45] ^= 0x04
        sigs[i] = bytes(s)


def _call(e, keys, kidx, sigs, msgs):
    p0 = e.diag_comb_pass()
    ok, bits = e.verify_batch_keyed(keys, kidx, sigs, msgs)
    p1 = e.diag_comb_pass()
    want = [of.verify(keys[k], s, m) for k, s, m in zip(kidx, sigs, msgs)]
    return {"equal": bits == want, "ok": ok, "rejected": want.count(False), "pass": [p1[0] - p0[0], p1[1] - p0[1]]}, want


def _stats(e):
    s = e.keycache_stats(0)
    return [s["used"], s["comb_used"]]


def epoch():
    out = {"comb_keys": os.environ.get("NWV_COMB_KEYS")}
    e = _engine(device=0)
    rnd = random.Random(88)
    kseeds = [rnd.randbytes(32) for _ in range(8)]
    nseeds = [rnd.randbytes(32) for _ in range(4)]
    K, N = [of.pubkey(s) for s in kseeds], [of.pubkey(s) for s in nseeds]
    e.keycache_register(K)
    out["stats_K"] = _stats(e)
    r = e.keycache_retain(K[:4])  # K[4:] retire: four slots, four tables
    out["retired"] = [r["slots_retired"], r["combs_retired"]]
    out["stats_retained"] = _stats(e)
    e.keycache_register(N)
    out["stats_N"] = _stats(e)
    live, lseeds = K[:4] + N, kseeds[:4] + nseeds
    n = 100
    # live keys only
    kidx = [rnd.randrange(8) for _ in range(n)]
    sigs, msgs = _signed(lseeds, kidx, 1)
    _spoil(sigs, sorted({0, 63, 64, n - 1} | set(rnd.sample(range(n), 6))))
    out["live"], _ = _call(e, live, kidx, sigs, msgs)
    # a retired key named too (the call caches it itself, without a table)
    keys2, seeds2 = live + [K[5]], lseeds + [kseeds[5]]
    kidx2 = list(kidx)
    kidx2[10] = kidx2[70] = 8
    sigs2, msgs2 = _signed(seeds2, kidx2, 2)
    _spoil(sigs2, sorted({0, 63, 64, n - 1} | set(rnd.sample(range(n), 6))))
    out["retired_named"], _ = _call(e, keys2, kidx2, sigs2, msgs2)
    e.keycache_retain(live)  # (retire it again: the tables are as after the registration of N)
    # a signature by retired key K[4 + k] named under new key N[j], all sixteen (j, k)
    kidx3 = [rnd.randrange(8) for _ in range(n)]
    signer = [lseeds[k] for k in kidx3]
    crossed = rnd.sample(range(n), 16)
    for c, i in enumerate(crossed):
        kidx3[i] = 4 + c // 4
        signer[i] = kseeds[4 + c % 4]
    m3 = [rnd.randbytes(32) for _ in range(n)]
    sigs3 = [of.sign(s, m) for s, m in zip(signer, m3)]
    res, want = _call(e, live, kidx3, sigs3, m3)
    res["crossed_rejected"] = sum(1 for i in crossed if not want[i])
    out["crossed"] = res
    e.close()
    return out


def replicas():
    out = {}
    e = _engine(device=None, n_devices=0)
    out["devices"] = e.device_count
    rnd = random.Random(99)
    seeds = [rnd.randbytes(32) for _ in range(10)]
    keys = [of.pubkey(s) for s in seeds]
    e.keycache_register(keys)
    n = 300
    jobs = []
    for t in range(3):
        kidx = [rnd.randrange(10) for _ in range(n)]
        sigs, msgs = _signed(seeds, kidx, 10 + t)
        _spoil(sigs, sorted({0, 63, 64, n - 1} | set(rnd.sample(range(n), 5 + t))))
        want = [of.verify(keys[k], s, m) for k, s, m in zip(kidx, sigs, msgs)]
        jobs.append((kidx, sigs, msgs, want))
    got = [None] * 3
    gate = threading.Barrier(3)

    def work(t):
        kidx, sigs, msgs, _ = jobs[t]
        gate.wait(timeout=60)
        got[t] = e.verify_batch_keyed(keys, kidx, sigs, msgs)

    p0 = e.diag_comb_pass()
    d0 = [e.device_counters(ED, i)["each"] for i in range(e.device_count)]
    th = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(3)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    out["alive"] = [x.is_alive() for x in th]
    p1 = e.diag_comb_pass()
    d1 = [e.device_counters(ED, i)["each"] for i in range(e.device_count)]
    out["equal"] = [g is not None and g[1] == j[3] for g, j in zip(got, jobs)]
    out["ok"] = [g is not None and g[0] for g in got]
    out["rejected"] = [j[3].count(False) for j in jobs]
    out["sets_differ"] = jobs[0][3] != jobs[1][3] != jobs[2][3]
    out["pass"] = [p1[0] - p0[0], p1[1] - p0[1]]
    out["each_by_device"] = [b - a for a, b in zip(d0, d1)]
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["epoch", "replicas"])
    a = ap.parse_args()
    print(json.dumps(epoch() if a.part == "epoch" else replicas()))


if __name__ == "__main__":
    main()
