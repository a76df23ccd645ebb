#!/usr/bin/env python3
"""Latency of small BLS calls with and without the message ring (nwv_bls_set_msg_ring): the C call
alone, over inputs packed once, one JSON line a run (profiles/bls_msg_ring_latency.json collects
them).  Run every mode in a fresh process; NWV_LIB selects another build of the library in
narwhal_amd/lib (the parent commit's, for the ring-off comparison).

  off [reps]    ring off, works with either library: p50 / p99 of a single nwv_bls_verify by a
                registered key, and p50 of the 100-certificate nwv_bls_verify_mixed_many
  ring [reps]   this library: a single nwv_bls_verify with the ring off, then on -- a cached
                message by a registered key (the record is copied) and by an unregistered key (the
                h_eff chain runs on it), a cold message (the miss path: reserve, publish) -- and a
                header-only nwv_bls_verify_mixed_many of 4 fresh headers with the ring off and on
                (on: 4 certificate digests hashed ahead beside the checks)"""
import ctypes
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
WARM = 20


def stats(lat):
    return {"p50_ms": float(np.median(lat)) * 1e3, "p99_ms": float(np.percentile(lat, 99)) * 1e3,
            "min_ms": float(min(lat)) * 1e3, "calls": len(lat)}


def timed(calls):
    """calls: a list of zero-argument functions returning the status to check; the first WARM are not timed"""
    lat = []
    for k, f in enumerate(calls):
        t = time.perf_counter()
        rc = f()
        dt = time.perf_counter() - t
        assert rc == 0, rc
        if k >= WARM:
            lat.append(dt)
    return stats(lat)


def single(eng, pk, msg, sig):
    f = eng.lib.nwv_bls_verify
    return lambda: f(eng._h, pk, msg, len(msg), sig)


class Round:
    """a 100-node committee, registered; its round-1 headers and certificates (as tests/test_gpu_types_bls.py)"""

    def __init__(self, eng, bls, n=100, seed=41):
        from narwhal_amd import types as T
        self.T, self.eng, self.bls = T, eng, bls
        self.rnd = random.Random(seed)
        sks = [self.rnd.randrange(1, R).to_bytes(32, "big") for _ in range(n)]
        self.sk_of = dict(zip(bls.keygen(sks), sks))
        self.com = T.Committee(sorted(self.sk_of), [1] * n, 0, [[0, 1, 2, 3]] * n)
        self.parents = T.bls_certificate_digests(eng, T.BlsCertificate.genesis(self.com))
        bls.register_keys(self.com.keys)

    def headers(self, authors, round_):
        T = self.T
        hs = [T.Header(author=self.com.keys[a], round=round_, epoch=0, payload=[(self.rnd.randbytes(32), a % 4)],
                       parents=list(self.parents), signature=bytes(48)) for a in authors]
        for h, d in zip(hs, T.bls_header_digests(self.eng, hs)):
            h.id = d
        for h, s in zip(hs, self.bls.sign([self.sk_of[h.author] for h in hs], [h.id for h in hs])):
            h.signature = s
        return hs

    def certificates(self, hs):
        T, com = self.T, self.com
        q = com.quorum_threshold()
        n = len(com.keys)
        votes = [T.Vote(h.id, h.round, 0, h.author, com.keys[v], bytes(48))
                 for a, h in enumerate(hs) for v in [i for i in range(n) if i != a][:q]]
        for v, s in zip(votes, self.bls.sign([self.sk_of[v.author] for v in votes], T.bls_vote_digests(self.eng, votes))):
            v.signature = s
        return [T.BlsCertificate.new(self.eng, com, h, [(v.author, v.signature) for v in votes[a * q:(a + 1) * q]])
                for a, h in enumerate(hs)]

    def packed_call(self, headers=(), certs=()):
        """nwv_bls_verify_mixed_many over arguments packed once -> a function returning the worst code"""
        T = self.T
        keep = T._Keep()
        c = self.com._c(keep)
        args, outs = [], []
        for items, cls in ((list(headers), T._Header), ([], T._Vote), (list(certs), T._BlsCertificate)):
            n = len(items)
            arr = (cls * max(n, 1))(*[it._c(keep) for it in items])
            res = (ctypes.c_int32 * max(n, 1))()
            keep.objs += [arr, res]
            args += [n, ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(res, ctypes.c_void_p)]
            outs.append((res, n))
        f = T.lib().nwv_bls_verify_mixed_many

        def call(_keep=keep):
            rc = f(self.eng._h, ctypes.byref(c), *args)
            return rc or max([max(r[:n]) for r, n in outs if n] or [0])
        return call


def mode_off(eng, bls, reps):
    rd = Round(eng, bls)
    pk = rd.com.keys[0]
    msg = rd.rnd.randbytes(32)
    sig = bls.sign([rd.sk_of[pk]], [msg])[0]
    out = {"single_verify": timed([single(eng, pk, msg, sig)] * (reps + WARM))}
    certs = rd.certificates(rd.headers(range(100), 1))
    out["mixed_100_certificates"] = timed([rd.packed_call(certs=certs)] * (20 + WARM))
    return out


def mode_ring(eng, bls, reps):
    rd = Round(eng, bls, n=10)
    pk = rd.com.keys[0]
    stray_sk = (12345).to_bytes(32, "big")
    stray = bls.keygen([stray_sk])[0]
    msg = rd.rnd.randbytes(32)
    sig, sig_stray = bls.sign([rd.sk_of[pk], stray_sk], [msg, msg])
    cold = [rd.rnd.randbytes(32) for _ in range(reps + WARM)]
    cold_sigs = bls.sign([rd.sk_of[pk]] * len(cold), cold)
    sets = [rd.headers(range(4), 2 + k) for k in range(30 + WARM)]   # fresh headers every call
    out = {}
    # ring off, three runs (their spread is what a difference is read against)
    out["off_single_registered"] = [timed([single(eng, pk, msg, sig)] * (reps + WARM)) for _ in range(3)]
    out["off_single_unregistered"] = timed([single(eng, stray, msg, sig_stray)] * (reps + WARM))
    out["off_single_cold"] = timed([single(eng, pk, m, s) for m, s in zip(cold, cold_sigs)])
    out["off_mixed_4_headers"] = timed([rd.packed_call(headers=hs) for hs in sets])
    bls.set_msg_ring(4096)
    sets2 = [rd.headers(range(4), 100 + k) for k in range(30 + WARM)]
    out["on_single_hit_copied"] = [timed([single(eng, pk, msg, sig)] * (reps + WARM)) for _ in range(3)]
    out["on_single_hit_copied_counters"] = bls.last_msgs()
    out["on_single_hit_chained"] = timed([single(eng, stray, msg, sig_stray)] * (reps + WARM))
    out["on_single_hit_chained_counters"] = bls.last_msgs()
    cold2 = [rd.rnd.randbytes(32) for _ in range(reps + WARM)]
    cold2_sigs = bls.sign([rd.sk_of[pk]] * len(cold2), cold2)
    out["on_single_cold"] = timed([single(eng, pk, m, s) for m, s in zip(cold2, cold2_sigs)])
    out["on_single_cold_counters"] = bls.last_msgs()
    out["on_mixed_4_headers_ahead"] = timed([rd.packed_call(headers=hs) for hs in sets2])
    out["on_mixed_4_headers_ahead_counters"] = bls.last_msgs()
    out["ring_stats"] = list(bls.msg_ring_stats())
    return out


def main():
    import narwhal_amd
    from narwhal_amd.bls import Bls
    mode = sys.argv[1] if len(sys.argv) > 1 else "off"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 300
    eng = narwhal_amd.Engine(device=0)
    bls = Bls(eng)
    out = {"mode": mode, "lib": os.environ.get("NWV_LIB", "libnwv.so"), "reps": reps}
    out.update({"off": mode_off, "ring": mode_ring}[mode](eng, bls, reps))
    eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
