#!/usr/bin/env python3
"""Latency of certificate-shaped BLS calls with and without the aggregate-key ring
(nwv_bls_set_apk_ring): the C call alone, over inputs packed once, one JSON line a run
(profiles/bls_apk_ring_latency.json collects them).  Run every mode in a fresh process; NWV_LIB
selects another build of the library in narwhal_amd/lib (the parent commit's, for the ring-off
comparison).

  off [reps]    ring off, works with either library: p50 / p99 of a single nwv_bls_verify by a
                registered key, of one 67-of-100 certificate item (nwv_bls_verify_many, one item),
                and p50 of the 100-certificate nwv_bls_verify_mixed_many
  ring [reps]   this library: one certificate-shaped item of 3 and of 67 registered keys (of 100)
                with the ring off, at its set's first sighting (noted), at the second (the call
                that fills the slot) and as a hit -- each over reps different sets, so the three
                passes are the same calls in the same order -- then the same hit with the message
                ring on too, and the 100-certificate nwv_bls_verify_mixed_many over five recurring
                signer sets with the ring off and fully warm"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bls_msg_ring_lat import WARM, Round, single, timed  # noqa: E402


class Item:
    """one aggregate item over its own key table, packed for nwv_bls_verify_many"""

    def __init__(self, bls, rd, who, msg):
        import bls_ffi as B
        keys = [rd.com.keys[k] for k in who]
        sigs = bls.sign([rd.sk_of[k] for k in keys], [msg] * len(keys))
        rc, agg = B.aggregate(sigs)
        assert rc == 0
        self.kb = np.frombuffer(b"".join(keys), dtype=np.uint8)
        self.sig = np.frombuffer(agg, dtype=np.uint8)
        self.off = np.zeros(1, dtype=np.uint32)
        self.cnt = np.array([len(who)], dtype=np.uint32)
        self.idx = np.arange(len(who), dtype=np.uint32)
        self.msg = np.frombuffer(msg + bytes(8), dtype=np.uint8)
        self.moff = np.zeros(1, dtype=np.uint64)
        self.mlen = np.array([len(msg)], dtype=np.uint32)
        self.st = np.full(1, -1, dtype=np.int32)
        self.n_keys = len(who)

    def call(self, bls):
        f, h = bls.lib.nwv_bls_verify_many, bls._h
        a = (h, self.n_keys, self.kb.ctypes.data, 1, self.sig.ctypes.data, self.off.ctypes.data, self.cnt.ctypes.data,
             self.idx.ctypes.data, self.msg.ctypes.data, self.moff.ctypes.data, self.mlen.ctypes.data, None, 0,
             self.st.ctypes.data)
        return lambda: f(*a) or int(self.st[0])


def recurring_certificates(rd, n_sets=5):
    """the round's 100 certificates, signed by n_sets quorums in turn"""
    T, com = rd.T, rd.com
    q, n = com.quorum_threshold(), len(com.keys)
    sets = [sorted(rd.rnd.sample(range(n), q)) for _ in range(n_sets)]
    hs = rd.headers(range(n), 1)
    votes = [T.Vote(h.id, h.round, 0, h.author, com.keys[v], bytes(48)) for a, h in enumerate(hs) for v in sets[a % n_sets]]
    for v, s in zip(votes, rd.bls.sign([rd.sk_of[v.author] for v in votes], T.bls_vote_digests(rd.eng, votes))):
        v.signature = s
    return [T.BlsCertificate.new(rd.eng, com, h, [(v.author, v.signature) for v in votes[a * q:(a + 1) * q]])
            for a, h in enumerate(hs)]


def mode_off(eng, bls, reps):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    rd = Round(eng, bls)
    pk = rd.com.keys[0]
    msg = rd.rnd.randbytes(32)
    sig = bls.sign([rd.sk_of[pk]], [msg])[0]
    out = {"single_verify": timed([single(eng, pk, msg, sig)] * (reps + WARM))}
    it = Item(bls, rd, sorted(rd.rnd.sample(range(100), 67)), rd.rnd.randbytes(32))
    out["one_certificate_67_of_100"] = timed([it.call(bls)] * (reps + WARM))
    certs = recurring_certificates(rd)
    out["mixed_100_certificates"] = timed([rd.packed_call(certs=certs)] * (20 + WARM))
    return out


def mode_ring(eng, bls, reps):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    rd = Round(eng, bls)
    out = {}
    certs = recurring_certificates(rd)
    mixed = rd.packed_call(certs=certs)
    out["off_mixed_100_certificates"] = timed([mixed] * (20 + WARM))
    items = {}
    for k in (3, 67):
        items[k] = [Item(bls, rd, sorted(rd.rnd.sample(range(100), k)), rd.rnd.randbytes(32)) for _ in range(reps + WARM)]
        calls = [it.call(bls) for it in items[k]]
        out["off_%d" % k] = [timed(calls) for _ in range(3)]          # (their spread is what a difference is read against)
        out["off_%d_same_set" % k] = timed(calls[:1] * (reps + WARM))
    bls.set_apk_ring(4096)
    for k in (3, 67):
        calls = [it.call(bls) for it in items[k]]
        for leg in ("first_sighting", "filling_call", "hit"):
            out["on_%d_%s" % (k, leg)] = timed(calls)
            out["on_%d_%s_counters" % (k, leg)] = bls.last_apk()
        out["on_%d_hit_same_set" % k] = timed(calls[:1] * (reps + WARM))
    out["on_mixed_100_certificates_first_calls"] = [mixed() or bls.last_apk() for _ in range(2)]
    out["on_mixed_100_certificates_warm"] = timed([mixed] * (20 + WARM))
    out["on_mixed_100_certificates_warm_counters"] = bls.last_apk()
    out["ring_stats"] = list(bls.apk_ring_stats())
    bls.set_msg_ring(4096)
    for k in (3, 67):
        out["on_%d_hit_same_set_msg_ring" % k] = timed([items[k][0].call(bls)] * (reps + WARM))
        out["on_%d_hit_same_set_msg_ring_counters" % k] = [bls.last_apk(), bls.last_msgs()]
    bls.set_apk_ring(0)
    for k in (3, 67):
        out["off_%d_same_set_msg_ring" % k] = timed([items[k][0].call(bls)] * (reps + WARM))
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
