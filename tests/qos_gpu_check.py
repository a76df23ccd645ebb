"""Child process of tests/test_gpu_qos.py: the latency class (nwv_set_latency_max; the lease rule of
narwhal_amd/csrc/lane_pool.h inside the library) on the GPU.  The variables (NWV_LANES,
NWV_LATENCY_LANES, NWV_LATENCY_DIGEST_BYTES, NWV_DEVICE_REPLICAS) are read at nwv_init, so every
part is a process of its own.  Which class a call ran in, and on which kind of lane, is read from
nwv_diag_qos; every verdict, bad set, status, digest and DagError code is compared with the oracle.

  --part off         nothing set: both bounds read 0, no call is latency class, no reserved lane
  --part edge        bounds 64 (Ed25519) and 2 (BLS), NWV_LATENCY_DIGEST_BYTES=4096: calls at the
                     bounds are latency class on a reserved lane, calls one past them ordinary; the
                     setter's clamp; the reserved lanes' stream priority
  --part beside      NWV_LANES=1, NWV_LATENCY_LANES=1, bound 64: one thread loops a 4,096-signature
                     batch, three threads issue certificates and verify_each calls beside it
  --part beside_bls  bound 2: one thread loops a 64-item call, two threads issue single verifies
  --part keycache    a retain and a registration of a rotated committee beside two threads of
                     certificate verifies under the old and the new committee
  --part replicas    NWV_DEVICE_REPLICAS=3: six threads of latency-class calls over three device objects

Prints one JSON line: {"checks": {name: bool}, ...}."""
import argparse
import hashlib
import json
import os
import random
import struct
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import bls_ffi as B  # noqa: E402  (checker)
import oracle_ffi as of  # noqa: E402  (checker)

ED, BLS = 0, 1
R_BLS = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
KEYS = ("latency_calls", "latency_reserved", "latency_waited", "other_calls", "other_waited", "reserved_open",
        "reserved_cap", "ordinary_open")


def signed(n, seed, nkeys=None):
    """n (pk, sig, msg) items by nkeys keys (default: one key each) -> (items, keys, key index of each)"""
    rnd = random.Random(seed)
    seeds = [rnd.randbytes(32) for _ in range(nkeys or n)]
    pks = [of.pubkey(s) for s in seeds]
    out = []
    for i in range(n):
        m = rnd.randbytes(32)
        out.append((pks[i % len(seeds)], of.sign(seeds[i % len(seeds)], m), m))
    return out, pks, [i % len(seeds) for i in range(n)]


def forge(items, i, byte=33, bit=0x10):
    """a decodable forgery: one bit of s flipped"""
    p, sg, m = items[i]
    items[i] = (p, sg[:byte] + bytes([sg[byte] ^ bit]) + sg[byte + 1:], m)


def qos(eng, engine):
    """the engine's lane counters: summed over its device objects, and per device"""
    nd = eng.device_counters(engine, 0)["devices"]
    per = [eng.diag_qos(engine, i) for i in range(nd)]
    return {k: sum(p[k] for p in per) for k in KEYS}, per


def delta(a, b):
    return {k: b[k] - a[k] for k in KEYS}


def rotated_fixture(nt, old, seed):
    """a committee that keeps the last two authorities of `old` and brings two new ones"""
    fx = nt.CommitteeFixture(4, of.pubkey, of.sign, seed=seed)
    fx.seeds = old.seeds[2:] + fx.seeds[:2]
    fx.authorities = [of.pubkey(s) for s in fx.seeds]
    fx.committee = nt.Committee(fx.authorities, [1] * 4, 0, [list(range(4))] * 4)
    return fx


class Shapes:
    """The calls of the test, each with the oracle's answer computed once: every method makes the
    call on the engine and returns whether the result equals the oracle's."""

    def __init__(self, eng, bulk=0, bls_bulk=0, fixture_seed=404):
        import types_util as tu
        from types_util import nt
        from narwhal_amd import types as T
        from narwhal_amd.bls import Bls
        self.eng, self.T, self.tu, self.nt, self.bls = eng, T, tu, nt, Bls(eng)
        rnd = random.Random(77)
        # a 4-node committee: a certificate is the header's signature and 3 votes
        self.fx = nt.CommitteeFixture(4, of.pubkey, of.sign, seed=fixture_seed)
        self.certs = self.make_certs(self.fx, rnd)
        fx = self.fx
        heads = [fx.header(author_idx=a, payload=[(rnd.randbytes(32), a % 4)]) for a in range(2)]
        votes = [fx.vote((a + 1) % 4, heads[a]) for a in range(2)]
        s = votes[1]["signature"]
        votes[1] = dict(votes[1], signature=s[:20] + bytes([s[20] ^ 1]) + s[21:])
        cert = tu.oracle_certificate(fx, heads[0], [1, 2, 3])
        self.mixed = ([tu.header(h) for h in heads], [tu.vote(v) for v in votes], [tu.certificate(cert)])
        self.mixed_want = ([nt.header_verify(fx.committee, h, of.verify) for h in heads],
                           [nt.vote_verify(fx.committee, v, of.verify) for v in votes],
                           [nt.certificate_verify(fx.committee, cert, of.verify)])
        # keyed batches of 64 and 65 signatures by 8 keys, one forgery each
        self.keyed = {}
        for n in (64, 65):
            its, keys, idx = signed(n, seed=900 + n, nkeys=8)
            forge(its, n - 3)
            self.keyed[n] = (its, keys, idx, [bool(of.verify(*it)) for it in its])
        # verify_each of 8 with two forgeries; a single signature for pubkey_verify, good and forged
        self.each, _, _ = signed(8, seed=31)
        forge(self.each, 2)
        forge(self.each, 7, byte=5, bit=0x02)
        self.each_want = [bool(of.verify(*it)) for it in self.each]
        self.one, _, _ = signed(2, seed=32)
        forge(self.one, 1)
        # digests: 64 and 65 messages of 64 bytes, 2 of 4 KiB; 64 serialized batches of 64 bytes each
        # (one transaction of 44 bytes), one of them malformed
        self.msgs = {k: [rnd.randbytes(sz) for _ in range(n)] for k, (n, sz) in
                     {"64x64": (64, 64), "65x64": (65, 64), "2x4096": (2, 4096)}.items()}
        self.msgs_want = {k: [of.blake2b256(m) for m in v] for k, v in self.msgs.items()}
        self.bufs = []
        for _ in range(64):
            tx = rnd.randbytes(44)
            self.bufs.append(struct.pack("<IQ", 0, 1) + struct.pack("<Q", len(tx)) + tx)
        self.bufs[9] = self.bufs[9][:12] + struct.pack("<Q", 45) + self.bufs[9][20:]  # longer than the buffer
        self.bufs_want = [of.batch_digest_serialized(b) for b in self.bufs]
        # a large batch with one decodable forgery (the bulk caller's)
        if bulk:
            self.bulk, _, _ = signed(bulk, seed=55, nkeys=16)
            forge(self.bulk, bulk - 70)
            self.bulk_want = [bool(of.verify(*it)) for it in self.bulk]
        # BLS: 4 keys, a vote by each over one digest, one forged
        self.bsk = [rnd.randrange(1, R_BLS).to_bytes(32, "big") for _ in range(4)]
        self.bpk = [B.keygen(sk)[1] for sk in self.bsk]
        self.bmsg = hashlib.sha256(b"qos-vote").digest()
        self.bsig = [B.sign(sk, self.bmsg) for sk in self.bsk]
        self.bsig_bad = B.sign(self.bsk[0], self.bmsg + b"!")
        if bls_bulk:
            self.bb_lists = [[i % 4] for i in range(bls_bulk)]
            self.bb_sigs = [self.bsig[i % 4] for i in range(bls_bulk)]
            self.bb_sigs[bls_bulk - 5] = self.bsig_bad
            self.bb_msgs = [self.bmsg] * bls_bulk
            self.bb_want = [B.fast_aggregate_verify(self.bb_sigs[i], [self.bpk[i % 4]], self.bmsg)
                            for i in (0, 1, 2, 3, bls_bulk - 5)]

    def make_certs(self, fx, rnd):
        """a valid certificate and one with a forged vote under fx -> [(object, oracle's code)]"""
        h = fx.header(author_idx=0, payload=[(rnd.randbytes(32), 1)])
        good = self.tu.oracle_certificate(fx, h, [1, 2, 3])
        s0 = good["sigs"][0]
        bad = dict(good, sigs=[s0[:9] + bytes([s0[9] ^ 2]) + s0[10:]] + good["sigs"][1:])
        return [(self.tu.certificate(x), self.nt.certificate_verify(fx.committee, x, of.verify)) for x in (good, bad)]

    # ---- the calls ----
    def certificate(self, k=0, certs=None, fx=None):
        c, want = (certs or self.certs)[k]
        return self.T.verify_certificates(self.eng, self.tu.committee((fx or self.fx).committee), [c]) == [want] and \
            (want == 0) == (k == 0)

    def keyed_batch(self, n):
        its, keys, idx, want = self.keyed[n]
        ok, bits = self.eng.verify_batch_keyed(keys, idx, [it[1] for it in its], [it[2] for it in its])
        return (not ok) and [bool(b) for b in bits] == want and [i for i, b in enumerate(bits) if not b] == [n - 3]

    def batch65(self):
        its, _, _, want = self.keyed[65]
        ok, bits = self.eng.verify_batch(its)
        return (not ok) and [bool(b) for b in bits] == want

    def verify_each8(self):
        return [bool(b) for b in self.eng.verify_each(self.each)] == self.each_want == \
            [i not in (2, 7) for i in range(8)]

    def pubkey_verify(self, k=0):
        pk, sg, m = self.one[k]
        f = self.eng.lib.nwv_ed25519_pubkey_verify
        rc = f(self.eng._h, np.frombuffer(pk, np.uint8).ctypes.data, np.frombuffer(m, np.uint8).ctypes.data, len(m),
               np.frombuffer(sg, np.uint8).ctypes.data)
        return (rc == 0) == bool(of.verify(pk, sg, m)) == (k == 0)

    def mixed_round(self):
        got = self.T.verify_mixed(self.eng, self.tu.committee(self.fx.committee), *self.mixed)
        return tuple(got) == self.mixed_want and self.mixed_want[1][1] != 0 and self.mixed_want[2] == [0]

    def blake2b(self, k):
        return self.eng.blake2b256_many(self.msgs[k]) == self.msgs_want[k]

    def serialized(self):
        got = self.eng.batch_digest_serialized(self.bufs)
        return got == self.bufs_want and self.bufs_want[9][1] >= 0 and self.bufs_want[0][1] == -1

    def bulk_batch(self):
        ok, bits = self.eng.verify_batch(self.bulk)
        return (not ok) and [bool(b) for b in bits] == self.bulk_want and \
            [i for i, b in enumerate(bits) if not b] == [len(self.bulk) - 70]

    def bls_verify(self, k=0, forged=False):
        sg = self.bsig_bad if forged else self.bsig[k]
        want = B.verify(self.bpk[k], self.bmsg, sg)
        return self.bls.verify(self.bpk[k], self.bmsg, sg) == (0 if want == 0 else 1) and (want == 0) == (not forged)

    def bls_many(self, n):
        """n items: item i is key i's vote; the last one forged"""
        sigs = self.bsig[:n - 1] + [self.bsig_bad]
        keys = self.bpk[:n] if n > 1 else [self.bpk[0]]
        lists = [[i] for i in range(n - 1)] + [[0]]
        st = list(self.bls.verify_many(keys, sigs, lists, [self.bmsg] * n))
        want = [B.fast_aggregate_verify(sigs[i], [keys[lists[i][0]]], self.bmsg) for i in range(n)]
        return st == want and want[:-1] == [0] * (n - 1) and want[-1] != 0

    def bls_aggregate(self, n=2):
        rc, agg, _ = self.bls.aggregate(self.bsig[:n])
        wrc, wagg = B.aggregate(self.bsig[:n])
        return rc == 0 and wrc == 0 and agg == wagg

    def bls_bulk(self):
        st = list(self.bls.verify_many(self.bpk, self.bb_sigs, self.bb_lists, self.bb_msgs))
        n = len(st)
        return [st[i] for i in (0, 1, 2, 3, n - 5)] == self.bb_want and self.bb_want[:4] == [0] * 4 and \
            self.bb_want[4] != 0 and [i for i, s in enumerate(st) if s != 0] == [n - 5]


def run_threads(plans):
    """plans: one list of calls per thread, started together -> (mismatches, errors)"""
    barrier = threading.Barrier(len(plans))
    bad, errs = [], []

    def work(t):
        try:
            barrier.wait()
            for k, f in enumerate(plans[t]):
                if not f():
                    bad.append((t, k))
        except Exception as e:  # noqa: BLE001  (reported through the checks)
            errs.append(repr(e))

    th = [threading.Thread(target=work, args=(t,)) for t in range(len(plans))]
    for x in th:
        x.start()
    for x in th:
        x.join()
    return bad, errs


def part_off(out):
    import narwhal_amd
    eng = narwhal_amd.Engine(device=0)
    ck = out["checks"]
    ck["fresh_getters_are_0"] = eng.latency_max(ED) == 0 and eng.latency_max(BLS) == 0
    sh = Shapes(eng)
    big, _, _ = signed(1024, seed=12, nkeys=16)
    ck["certificate_equal"] = sh.certificate(0) and sh.certificate(1)
    ok, bits = eng.verify_batch(big)
    ck["batch_1024_accepts"] = ok and all(bits)
    ck["bls_single_verify_equal"] = sh.bls_verify(0) and sh.bls_verify(0, forged=True)
    for name, engine in (("ed25519", ED), ("bls", BLS)):
        q, _ = qos(eng, engine)
        out[name] = q
        ck[f"{name}_no_latency_call"] = q["latency_calls"] == 0 and q["latency_reserved"] == 0
        ck[f"{name}_no_reserved_lane"] = q["reserved_open"] == 0 and q["ordinary_open"] >= 1
        ck[f"{name}_calls_counted"] = q["other_calls"] >= 2
        ck[f"{name}_no_reserved_stream"] = eng.diag_qos_priority(engine)[0] == 0
    ck["getters_still_0"] = eng.latency_max(ED) == 0 and eng.latency_max(BLS) == 0
    eng.close()


def part_edge(out):
    import narwhal_amd
    eng = narwhal_amd.Engine(device=0)
    ck = out["checks"]
    sh = Shapes(eng)
    ck["warm_up"] = sh.certificate(0) and sh.bls_verify(0)  # the committee registered: an ordinary call
    eng.set_latency_max(ED, 64)
    eng.set_latency_max(BLS, 2)
    ck["getters"] = eng.latency_max(ED) == 64 and eng.latency_max(BLS) == 2
    ck["digest_bytes_env"] = os.environ.get("NWV_LATENCY_DIGEST_BYTES") == "4096"

    def classed(name, engine, call, latency):
        q0, _ = qos(eng, engine)
        ok = call()
        d = delta(q0, qos(eng, engine)[0])
        out["deltas"][name] = [d[k] for k in KEYS[:5]]
        ck[f"{name}_oracle"] = bool(ok)
        if latency:  # in [0] and [1], nothing in [3]; nobody else runs, so nothing waits
            ck[f"{name}_latency_class"] = d["latency_calls"] >= 1 and d["latency_reserved"] == d["latency_calls"] and \
                d["other_calls"] == 0 and d["latency_waited"] == 0
        else:
            ck[f"{name}_ordinary"] = d["other_calls"] >= 1 and d["latency_calls"] == 0 and d["latency_reserved"] == 0

    classed("certificate_4_sigs", ED, lambda: sh.certificate(0), True)
    classed("certificate_forged", ED, lambda: sh.certificate(1), True)
    classed("keyed_64_bad_set", ED, lambda: sh.keyed_batch(64), True)
    classed("verify_each_8", ED, sh.verify_each8, True)
    classed("pubkey_verify", ED, lambda: sh.pubkey_verify(0) and sh.pubkey_verify(1), True)
    classed("mixed_2_2_1", ED, sh.mixed_round, True)
    classed("blake2b_64x64", ED, lambda: sh.blake2b("64x64"), True)
    classed("serialized_64x64", ED, sh.serialized, True)
    classed("bls_single", BLS, lambda: sh.bls_verify(1) and sh.bls_verify(0, forged=True), True)
    classed("bls_2_items", BLS, lambda: sh.bls_many(2), True)
    classed("bls_aggregate_2", BLS, lambda: sh.bls_aggregate(2), True)
    classed("batch_65", ED, sh.batch65, False)
    classed("keyed_65", ED, lambda: sh.keyed_batch(65), False)
    classed("blake2b_65x64", ED, lambda: sh.blake2b("65x64"), False)
    classed("blake2b_2x4096", ED, lambda: sh.blake2b("2x4096"), False)
    classed("bls_3_items", BLS, lambda: sh.bls_many(3), False)
    classed("bls_aggregate_3", BLS, lambda: sh.bls_aggregate(3), False)
    # the priority in force, and the reserved lanes within their cap
    for name, engine in (("ed25519", ED), ("bls", BLS)):
        pr = eng.diag_qos_priority(engine)
        q, _ = qos(eng, engine)
        out[f"{name}_priority"], out[name] = list(pr), q
        ck[f"{name}_reserved_streams_at_the_greatest_priority"] = pr[0] == pr[1]
        ck[f"{name}_reserved_lanes_within_cap"] = 1 <= q["reserved_open"] <= q["reserved_cap"]
    # the setter's clamp: just below the shard minimum (16,384 signatures; 256 items)
    eng.set_latency_max(ED, 16384)
    eng.set_latency_max(BLS, 1 << 20)
    out["clamped"] = [eng.latency_max(ED), eng.latency_max(BLS)]
    ck["clamped_below_the_shard_minimum"] = out["clamped"] == [16383, 255]
    eng.set_latency_max(ED, 16383)
    ck["below_the_minimum_kept"] = eng.latency_max(ED) == 16383
    eng.set_latency_max(ED, 0)
    eng.set_latency_max(BLS, 0)
    q0, _ = qos(eng, ED)
    ck["off_again"] = sh.certificate(0) and delta(q0, qos(eng, ED)[0])["latency_calls"] == 0
    eng.close()


def part_beside(out):
    import narwhal_amd
    eng = narwhal_amd.Engine(device=0)
    ck = out["checks"]
    sh = Shapes(eng, bulk=4096)
    ck["warm_up"] = sh.certificate(0) and sh.verify_each8()
    eng.set_latency_max(ED, 64)
    q0, _ = qos(eng, ED)
    n_bulk, n_cert, n_each, n_fg = 40, 100, 30, 3
    fg = [lambda: sh.certificate(0)] * (n_cert // 2) + [lambda: sh.certificate(1)] * (n_cert // 2) + \
        [sh.verify_each8] * n_each
    plans = [[sh.bulk_batch] * n_bulk]
    for t in range(n_fg):
        calls = list(fg)
        random.Random(40 + t).shuffle(calls)
        plans.append(calls)
    bad, errs = run_threads(plans)
    out["mismatches"], out["errors"] = bad, errs
    ck["every_result_equals_the_oracle"] = not bad and not errs
    d = delta(q0, qos(eng, ED)[0])
    q, _ = qos(eng, ED)
    out["delta"], out["qos"] = d, q
    ck["latency_calls_equal_calls_issued"] = d["latency_calls"] == n_fg * (n_cert + n_each)
    ck["reserved_at_most_latency"] = d["latency_reserved"] <= d["latency_calls"]
    ck["bulk_calls_counted"] = d["other_calls"] >= n_bulk
    ck["one_lane_of_each_kind"] = q["reserved_open"] == 1 == q["reserved_cap"] and q["ordinary_open"] == 1
    eng.close()


def part_beside_bls(out):
    import narwhal_amd
    eng = narwhal_amd.Engine(device=0)
    ck = out["checks"]
    sh = Shapes(eng, bls_bulk=64)
    ck["warm_up"] = sh.bls_verify(0) and sh.bls_bulk()
    eng.set_latency_max(BLS, 2)
    q0, _ = qos(eng, BLS)
    n_bulk, n_single, n_fg = 10, 20, 2
    plans = [[sh.bls_bulk] * n_bulk]
    for t in range(n_fg):
        plans.append([(lambda k=k: sh.bls_verify(k % 4, forged=(k % 5 == 4))) for k in range(n_single)])
    bad, errs = run_threads(plans)
    out["mismatches"], out["errors"] = bad, errs
    ck["every_result_equals_the_oracle"] = not bad and not errs
    d = delta(q0, qos(eng, BLS)[0])
    q, _ = qos(eng, BLS)
    out["delta"], out["qos"] = d, q
    ck["latency_calls_equal_calls_issued"] = d["latency_calls"] == n_fg * n_single
    ck["reserved_at_most_latency"] = d["latency_reserved"] <= d["latency_calls"]
    ck["bulk_calls_counted"] = d["other_calls"] >= n_bulk
    ck["reserved_lanes_within_cap"] = 1 <= q["reserved_open"] <= q["reserved_cap"]
    eng.close()


def part_keycache(out):
    import narwhal_amd
    eng = narwhal_amd.Engine(device=0)
    ck = out["checks"]
    sh = Shapes(eng)
    new_fx = rotated_fixture(sh.nt, sh.fx, seed=505)
    new_certs = sh.make_certs(new_fx, random.Random(8))
    ck["committees_share_two_keys"] = len(set(sh.fx.authorities) & set(new_fx.authorities)) == 2
    ck["warm_up"] = sh.certificate(0)
    eng.set_latency_max(ED, 64)
    q0, _ = qos(eng, ED)
    retained = {}

    def epoch_change():
        retained.update(eng.keycache_retain(list(new_fx.committee.keys)))
        eng.keycache_register(list(new_fx.committee.keys))
        return True

    n = 40
    plans = [[epoch_change],
             [(lambda k=k: sh.certificate(k % 2)) for k in range(n)],
             [(lambda k=k: sh.certificate(k % 2, new_certs, new_fx)) for k in range(n)]]
    bad, errs = run_threads(plans)
    out["mismatches"], out["errors"], out["retained"] = bad, errs, retained
    ck["every_verdict_equals_the_oracle"] = not bad and not errs
    ck["retain_returned"] = "used" in retained and retained["used"] >= 1
    d = delta(q0, qos(eng, ED)[0])
    out["delta"] = d
    ck["certificates_were_latency_class"] = d["latency_calls"] == 2 * n
    ck["both_committees_verify_afterwards"] = sh.certificate(0) and sh.certificate(0, new_certs, new_fx) and \
        sh.certificate(1, new_certs, new_fx)
    eng.close()


def part_replicas(out):
    import narwhal_amd
    eng = narwhal_amd.Engine(device=None, n_devices=0)
    ck = out["checks"]
    sh = Shapes(eng)
    ck["three_device_objects"] = eng.device_count == 3
    ck["warm_up"] = sh.certificate(0)
    eng.set_latency_max(ED, 64)
    q0, _ = qos(eng, ED)
    n_threads, n_calls = 6, 24
    shapes = [lambda: sh.certificate(0), lambda: sh.certificate(1), sh.verify_each8, lambda: sh.keyed_batch(64),
              lambda: sh.blake2b("64x64"), sh.mixed_round]
    plans = []
    for t in range(n_threads):
        calls = [shapes[(t + k) % len(shapes)] for k in range(n_calls)]
        plans.append(calls)
    bad, errs = run_threads(plans)
    out["mismatches"], out["errors"] = bad, errs
    ck["every_result_equals_the_oracle"] = not bad and not errs
    q1, per = qos(eng, ED)
    d = delta(q0, q1)
    out["delta"], out["per_device"] = d, [[p[k] for k in KEYS] for p in per]
    ck["counters_sum_to_the_calls_issued"] = d["latency_calls"] == n_threads * n_calls and d["other_calls"] == 0
    ck["reserved_lanes_within_cap_on_every_device"] = all(p["reserved_open"] <= p["reserved_cap"] for p in per)
    ck["a_reserved_lane_somewhere"] = sum(p["reserved_open"] for p in per) >= 1
    eng.close()


PARTS = {"off": part_off, "edge": part_edge, "beside": part_beside, "beside_bls": part_beside_bls,
         "keycache": part_keycache, "replicas": part_replicas}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=sorted(PARTS), required=True)
    a = ap.parse_args()
    out = {"part": a.part, "checks": {}, "deltas": {}}
    PARTS[a.part](out)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
