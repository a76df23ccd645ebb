"""Child process of tests/test_gpu_place.py: run with NWV_DEVICE_REPLICAS=3 and
NWV_BLS_DEVICE_REPLICAS=3 (read at nwv_init / once per process), so one GPU carries three device
objects of either engine and an all-devices context (nwv_init(ctx, 0, 0)) places every call by the
load table of narwhal_amd/csrc/place.h.  Where a call ran is read from nwv_diag_device_counters;
every verdict, bad set, status, digest and DagError code is compared with the oracle.

  --part hold     a staged batch that has run and is not synced holds its device: with device 0
                  held the next call runs on device 1, with 0 and 1 held on device 2, with both
                  synced on device 0 again -- for a certificate, a 128-signature batch, a keyed
                  batch by new keys, a BLAKE2b call, a mixed round and a serialized-batch digest;
                  BLS single verifies, and aggregates that follow their signatures' ring
  --part rotate   (NWV_SHARD_MIN=64) three 128-signature batches of two ranges each leave two
                  ranges on every device; under NWV_PLACE=first 3, 3 and 0
  --part threads  six threads x twelve calls of all the shapes above at once

Prints one JSON line: {"checks": {name: bool}, ...}."""
import argparse
import hashlib
import json
import os
import random
import struct
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import bls_ffi as B  # noqa: E402  (checker)
import oracle_ffi as of  # noqa: E402  (checker)

ED, BLS = 0, 1
R_BLS = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


class Shapes:
    """The calls of the test, each with the oracle's answer computed once: call(name) makes the
    call on the engine and returns whether the result equals the oracle's."""

    def __init__(self, eng):
        import types_util as tu
        from types_util import nt
        from narwhal_amd import types as T
        from narwhal_amd.bls import Bls
        self.eng, self.T, self.tu, self.bls = eng, T, tu, Bls(eng)
        rnd = random.Random(2024)
        self.rnd = rnd
        # a 4-node committee: a certificate of 1 + 3 signatures; a round of 4 headers, 4
        # certificates and 3 votes with one bad vote
        fx = nt.CommitteeFixture(4, of.pubkey, of.sign, seed=404)
        self.c = tu.committee(fx.committee)
        q = fx.committee.quorum_threshold()
        heads = [fx.header(author_idx=a, payload=[(rnd.randbytes(32), a % 4)]) for a in range(4)]
        certs = [tu.oracle_certificate(fx, heads[a], [i for i in range(4) if i != a][:q]) for a in range(4)]
        votes = [fx.vote((a + 1) % 4, heads[a]) for a in range(3)]
        s = votes[1]["signature"]
        votes[1] = dict(votes[1], signature=s[:20] + bytes([s[20] ^ 1]) + s[21:])
        bad_cert = dict(certs[2], sigs=[certs[2]["sigs"][0][:9] + bytes([certs[2]["sigs"][0][9] ^ 2]) +
                                        certs[2]["sigs"][0][10:]] + certs[2]["sigs"][1:])
        self.cert = [tu.certificate(certs[0]), tu.certificate(bad_cert)]
        self.cert_want = [nt.certificate_verify(fx.committee, x, of.verify) for x in (certs[0], bad_cert)]
        self.mixed = ([tu.header(h) for h in heads], [tu.vote(v) for v in votes], [tu.certificate(x) for x in certs])
        self.mixed_want = ([nt.header_verify(fx.committee, h, of.verify) for h in heads],
                           [nt.vote_verify(fx.committee, v, of.verify) for v in votes],
                           [nt.certificate_verify(fx.committee, x, of.verify) for x in certs])
        # a 128-signature batch with one forgery
        self.batch = self.signed(128, seed=7)
        p, sg, m = self.batch[77]
        self.batch[77] = (p, sg[:33] + bytes([sg[33] ^ 0x10]) + sg[34:], m)
        self.batch_want = [bool(of.verify(*it)) for it in self.batch]
        # 8 BLAKE2b messages (0, 1 and 2 blocks, one above the quad kernel's 1 KiB)
        self.msgs = [rnd.randbytes(n) for n in (0, 1, 64, 127, 128, 129, 300, 1500)]
        self.msgs_want = [of.blake2b256(m) for m in self.msgs]
        # serialized worker batches, one malformed (truncated inside a transaction)
        txs = [rnd.randbytes(40) for _ in range(5)]
        ser = struct.pack("<IQ", 0, len(txs)) + b"".join(struct.pack("<Q", len(t)) + t for t in txs)
        self.bufs = [ser, ser[:-7], struct.pack("<IQ", 0, 0)]
        self.bufs_want = [of.batch_digest_serialized(b) for b in self.bufs]
        # BLS: a committee of 4 keys, a vote by each over one digest
        self.bsk = [rnd.randrange(1, R_BLS).to_bytes(32, "big") for _ in range(4)]
        self.bpk = [B.keygen(sk)[1] for sk in self.bsk]
        self.keyed_n = 0
        self.mu = threading.Lock()

    @staticmethod
    def signed(n, seed, nkeys=None):
        rnd = random.Random(seed)
        seeds = [rnd.randbytes(32) for _ in range(nkeys or n)]
        pks = [of.pubkey(s) for s in seeds]
        out = []
        for i in range(n):
            m = rnd.randbytes(32)
            k = i % len(seeds)
            out.append((pks[k], of.sign(seeds[k], m), m))
        return out

    def bls_votes(self, tag):
        """three fresh votes (signatures never seen by the engine) over one digest -> (pks, digest, sigs)"""
        d = hashlib.sha256(b"place-vote" + tag).digest()
        return self.bpk[:3], d, [B.sign(sk, d) for sk in self.bsk[:3]]

    # ---- the calls ----
    def certificate_one(self):
        return self.T.verify_certificates(self.eng, self.c, [self.cert[0]]) == self.cert_want[:1] == [0]

    def certificate_bad(self):
        return self.T.verify_certificates(self.eng, self.c, [self.cert[1]]) == self.cert_want[1:] != [0]

    def batch128(self):
        ok, bits = self.eng.verify_batch(self.batch)
        return (not ok) and [bool(b) for b in bits] == self.batch_want and \
            [i for i, b in enumerate(bits) if not b] == [77]

    def keyed_new(self):
        """a keyed batch of 128 signatures by 8 keys the engine has never seen, one forged"""
        with self.mu:
            self.keyed_n += 1
            seed = 1000 + self.keyed_n
        its = self.signed(128, seed=seed, nkeys=8)
        keys = [its[k][0] for k in range(8)]
        sigs = [it[1] for it in its]
        sigs[5] = sigs[5][:40] + bytes([sigs[5][40] ^ 1]) + sigs[5][41:]
        msgs = [it[2] for it in its]
        want = [bool(of.verify(keys[i % 8], sigs[i], msgs[i])) for i in range(128)]
        ok, bits = self.eng.verify_batch_keyed(keys, [i % 8 for i in range(128)], sigs, msgs)
        return (not ok) and [bool(b) for b in bits] == want and want.count(False) == 1

    def blake2b(self):
        return self.eng.blake2b256_many(self.msgs) == self.msgs_want

    def mixed_round(self):
        got = self.T.verify_mixed(self.eng, self.c, *self.mixed)
        return tuple(got) == self.mixed_want and self.mixed_want[1][1] != 0 and \
            all(x == 0 for x in self.mixed_want[0] + self.mixed_want[2])

    def serialized(self):
        got = self.eng.batch_digest_serialized(self.bufs)
        return got == self.bufs_want and self.bufs_want[1][1] >= 0 and self.bufs_want[0][1] == -1

    def bls_verify(self, pk, msg, sig):
        return self.bls.verify(pk, msg, sig) == (0 if B.verify(pk, msg, sig) == 0 else 1)

    def bls_aggregate(self, sigs):
        rc, agg, _ = self.bls.aggregate(sigs)
        wrc, wagg = B.aggregate(sigs)
        return rc == 0 and wrc == 0 and agg == wagg


def ed_ranges(eng):
    return [eng.device_counters(ED, i)["ranges"] for i in range(eng.device_count)]


def counters(eng, engine, key):
    nd = eng.device_counters(engine, 0)["devices"]
    return [eng.device_counters(engine, i)[key] for i in range(nd)]


def delta(a, b):
    return [y - x for x, y in zip(a, b)]


def staged_64(eng, seed, device_index):
    its = Shapes.signed(64, seed=seed)
    from narwhal_amd import _lib
    return eng.stage(*_lib.soa(its), device_index=device_index)


def part_hold(out):
    import narwhal_amd
    eng = narwhal_amd.Engine(device=None, n_devices=0)
    sh = Shapes(eng)
    ck, placed = out["checks"], out["placed"]
    c0 = eng.device_counters(ED, 0)
    b0 = eng.device_counters(BLS, 0)
    ck["three_device_objects_each"] = eng.device_count == 3 and c0["devices"] == 3 and b0["devices"] == 3 and \
        len(c0) == 10 and len(b0) == 6 and c0["ordinal"] == eng.lib.nwv_device_ordinal(eng._h, 0)
    # the first call on the idle context registers the committee on every device and runs on device 0
    r0 = ed_ranges(eng)
    ck["idle_certificate_ok"] = sh.certificate_one()
    ck["idle_call_on_device_0"] = delta(r0, ed_ranges(eng)) == [1, 0, 0]
    st_a, st_b = staged_64(eng, 31, 0), staged_64(eng, 32, 1)

    def three_steps(name, call, extra=None, exact=True):
        """device 0 held -> device 1; devices 0 and 1 held -> device 2; both synced -> device 0;
        extra(): a per-device figure that must move on the call's device alone (by 1 when exact)"""
        want = ([0, 1, 0], [0, 0, 1], [1, 0, 0])
        seen = []
        for step in range(3):
            if step == 0:
                st_a.run(mode=1)  # runs, not synced: one outstanding range on device 0
            elif step == 1:
                st_b.run(mode=1)
            else:
                st_a.sync()
                st_b.sync()
            before = ed_ranges(eng)
            x0 = extra() if extra else None
            ok = call()
            d = delta(before, ed_ranges(eng))
            seen.append(d)
            ck[f"{name}_oracle_step{step}"] = bool(ok)
            ck[f"{name}_device_step{step}"] = d == want[step]
            if extra:
                dx = delta(x0, extra())
                ck[f"{name}_extra_step{step}"] = (dx if exact else [int(v > 0) for v in dx]) == want[step] and \
                    min(dx) >= 0
        placed[name] = seen
        ck[f"{name}_nothing_outstanding"] = counters(eng, ED, "outstanding") == [0, 0, 0]

    # the certificate also counts on its device's one-launch path: registration reached every
    # device's comb tables
    three_steps("certificate", sh.certificate_one, lambda: counters(eng, ED, "tiny"))
    three_steps("certificate_bad", sh.certificate_bad, lambda: counters(eng, ED, "tiny"))
    three_steps("batch128", sh.batch128)
    # keys never seen before fill the key cache of the device the call ran on, and no other
    three_steps("keyed_new", sh.keyed_new, lambda: [eng.keycache_stats(i)["used"] for i in range(3)], exact=False)
    three_steps("blake2b", sh.blake2b)
    three_steps("mixed", sh.mixed_round)
    three_steps("serialized", sh.serialized)
    ck["staged_batches_accept"] = st_a.fetch()[0] and st_b.fetch()[0]

    # BLS, with device 0 held (both engines see one load per device)
    st_a.run(mode=1)
    pks, d, sigs = sh.bls_votes(b"hold")
    b_before = counters(eng, BLS, "ranges")
    ck["bls_verify_valid"] = all(sh.bls_verify(pk, d, sg) for pk, sg in zip(pks, sigs))
    ck["bls_verify_forged"] = sh.bls_verify(pks[0], d + b"!", sigs[0]) and B.verify(pks[0], d + b"!", sigs[0]) != 0
    placed["bls_verify_held"] = delta(b_before, counters(eng, BLS, "ranges"))
    ck["bls_verify_on_device_1"] = placed["bls_verify_held"] == [0, 4, 0]
    st_a.sync()
    ck["bls_released"] = counters(eng, BLS, "outstanding") == [0, 0, 0]
    # the three votes were verified on device 1: their aggregate follows them there, hold or no hold
    b_before = counters(eng, BLS, "ranges")
    ck["bls_aggregate_equal"] = sh.bls_aggregate(sigs)
    placed["bls_aggregate_verified"] = delta(b_before, counters(eng, BLS, "ranges"))
    ck["bls_aggregate_on_device_1"] = placed["bls_aggregate_verified"] == [0, 1, 0]
    # signatures never verified, idle context: device 0
    _, _, fresh = sh.bls_votes(b"fresh")
    b_before = counters(eng, BLS, "ranges")
    ck["bls_aggregate_fresh_equal"] = sh.bls_aggregate(fresh)
    placed["bls_aggregate_fresh"] = delta(b_before, counters(eng, BLS, "ranges"))
    ck["bls_aggregate_fresh_on_device_0"] = placed["bls_aggregate_fresh"] == [1, 0, 0]
    ck["peak_is_one_per_device"] = counters(eng, ED, "peak") == [1, 1, 1] == counters(eng, BLS, "peak")
    st_a.free()
    st_b.free()
    eng.close()


def part_rotate(out):
    import narwhal_amd
    eng = narwhal_amd.Engine(device=None, n_devices=0)
    ck = out["checks"]
    its = Shapes.signed(128, seed=9)
    for i in (63, 64, 127):
        p, sg, m = its[i]
        its[i] = (p, sg[:44] + bytes([sg[44] ^ 0x04]) + sg[45:], m)
    want = [bool(of.verify(*it)) for it in its]
    ck["oracle_bad_set"] = [i for i, w in enumerate(want) if not w] == [63, 64, 127]
    r0 = ed_ranges(eng)
    for k in range(3):
        ok, bits = eng.verify_batch(its)
        ck[f"bits_equal_call{k}"] = (not ok) and [bool(b) for b in bits] == want
        ck[f"bad_set_exact_call{k}"] = [i for i, b in enumerate(bits) if not b] == [63, 64, 127]
    out["ranges"] = delta(r0, ed_ranges(eng))
    out["items"] = [eng.device_counters(ED, i)["items"] for i in range(3)]
    ck["nothing_outstanding"] = counters(eng, ED, "outstanding") == [0, 0, 0]
    eng.close()


def part_threads(out):
    import narwhal_amd
    eng = narwhal_amd.Engine(device=None, n_devices=0)
    sh = Shapes(eng)
    ck = out["checks"]
    ck["warm_up"] = sh.certificate_one()  # the committee registered before the threads start
    pks, d, sigs = sh.bls_votes(b"threads")
    n_threads, n_calls = 6, 12
    ed_calls = [sh.certificate_one, sh.batch128, sh.keyed_new, sh.blake2b, sh.mixed_round, sh.serialized]
    bls_calls = [lambda: sh.bls_verify(pks[0], d, sigs[0]), lambda: sh.bls_verify(pks[1], d + b"!", sigs[1]),
                 lambda: sh.bls_aggregate(sigs)]
    plan = []  # per thread: (engine, call), twelve each, every shape in every thread
    for t in range(n_threads):
        rnd = random.Random(600 + t)
        calls = [(ED, f) for f in ed_calls] + [(BLS, f) for f in bls_calls]
        calls += [rnd.choice(calls) for _ in range(n_calls - len(calls))]
        rnd.shuffle(calls)
        plan.append(calls)
    e0, b0 = counters(eng, ED, "ranges"), counters(eng, BLS, "ranges")
    barrier = threading.Barrier(n_threads)
    bad, errs = [], []

    def work(t):
        try:
            barrier.wait()
            for k, (_, f) in enumerate(plan[t]):
                if not f():
                    bad.append((t, k))
        except Exception as e:  # noqa: BLE001  (reported through the checks)
            errs.append(repr(e))

    th = [threading.Thread(target=work, args=(t,)) for t in range(n_threads)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    out["errors"], out["mismatches"] = errs, bad
    ck["every_result_equals_the_oracle"] = not bad and not errs
    for engine, name, base in ((ED, "ed25519", e0), (BLS, "bls", b0)):
        issued = sum(1 for calls in plan for e, _ in calls if e == engine)
        got = delta(base, counters(eng, engine, "ranges"))
        out[f"{name}_distribution"] = got  # for the record: depends on timing
        out[f"{name}_peak"] = counters(eng, engine, "peak")
        ck[f"{name}_ranges_sum_to_calls"] = sum(got) == issued
        ck[f"{name}_nothing_outstanding"] = counters(eng, engine, "outstanding") == [0, 0, 0]
        ck[f"{name}_peak_at_most_threads"] = max(out[f"{name}_peak"]) >= 1 and \
            all(p <= n_threads for p in out[f"{name}_peak"])
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["hold", "rotate", "threads"], required=True)
    a = ap.parse_args()
    out = {"part": a.part, "place": os.environ.get("NWV_PLACE", "load"), "checks": {}, "placed": {}}
    {"hold": part_hold, "rotate": part_rotate, "threads": part_threads}[a.part](out)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
