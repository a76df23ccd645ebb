"""Child process of tests/test_gpu_bls_apk_ring.py.  NWV_BLS_DEVICE_REPLICAS is read once per
process, so that configuration runs in a process of its own; every other scenario needs only a
context of its own (the ring's size and a context's flags are fixed per context), and the scenarios
named on the command line run one after another, each on a fresh engine, one JSON object out.
Expected statuses come from the oracle (bls_ffi.fast_aggregate_verify) or, for the types layer, from
oracle/narwhal_types.py with the BLS oracle deciding every signature check; the ring's part in a
call is read from nwv_bls_last_apk."""
import json
import os
import random
import sys
import threading
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import bls_ffi as B  # noqa: E402

r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


class Rig:
    """n_reg registered keys and one stray key (index n_reg) that is never registered"""

    def __init__(self, bls, seed, n_reg=4, register=True):
        self.bls = bls
        self.rnd = random.Random(seed)
        self.sks = [self.rnd.randrange(1, r).to_bytes(32, "big") for _ in range(n_reg + 1)]
        self.keys = bls.keygen(self.sks)
        self.sk_of = dict(zip(self.keys, self.sks))
        self.stray = n_reg
        if register:
            bls.register_keys(self.keys[:n_reg])

    def msg(self):
        return self.rnd.randbytes(32)

    def item(self, who, m):
        """a valid item: the aggregate of who's signatures over m"""
        sigs = self.bls.sign([self.sks[k] for k in who], [m] * len(who))
        rc, agg = B.aggregate(sigs)
        assert rc == 0
        return agg, list(who), m

    def run(self, items, keys=None):
        """-> the engine's statuses, the oracle's, the ring's counters, the call's path"""
        keys = keys or self.keys
        got = self.bls.verify_many(keys, [i[0] for i in items], [i[1] for i in items], [i[2] for i in items])
        want = [int(B.fast_aggregate_verify(s, [keys[k] for k in ks], m)) for s, ks, m in items]
        a = self.bls.last_apk()
        return {"got": [int(x) for x in got], "want": want,
                "apk": [a["hits"], a["missed"], a["noted"], a["published"]],
                "path": int(self.bls.lib.nwv_bls_last_path(self.bls._h)), "stats": list(self.bls.apk_ring_stats())}

    def warm(self, who):
        """a set brought to a hit: noted, filled, hit (three valid certificates)"""
        return [self.run([self.item(who, self.msg())]) for _ in range(3)]


def sc_default_off(bls):
    out = {"size_fresh": bls.apk_ring()}
    rig = Rig(bls, 101)
    it = rig.item([0, 1, 2], rig.msg())
    out["runs"] = [rig.run([it]) for _ in range(3)]
    out["size_after"] = bls.apk_ring()
    # the setting itself: on, the same size again, another size refused, too large refused, off
    bls.set_apk_ring(8)
    out["size_on"] = bls.apk_ring()
    bls.set_apk_ring(8)
    for name, slots in (("resize_refused", 16), ("too_large_refused", 4097)):
        try:
            bls.set_apk_ring(slots)
            out[name] = False
        except Exception:
            out[name] = True
    out["on"] = [rig.run([it]) for _ in range(3)]
    bls.set_apk_ring(0)
    out["size_off_again"] = bls.apk_ring()
    out["off_again"] = rig.run([it])
    bls.set_apk_ring(8)                              # (off and on again: the slots stay)
    out["on_again"] = rig.run([it])
    return out


def sc_noted_filled_hit(bls):
    bls.set_apk_ring(8)
    rig = Rig(bls, 102)
    it = rig.item([0, 1, 2], rig.msg())
    return {"runs": [rig.run([it]) for _ in range(3)]}


def sc_held_set(bls):
    """a held set {0, 1, 2} of a committee of four, then every near miss"""
    bls.set_apk_ring(8)
    rig = Rig(bls, 103)
    out = {"warm": rig.warm([0, 1, 2])}
    m = rig.msg()
    good = rig.item([0, 1, 2], m)
    other = rig.item([1, 2, 3], m)
    out["forged"] = rig.run([(other[0], [0, 1, 2], m)])
    out["wrong_message"] = rig.run([(good[0], [0, 1, 2], rig.msg())])
    out["key_dropped"] = rig.run([(good[0], [0, 1], m)])             # the held set's aggregate, one key short
    out["key_dropped_valid"] = rig.run([rig.item([0, 1], m)])
    out["key_added"] = rig.run([(good[0], [0, 1, 2, 3], m)])
    out["key_added_valid"] = rig.run([rig.item([0, 1, 2, 3], m)])
    out["permuted"] = rig.run([(good[0], [2, 0, 1], m)])
    # [a, a, b] against [a, b]: bring [0, 1] to a hit, then present [0, 0, 1] both ways
    out["warm_ab"] = rig.warm([0, 1])
    ab, aab = rig.item([0, 1], m), rig.item([0, 0, 1], m)
    out["aab_with_ab_aggregate"] = rig.run([(ab[0], [0, 0, 1], m)])
    out["aab_valid"] = rig.run([aab])
    out["ab_with_aab_aggregate"] = rig.run([(aab[0], [1, 0], m)])
    out["ab_valid"] = rig.run([ab])
    return out


def sc_gate(bls):
    bls.set_apk_ring(8)
    rig = Rig(bls, 104)
    m = rig.msg()
    forged = (rig.item([1, 2, 3], m)[0], [0, 1, 2], m)
    out = {"runs": [rig.run([forged]) for _ in range(5)]}
    out["then_valid"] = rig.run([rig.item([0, 1, 2], m)])
    return out


def sc_identity(bls):
    """keys of sk and r - sk: an identity key sum, PK_INFINITY every time, never held"""
    bls.set_apk_ring(8)
    rnd = random.Random(105)
    sk = rnd.randrange(1, r)
    sks = [sk.to_bytes(32, "big"), (r - sk).to_bytes(32, "big")]
    keys = bls.keygen(sks)
    bls.register_keys(keys)
    m = rnd.randbytes(32)
    rc, agg = B.aggregate(bls.sign(sks, [m, m]))
    runs = []
    for _ in range(4):
        got = bls.verify_many(keys, [agg], [[0, 1]], [m])
        a = bls.last_apk()
        runs.append({"got": [int(x) for x in got], "want": [int(B.fast_aggregate_verify(agg, keys, m))],
                     "apk": [a["hits"], a["missed"], a["noted"], a["published"]], "stats": list(bls.apk_ring_stats())})
    return {"runs": runs}


def sc_eviction(bls):
    """capacity 2, three recurring sets A, B, C: each brought to a hit in turn (C's fill takes A's
    slot), then C, B hit and A is found gone"""
    bls.set_apk_ring(2)
    rig = Rig(bls, 106)
    sets = {"A": [0, 1, 2], "B": [1, 2, 3], "C": [0, 2, 3]}
    out = {"warm": {k: rig.warm(v) for k, v in sets.items()}}
    out["after"] = {k: rig.run([rig.item(sets[k], rig.msg())]) for k in ("C", "B", "A")}
    return out


def sc_epoch(bls):
    bls.set_apk_ring(8)
    rig = Rig(bls, 107, register=False)
    k = rig.keys[:4]
    bls.register_keys(k)
    out = {"warm": rig.warm([0, 1, 2])}
    bls.reset_keys()
    out["stats_after_reset"] = list(bls.apk_ring_stats())
    bls.register_keys(k[::-1])                       # k3, k2, k1 now sit in cache slots 0, 1, 2
    m = rig.msg()
    out["k3k2k1"] = rig.run([rig.item([3, 2, 1], m)])
    out["k0k1k2"] = rig.run([rig.item([0, 1, 2], m)])
    out["swapped"] = rig.run([(rig.item([0, 1, 2], m)[0], [3, 2, 1], m)])
    return out


def sc_real_size(bls):
    bls.set_apk_ring(8)
    rig = Rig(bls, 108, n_reg=100)
    who = sorted(rig.rnd.sample(range(100), 67))
    out = {"warm": rig.warm(who)}
    m = rig.msg()
    good = rig.item(who, m)
    other = rig.item(who[:66] + [next(j for j in range(100) if j not in who)], m)
    out["valid"] = rig.run([good])
    out["forged"] = rig.run([(other[0], who, m)])
    return out


def sc_with_msg_ring(bls):
    bls.set_apk_ring(8)
    bls.set_msg_ring(16)
    rig = Rig(bls, 109)
    m = rig.msg()
    good = rig.item([0, 1, 2], m)
    runs = []
    for _ in range(3):
        x = rig.run([good])
        x["msgs"] = bls.last_msgs()
        runs.append(x)
    forged = rig.run([(rig.item([1, 2, 3], m)[0], [0, 1, 2], m)])
    forged["msgs"] = bls.last_msgs()
    return {"runs": runs, "forged": forged}


def sc_types(bls):
    """a 4-node committee: four headers, six votes and six certificates over two signer sets (one
    certificate carries another's aggregate), through nwv_bls_verify_mixed_many and
    nwv_bls_validate_certificates, three times"""
    import copy
    import test_gpu_types_bls as TB
    from narwhal_amd import types as T
    eng = bls.eng
    # (4,096 filter entries: the two sets, sighted in turn within one call, share one with
    # probability 1 / 4,096 under the process's hash salt, and would then keep each other out)
    bls.set_apk_ring(1024)
    rnd = random.Random(110)
    n = 4
    sks = [rnd.randrange(1, r).to_bytes(32, "big") for _ in range(n)]
    sk_of = dict(zip(bls.keygen(sks), sks))
    com = T.Committee(sorted(sk_of), [1] * n, 0, [[0, 1, 2, 3]] * n)
    q = com.quorum_threshold()
    parents = T.bls_certificate_digests(eng, T.BlsCertificate.genesis(com))
    # six headers by the four authors (rounds 1 and 2), so six certificates
    headers = [T.Header(author=com.keys[a % n], round=1 + a // n, epoch=0, payload=[(rnd.randbytes(32), a % 4)],
                        parents=list(parents), signature=bytes(48)) for a in range(6)]
    for h, d in zip(headers, T.bls_header_digests(eng, headers)):
        h.id = d
    for h, s in zip(headers, bls.sign([sk_of[h.author] for h in headers], [h.id for h in headers])):
        h.signature = s
    sets = [[0, 1, 2], [1, 2, 3]]
    voters = [sets[a % 2] for a in range(6)]
    votes = [T.Vote(headers[a].id, headers[a].round, 0, headers[a].author, com.keys[v], bytes(48))
             for a in range(6) for v in voters[a]]
    for v, s in zip(votes, bls.sign([sk_of[v.author] for v in votes], T.bls_vote_digests(eng, votes))):
        v.signature = s
    certs = [T.BlsCertificate.new(eng, com, headers[a], [(v.author, v.signature) for v in votes[a * q:(a + 1) * q]])
             for a in range(6)]
    certs[4] = copy.deepcopy(certs[4])
    certs[4].aggregated_signature = certs[2].aggregated_signature     # the invalid one
    env = {"com": com}
    some_votes = votes[::3]
    want = [list(x) for x in TB._oracle_codes(env, headers[:4], some_votes, certs)]
    out = {"q": q, "signed": [list(c.signed_authorities) for c in certs], "want": want, "calls": []}
    for _ in range(3):
        got = T.bls_verify_mixed(eng, com, headers[:4], some_votes, certs)
        a = bls.last_apk()
        ok, bad = T.bls_validate_certificates(eng, com, certs)
        b = bls.last_apk()
        out["calls"].append({"got": [list(x) for x in got], "apk": [a[k] for k in ("hits", "missed", "noted", "published")],
                             "validate": [bool(ok), [int(i) for i in bad]],
                             "validate_apk": [b[k] for k in ("hits", "missed", "noted", "published")]})
    out["stats"] = list(bls.apk_ring_stats())
    return out


def sc_threads(bls):
    """four threads on a ring of two, three sets, twenty one-item calls a thread"""
    bls.set_apk_ring(2)
    rig = Rig(bls, 111)
    sets = [[0, 1, 2], [1, 2, 3], [0, 2, 3]]
    pool = []
    for j in range(6):
        m = rig.msg()
        it = rig.item(sets[j % 3], m)
        pool.append(it)
        pool.append((it[0], sets[(j + 1) % 3], m))          # the aggregate under another set
    want = [int(B.fast_aggregate_verify(s, [rig.keys[k] for k in ks], m)) for s, ks, m in pool]
    bad, calls, errors, hits = [], [0] * 4, [], [0] * 4

    def worker(t):
        rnd = random.Random(1100 + t)
        try:
            for c in range(20):
                p = rnd.randrange(len(pool))
                s, ks, m = pool[p]
                ks = list(ks)
                rnd.shuffle(ks)
                got = bls.verify_many(rig.keys, [s], [ks], [m])
                if [int(x) for x in got] != [want[p]]:
                    bad.append((t, c, p, [int(x) for x in got]))
                a = bls.last_apk()
                if a["hits"] + a["missed"] != 1:
                    bad.append((t, c, "counters", a))
                hits[t] += a["hits"]
                calls[t] += 1
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    return {"bad": bad, "errors": errors, "calls": calls, "hits": hits, "stats": list(bls.apk_ring_stats()),
            "statuses_seen": sorted(set(want))}


def sc_replicas(bls):
    """two BLS device objects on one GPU: a staged Ed25519 batch that has run and is not synced
    holds its device, so the same certificate goes three times to each device in turn; each ring
    fills on its own sightings"""
    import place_gpu_check as P
    eng = bls.eng
    bls.set_apk_ring(8)
    rig = Rig(bls, 112)
    it = rig.item([0, 1, 2], rig.msg())
    out = {"devices": eng.device_counters(P.BLS, 0)["devices"], "runs": [], "placed": []}

    def three():
        for _ in range(3):
            before = P.counters(eng, P.BLS, "ranges")
            out["runs"].append(rig.run([it]))
            out["placed"].append(P.delta(before, P.counters(eng, P.BLS, "ranges")))

    three()                                          # an idle context: the first device object
    st = P.staged_64(eng, 31, 0)
    st.run(mode=1)                                   # device object 0 is loaded: the second serves
    three()
    st.sync()
    out["staged_ok"] = bool(st.fetch()[0])
    st.free()
    three()                                          # idle again: the first, whose ring still holds the set
    return out


def sc_many_keys(bls):
    """a call whose key table names more uncached keys than the key cache has slots (65,536): its
    scratch entries' indices run past twice the cache's size and must stay clear of the ring's index
    range.  A hit item beside an item signed by the table's last key, an outsider's"""
    bls.set_apk_ring(8)
    rig = Rig(bls, 114)
    out = {"warm": rig.warm([0, 1, 2])}
    strays = [bytes([0x80 | (i & 0x1f)]) + i.to_bytes(4, "big") + bytes(91) for i in range(66000)]   # undecodable
    keys = rig.keys[:4] + strays + [rig.keys[rig.stray]]
    last = len(keys) - 1
    m = rig.msg()
    items = [rig.item([0, 1, 2], m), (rig.item([rig.stray], m)[0], [last], m), (rig.item([0], m)[0], [4 + 65600], m),
             (rig.item([1, 2, 3], m)[0], [0, 1, 2], m)]
    out["n_keys"] = len(keys)
    out["run"] = rig.run(items, keys)
    return out


def sc_ignored(bls, what):
    """a path that does not use the ring, with the ring on: the set three times"""
    bls.set_apk_ring(8)
    if what == "unregistered":
        rig = Rig(bls, 113)
        it = rig.item([0, 1, rig.stray], rig.msg())
        return {"size": bls.apk_ring(), "runs": [rig.run([it]) for _ in range(3)]}
    rig = Rig(bls, 113)
    it = rig.item([0, 1, 2], rig.msg())
    if what == "n1025":
        bad = (it[0], [1, 2, 3], it[2])
        items = [it] * 1024 + [bad]
        want = [int(B.fast_aggregate_verify(s, [rig.keys[k] for k in ks], m)) for s, ks, m in (it, bad)]
        runs = []
        for _ in range(2):
            got = bls.verify_many(rig.keys, [i[0] for i in items], [i[1] for i in items], [i[2] for i in items])
            a = bls.last_apk()
            runs.append({"got": sorted(set(int(x) for x in got[:1024])) + [int(got[1024])], "want": want,
                         "apk": [a["hits"], a["missed"], a["noted"], a["published"]],
                         "stats": list(bls.apk_ring_stats())})
        return {"size": bls.apk_ring(), "runs": runs}
    return {"size": bls.apk_ring(), "runs": [rig.run([it]) for _ in range(3)]}


def main():
    import narwhal_amd
    from narwhal_amd import _lib
    from narwhal_amd.bls import Bls
    flags_of = {"batch": _lib.NWV_FLAG_BLS_BATCH, "per_item": _lib.NWV_FLAG_BLS_PER_ITEM,
                "no_keycache": _lib.NWV_FLAG_NO_KEYCACHE}
    out = {}
    for name in sys.argv[1:]:
        scenario, _, arg = name.partition(":")
        try:
            if scenario == "replicas":
                e = narwhal_amd.Engine(device=None, n_devices=0)
            else:
                e = narwhal_amd.Engine(device=0, flags=flags_of.get(arg, 0))
            bls = Bls(e)
            out[name] = sc_ignored(bls, arg) if scenario == "ignored" else globals()["sc_" + scenario](bls)
            e.close()
        except Exception:  # noqa: BLE001
            # (nothing more runs on the GPU after a failure: the scenarios left are reported as not run)
            out[name] = {"error": traceback.format_exc()[-3000:]}
            break
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
