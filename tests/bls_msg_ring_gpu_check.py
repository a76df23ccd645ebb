"""Child process of tests/test_gpu_bls_msg_ring.py.  NWV_BLS_WAVE_MAX, NWV_BLS_DEVICE_REPLICAS and
NWV_DEVICE_REPLICAS are read once per process and a context's flags are fixed at nwv_init, so
every configuration runs in a fresh process: the parent sets the environment, this runs one
scenario (argv[1]) and prints one JSON line.  Expected statuses come from the oracle
(bls_ffi.fast_aggregate_verify) or, for the types layer, from oracle/narwhal_types.py with the BLS
oracle deciding every signature check; the ring's part in a call is read from nwv_bls_last_msgs."""
import json
import os
import random
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import bls_cases as C  # noqa: E402
import bls_ffi as B  # noqa: E402

r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
ZERO = {"hits_copied": 0, "hits_chained": 0, "computed": 0, "published": 0, "ahead_published": 0}


def cnt(**kw):
    return dict(ZERO, **kw)


class Rig:
    """n_reg registered keys and one stray key (index n_reg) that is never registered"""

    def __init__(self, bls, seed, n_reg=10):
        self.bls = bls
        self.rnd = random.Random(seed)
        self.sks = [self.rnd.randrange(1, r).to_bytes(32, "big") for _ in range(n_reg + 1)]
        self.keys = bls.keygen(self.sks)
        self.stray = n_reg
        bls.register_keys(self.keys[:n_reg])

    def msg(self):
        return self.rnd.randbytes(32)

    def item(self, who, m, dst=None):
        """a valid item: the aggregate of who's signatures over m"""
        sigs = self.bls.sign([self.sks[k] for k in who], [m] * len(who), dst=dst)
        rc, agg = B.aggregate(sigs)
        assert rc == 0
        return agg, list(who), m

    def run(self, items, keys=None, dst=None, ahead=None, gates=None):
        """-> {"got", "want", "msgs"}: the engine's statuses, the oracle's, the ring's counters"""
        keys = keys or self.keys
        a = ([i[0] for i in items], [i[1] for i in items], [i[2] for i in items])
        if ahead is None:
            got = self.bls.verify_many(keys, *a, dst=dst)
        else:
            got = self.bls.verify_many_ahead(keys, *a, ahead, gates, dst=dst)
        want = [int(B.fast_aggregate_verify(s, [keys[k] for k in ks], m, **({"dst": dst} if dst else {})))
                for s, ks, m in items]
        return {"got": [int(x) for x in got], "want": want, "msgs": self.bls.last_msgs()}


def forge(item):
    s, ks, m = item
    return s, ks, m[:-1] + bytes([m[-1] ^ 1])


def sc_default_off(bls):
    out = {"size_fresh": bls.msg_ring()}
    rig = Rig(bls, 81)
    it = rig.item([0], rig.msg())
    out["verify"] = rig.run([it])
    bls.hash_ahead([it[2], rig.msg()])
    out["after_hash_ahead"] = rig.run([it])
    out["stats"] = list(bls.msg_ring_stats())
    out["size_after"] = bls.msg_ring()
    # the setting itself: on, the same size again, another size refused, off
    bls.set_msg_ring(16)
    out["size_on"] = bls.msg_ring()
    bls.set_msg_ring(16)
    try:
        bls.set_msg_ring(32)
        out["resize_refused"] = False
    except Exception:
        out["resize_refused"] = True
    try:
        bls.set_msg_ring(65537)
        out["too_large_refused"] = False
    except Exception:
        out["too_large_refused"] = True
    out["on"] = [rig.run([it]), rig.run([it])]
    bls.set_msg_ring(0)
    out["size_off_again"] = bls.msg_ring()
    out["off_again"] = rig.run([it])
    return out


def sc_hit_miss(bls):
    bls.set_msg_ring(64)
    rig = Rig(bls, 82)
    m = rig.msg()
    a, b = rig.item([0], m), rig.item([1], m)
    out = {"first": rig.run([a]), "second": rig.run([a])}
    wrong = (b[0], [0], m)                           # key 1's signature presented as key 0's
    out["forged_over_cached"] = rig.run([wrong])
    out["other_key"] = rig.run([b])
    dst2 = b"NWV-TEST-DST-V01"
    out["other_dst_valid"] = rig.run([rig.item([0], m, dst=dst2)], dst=dst2)
    out["other_dst_again"] = rig.run([(a[0], [0], m)], dst=dst2)   # the first DST's signature: the oracle rejects
    out["long_message"] = [rig.run([rig.item([0], bytes(65))]), rig.run([rig.item([0], bytes(65))])]
    return out


def sc_forms(bls):
    bls.set_msg_ring(64)
    rig = Rig(bls, 83, n_reg=100)
    s = rig.stray
    out = {}
    m1 = rig.msg()
    out["registered_first"] = rig.run([rig.item([3], m1)])
    out["then_unregistered"] = rig.run([rig.item([s], m1)])        # a chain hit
    m2 = rig.msg()
    out["unregistered_first"] = rig.run([rig.item([s], m2)])
    out["then_registered"] = rig.run([rig.item([4], m2)])          # a copied hit
    m3 = rig.msg()
    bls.hash_ahead([m3])
    who = sorted(rig.rnd.sample(range(100), 67))
    out["aggregate_67_of_100"] = rig.run([rig.item(who, m3)])      # a copied hit
    out["aggregate_with_stranger"] = rig.run([rig.item(who[:66] + [s], m3)])   # a chain hit
    out["aggregate_forged"] = rig.run([forge(rig.item(who, m3))])
    return out


def sc_two_items(bls):
    bls.set_msg_ring(64)
    rig = Rig(bls, 84)
    m1, m2 = rig.msg(), rig.msg()
    out = {"warm": rig.run([rig.item([0], m1)])}
    out["one_cached_one_not"] = rig.run([rig.item([1], m2), rig.item([2], m1)])
    out["both_cached_mixed_forms"] = rig.run([rig.item([rig.stray], m2), rig.item([3], m1)])
    return out


def sc_duplicates(bls):
    bls.set_msg_ring(64)
    rig = Rig(bls, 85)
    m = rig.msg()
    items = [rig.item([k], m) for k in (0, 1, 2, rig.stray, 4)]
    items[2] = (items[1][0], [2], m)                 # one of them forged
    return {"cold": rig.run(items), "repeated": rig.run(items), "stats": list(bls.msg_ring_stats())}


def sc_failures(bls):
    """bls_wave_batch_gpu_check.sc_pre's items: every category that fails before the pairing
    equation beside valid items, every second valid item by the unregistered key; run twice"""
    bls.set_msg_ring(64)
    rig = Rig(bls, 86)
    keys = rig.keys + [C.not_in_g2(), C.IDENTITY_G2, C.negate_g2(rig.keys[0])]  # 11, 12, 13
    v = [rig.item([rig.stray] if i % 2 else [i % 10], rig.msg()) for i in range(12)]
    v[3] = rig.item([1, 4, 7], v[3][2])
    agg, who, d = v[0]
    bad = [(agg, [], d),                       # empty key list
           (agg, who + [11], d),               # a key outside G2
           (agg, who + [12], d),               # identity key
           (agg, [0, 13], d),                  # identity key sum
           (C.not_in_g1(), who, d),            # signature outside G1
           (C.IDENTITY_G1, who, d),            # identity signature
           ] + [(b, who, d) for b in C.bad_encodings_g1(agg)]
    items = v[:5] + bad[:5] + v[5:9] + bad[5:] + v[9:]
    return {"n": len(items), "n_bad": len(bad), "n_messages": 12,
            "first": rig.run(items, keys), "second": rig.run(items, keys), "stats": list(bls.msg_ring_stats())}


def sc_eviction(bls, cap):
    """hash_ahead of six messages into a ring of cap < 6 slots keeps the last cap of them.  The six
    verifies go newest first: a verify that misses takes the ring's oldest slot for its own
    message (a FIFO), so in the order 0..5 the first misses would push out the very entries the
    later verifies look for."""
    bls.set_msg_ring(cap)
    rig = Rig(bls, 87)
    msgs = [rig.msg() for _ in range(6)]
    items = [rig.item([k], m) for k, m in enumerate(msgs)]
    bls.hash_ahead(msgs)
    out = {"size": bls.msg_ring(), "runs": {}}
    for k in (5, 4, 3, 2, 1, 0):
        out["runs"][str(k)] = rig.run([items[k]])
    out["stats"] = list(bls.msg_ring_stats())
    return out


def sc_gate(bls):
    bls.set_msg_ring(64)
    rig = Rig(bls, 88)
    good, bad = rig.item([0], rig.msg()), forge(rig.item([1], rig.msg()))
    ahead = [rig.msg(), rig.msg(), rig.msg(), bytes(65), good[2]]
    ahead.append(ahead[0])                                         # a duplicate within the call
    gates = [0, 1, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0]
    out = {"plain": rig.run([good, bad])}
    bls.set_msg_ring(0)
    bls.set_msg_ring(64)                                           # (off and on again: the slots stay)
    out["with_ahead"] = rig.run([good, bad], ahead=ahead, gates=gates)
    out["found"] = [rig.run([rig.item([2], m)])["msgs"] for m in ahead[:3]]
    out["checks_ok"] = all(x["got"] == x["want"] for x in (out["plain"], out["with_ahead"]))
    try:
        rig.run([good], ahead=ahead[:1], gates=[1])
        out["bad_gate_refused"] = False
    except Exception:
        out["bad_gate_refused"] = True
    return out


def sc_types(bls, ring):
    """three headers (one with a forged signature) in one nwv_bls_verify_mixed_many call, then their
    certificates and two votes per header in another"""
    import copy
    import test_gpu_types_bls as TB
    from narwhal_amd import types as T
    eng = bls.eng
    if ring:
        bls.set_msg_ring(64)
    rnd = random.Random(89)
    n = 4
    sks = [rnd.randrange(1, r).to_bytes(32, "big") for _ in range(n)]
    sk_of = dict(zip(bls.keygen(sks), sks))
    com = T.Committee(sorted(sk_of), [1] * n, 0, [[0, 1, 2, 3]] * n)
    q = com.quorum_threshold()
    parents = T.bls_certificate_digests(eng, T.BlsCertificate.genesis(com))
    headers = [T.Header(author=k, round=1, epoch=0, payload=[(rnd.randbytes(32), a % 4)], parents=list(parents),
                        signature=bytes(48)) for a, k in enumerate(com.keys[:3])]
    for h, d in zip(headers, T.bls_header_digests(eng, headers)):
        h.id = d
    for h, s in zip(headers, bls.sign([sk_of[h.author] for h in headers], [h.id for h in headers])):
        h.signature = s
    voters = [[i for i in range(n) if i != a][:q] for a in range(3)]
    votes = [T.Vote(headers[a].id, 1, 0, com.keys[a], com.keys[v], bytes(48)) for a in range(3) for v in voters[a]]
    for v, s in zip(votes, bls.sign([sk_of[v.author] for v in votes], T.bls_vote_digests(eng, votes))):
        v.signature = s
    certs = [T.BlsCertificate.new(eng, com, headers[a], [(v.author, v.signature) for v in votes[a * q:(a + 1) * q]])
             for a in range(3)]
    headers[1] = copy.deepcopy(headers[1])
    headers[1].signature = headers[0].signature                    # the forged one
    env = {"com": com}
    out = {"ring": bls.msg_ring()}
    two = [votes[a * q + j] for a in range(3) for j in range(2)]
    got1 = T.bls_verify_mixed(eng, com, headers, [], [])
    out["call1"] = {"got": [list(x) for x in got1], "msgs": bls.last_msgs(),
                    "want": [list(x) for x in TB._oracle_codes(env, headers, [], [])]}
    got2 = T.bls_verify_mixed(eng, com, [], two, certs)
    out["call2"] = {"got": [list(x) for x in got2], "msgs": bls.last_msgs(),
                    "want": [list(x) for x in TB._oracle_codes(env, [], two, certs)]}
    # the forged header's certificate carries the honest signature: valid, and its digest was not hashed ahead
    out["stats"] = list(bls.msg_ring_stats())
    return out


def sc_concurrency(bls):
    """six threads, a ring of 8, overlapping sets of 12 messages, 20 one- and two-item calls each"""
    bls.set_msg_ring(8)
    rig = Rig(bls, 90)
    msgs = [rig.msg() for _ in range(12)]
    pool = []                                                       # (item, the oracle's status)
    for j, m in enumerate(msgs):
        for who in ([j % 10], [rig.stray]):
            it = rig.item(who, m)
            pool.append(it)
            pool.append(forge(it) if j % 3 == 0 else (it[0], [(who[0] + 1) % 10], m))
    want = [int(B.fast_aggregate_verify(s, [rig.keys[k] for k in ks], m)) for s, ks, m in pool]
    by_msg = {}
    for idx, it in enumerate(pool):
        by_msg.setdefault(it[2], []).append(idx)
    bad, calls, errors = [], [0] * 6, []

    def worker(t):
        rnd = random.Random(900 + t)
        mine = [msgs[(2 * t + k) % 12] for k in range(6)]           # overlaps its neighbours' sets
        try:
            for c in range(20):
                picks = [rnd.choice(by_msg[rnd.choice(mine)]) for _ in range(1 + c % 2)]
                items = [pool[p] for p in picks]
                got = bls.verify_many(rig.keys, [i[0] for i in items], [i[1] for i in items], [i[2] for i in items])
                if [int(x) for x in got] != [want[p] for p in picks]:
                    bad.append((t, c, picks, [int(x) for x in got]))
                m = bls.last_msgs()
                if m["hits_copied"] + m["hits_chained"] + m["computed"] != len(items):
                    bad.append((t, c, "counters", m))
                calls[t] += 1
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(6)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    return {"bad": bad, "errors": errors, "calls": calls, "stats": list(bls.msg_ring_stats()),
            "statuses_seen": sorted(set(want))}


def sc_replicas(bls):
    """three BLS device objects on one GPU: hash_ahead fills every ring, so a verify hits wherever
    placement sends it (a staged Ed25519 batch that has run and is not synced holds its device)"""
    import place_gpu_check as P
    eng = bls.eng
    bls.set_msg_ring(16)
    rig = Rig(bls, 91)
    msgs = [rig.msg() for _ in range(3)]
    items = [rig.item([k], m) for k, m in enumerate(msgs)]
    bls.hash_ahead(msgs)
    st_a, st_b = P.staged_64(eng, 31, 0), P.staged_64(eng, 32, 1)
    out = {"devices": eng.device_counters(P.BLS, 0)["devices"], "runs": [], "placed": []}
    for step in range(3):
        if step == 1:
            st_a.run(mode=1)
        elif step == 2:
            st_b.run(mode=1)
        before = P.counters(eng, P.BLS, "ranges")
        out["runs"].append(rig.run([items[step]]))
        out["placed"].append(P.delta(before, P.counters(eng, P.BLS, "ranges")))
    st_a.sync()
    st_b.sync()
    out["staged_ok"] = bool(st_a.fetch()[0] and st_b.fetch()[0])
    st_a.free()
    st_b.free()
    return out


def sc_ignored(bls):
    """a path that does not use the ring (the parent chose it: NWV_BLS_WAVE_MAX=4, or a
    NWV_FLAG_BLS_BATCH / NWV_FLAG_BLS_PER_ITEM context): six items, twice, with the ring on"""
    bls.set_msg_ring(64)
    rig = Rig(bls, 92)
    items = [rig.item([k], rig.msg()) for k in range(6)]
    items[4] = forge(items[4])
    bls.hash_ahead([items[0][2]])
    out = {"size": bls.msg_ring(), "first": rig.run(items), "second": rig.run(items), "path": bls.last_path()}
    out["with_ahead"] = rig.run(items, ahead=[rig.msg()], gates=[0])
    return out


def main():
    import narwhal_amd
    from narwhal_amd import _lib
    from narwhal_amd.bls import Bls
    scenario = sys.argv[1]
    arg = sys.argv[2] if len(sys.argv) > 2 else ""
    flags = {"batch": _lib.NWV_FLAG_BLS_BATCH, "per_item": _lib.NWV_FLAG_BLS_PER_ITEM}.get(arg, 0)
    if scenario == "replicas":
        e = narwhal_amd.Engine(device=None, n_devices=0)
    else:
        e = narwhal_amd.Engine(device=0, flags=flags)
    bls = Bls(e)
    if scenario == "eviction":
        out = sc_eviction(bls, int(arg))
    elif scenario == "types":
        out = sc_types(bls, arg == "on")
    else:
        out = globals()["sc_" + scenario](bls)
    e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
