"""Child process of tests/test_gpu_bls_key_batch.py.  The key-transposed batch check's settings
(NWV_BLS_WAVE_MAX, NWV_BLS_KEY_GROUP, NWV_BLS_KEY_GROUP_RATIO, NWV_BLS_DEVICE_REPLICAS,
NWV_BLS_SHARD_MIN) are read once per process, so every configuration runs in a fresh one: the
parent sets the environment, this runs one scenario (argv[1], with the item layout in argv[2]
where one applies) on a context with nwv_bls_set_key_batch_min(1) and prints one JSON line.  The
oracle is bls_ffi.fast_aggregate_verify."""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import bls_cases as C  # noqa: E402
import bls_ffi as B  # noqa: E402

r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
GROUP = 6


def neg_g1(sig):
    """-P of a compressed G1 point: the encoding's sign bit flipped"""
    b = bytearray(sig)
    b[0] ^= 0x20
    return bytes(b)


def oracle(keys, items):
    return [int(B.fast_aggregate_verify(s, [keys[k] for k in ks], m)) for s, ks, m in items]


def millers(who, group=GROUP):
    """sum over the groups of (distinct keys + 1), every item of `who` in the groups"""
    return sum(len({k for ks in who[lo:lo + group] for k in ks}) + 1 for lo in range(0, len(who), group))


class Rig:
    """a registered 4-key committee (keys 0..3) and one valid key that is never registered (4)"""

    def __init__(self, bls, seed):
        self.bls = bls
        self.rnd = random.Random(seed)
        self.sks = [self.rnd.randrange(1, r).to_bytes(32, "big") for _ in range(5)]
        self.keys = bls.keygen(self.sks)
        bls.register_keys(self.keys[:4])

    def who(self, n, layout):
        """onekey: one-key items over keys 0..2; certs: 3-of-4 certificates; mixed: both in turn"""
        out = []
        for i in range(n):
            if layout == "certs" or (layout == "mixed" and i % 2):
                out.append(sorted(self.rnd.sample(range(4), 3)))
            else:
                out.append([i % 3])
        return out

    def sign(self, who, msgs=None):
        msgs = msgs or [self.rnd.randbytes(32) for _ in who]
        flat = self.bls.sign([self.sks[k] for ks in who for k in ks], [m for ks, m in zip(who, msgs) for _ in ks])
        items, at = [], 0
        for ks, m in zip(who, msgs):
            rc, agg = B.aggregate(flat[at:at + len(ks)])
            assert rc == 0
            at += len(ks)
            items.append((agg, list(ks), m))
        return items

    def run(self, items, keys=None):
        keys = keys or self.keys
        got = self.bls.verify_many(keys, [i[0] for i in items], [i[1] for i in items], [i[2] for i in items])
        return {"got": [int(x) for x in got], "want": oracle(keys, items), "path": self.bls.last_path(),
                "kb": list(self.bls.last_key_batch()), "batch": list(self.bls.last_batch())}


def wrong_message(item):
    s, ks, m = item
    return (s, ks, m[:-1] + bytes([m[-1] ^ 1]))


def sc_sizes(bls, layout):
    rig = Rig(bls, 171)
    runs = {}
    for n in (1, 6, 7, 13, 23):
        who = rig.who(n, layout)
        runs[str(n)] = dict(rig.run(rig.sign(who)), millers=millers(who))
    return {"runs": runs}


def sc_forgery(bls, layout):
    """30 items, five groups of six; item 14 (the third group) signs another message"""
    rig = Rig(bls, 172)
    items = rig.sign(rig.who(30, layout))
    items[14] = wrong_message(items[14])
    return rig.run(items)


def sc_cancel(bls, layout):
    """sig_a + D and sig_b - D in the second group"""
    rig = Rig(bls, 173)
    items = rig.sign(rig.who(16, layout))
    a, b, D = 7, 10, items[15][0]
    rc1, sa = B.aggregate([items[a][0], D])
    rc2, sb = B.aggregate([items[b][0], neg_g1(D)])
    assert rc1 == 0 and rc2 == 0
    same_sum = B.aggregate([sa, sb])[1] == B.aggregate([items[a][0], items[b][0]])[1]
    items[a] = (sa,) + items[a][1:]
    items[b] = (sb,) + items[b][1:]
    return dict(rig.run(items), a=a, b=b, same_sum=same_sum)


def sc_swap(bls, layout):
    """items 7 and 9 (one group) on one message: 7 carries key 1's signature and names key 2, 9 the
    reverse.  sig_7 + sig_9 verifies under the two keys' sum, so the product without coefficients is 1"""
    rig = Rig(bls, 174)
    items = rig.sign(rig.who(14, layout))
    m = rig.rnd.randbytes(32)
    s1, s2 = rig.bls.sign([rig.sks[1], rig.sks[2]], [m, m])
    items[7] = (s1, [2], m)
    items[9] = (s2, [1], m)
    unweighted = int(B.fast_aggregate_verify(B.aggregate([s1, s2])[1], [rig.keys[2], rig.keys[1]], m))
    return dict(rig.run(items), unweighted=unweighted)


def sc_multi(bls, layout):
    """an item that names key 1 twice (its signature is by 2 sk_1: the aggregate of two signatures
    by key 1), key 0 on four different messages, one message signed by keys 0, 1 and 2 in three items"""
    rig = Rig(bls, 175)
    shared = rig.rnd.randbytes(32)
    who = [[1, 1], [0], [0], [2, 1, 1, 3], [0], [0], [0], [1], [2], [0, 0, 0]]
    msgs = [rig.rnd.randbytes(32) for _ in who]
    for i in (6, 7, 8):
        msgs[i] = shared
    return dict(rig.run(rig.sign(who, msgs)), millers=millers(who))


def sc_outside(bls, layout):
    """items that stay out of the groups beside valid ones.  Keys: 5 = -key 3, registered (so [3, 5]
    is an identity key sum of cached keys), 6 outside G2, 4 valid and not registered.  Key 3 is
    named by stay-out items only."""
    rig = Rig(bls, 176)
    keys = rig.keys + [C.negate_g2(rig.keys[3]), C.not_in_g2()]
    bls.register_keys([keys[5]])
    v = rig.sign(rig.who(14, "onekey"))                # keys 0..2 only
    agg, who, d = v[0]
    stray = rig.sign([[4], [0, 4]])                    # valid, but key 4 is not in the cache
    bad = [(C.bad_encodings_g1(agg)[0], who, d),       # a bad encoding
           (C.not_in_g1(), who, d),                    # a signature outside G1
           (C.IDENTITY_G1, [3], d),                    # the identity signature
           (agg, [], d),                               # an empty key list
           (agg, [3, 5], d),                           # an identity key sum
           stray[0], stray[1],                         # an unregistered but valid key
           (agg, who + [6], d),                        # an unregistered key outside G2
           (v[1][0], [3], v[1][2])]                    # (a wrong key, in no cache trouble: it is grouped)
    items = v[:3] + bad[:4] + v[3:9] + bad[4:8] + v[9:]
    inside = [i[1] for i in items if i in v]
    out = dict(rig.run(items, keys), n_valid=len(v) + 2, millers=millers(inside))
    # the same call with the wrong-key item in: key 3 gets an entry, and its group rejects
    items2 = items + [bad[8]]
    out["with_wrong_key"] = rig.run(items2, keys)
    return out


def sc_sharded(bls, layout):
    """three shares of ten items (NWV_BLS_DEVICE_REPLICAS=3, NWV_BLS_SHARD_MIN=8), a forgery in each"""
    rig = Rig(bls, 177)
    items = rig.sign(rig.who(30, "mixed"))
    for k in (3, 14, 27):
        items[k] = wrong_message(items[k])
    return rig.run(items)


def sc_no_override(bls, layout):
    """no NWV_BLS_KEY_GROUP_RATIO: groups of six over three keys gain nothing, the call takes the
    path it takes with the setting off"""
    rig = Rig(bls, 178)
    items = rig.sign(rig.who(23, "mixed"))
    items[9] = wrong_message(items[9])
    on = rig.run(items)
    bls.set_key_batch_min(0)
    return {"on": on, "off": rig.run(items)}


def sc_default_off(bls, layout):
    """no environment: 1,100 one-key items over the committee, with the setting at its default,
    on, and back at 0"""
    rig = Rig(bls, 179)
    n = 1100
    who = [[i % 4] for i in range(n)]
    items = rig.sign(who)
    out = {"min_fresh": bls.key_batch_min()}

    def go():
        got = bls.verify_many(rig.keys, [i[0] for i in items], who, [i[2] for i in items])
        return {"got": [int(x) for x in got], "path": bls.last_path(), "kb": list(bls.last_key_batch())}

    out["off"] = go()
    bls.set_key_batch_min(1)
    out["min_set"] = bls.key_batch_min()
    out["on"] = go()
    bls.set_key_batch_min(0)
    out["min_after_zero"] = bls.key_batch_min()
    out["off_again"] = go()
    out["want"] = [int(x) for x in B.verify_items(rig.keys, [i[0] for i in items], who, [i[2] for i in items])]
    return out


def sc_precedence(bls, layout):
    """both settings qualify: the key-transposed check runs, with and without a forgery"""
    rig = Rig(bls, 180)
    bls.set_wave_batch_min(1)
    items = rig.sign(rig.who(13, "mixed"))
    good = rig.run(items)
    items[8] = wrong_message(items[8])
    return {"good": good, "forged": rig.run(items)}


def sc_types(bls, layout):
    """a 4-node committee's seven certificates (3 signers each; one carries another's aggregate)
    through nwv_bls_validate_certificates"""
    import copy
    import test_gpu_types_bls as TB
    from narwhal_amd import types as T
    eng = bls.eng
    rnd = random.Random(181)
    n = 4
    sks = [rnd.randrange(1, r).to_bytes(32, "big") for _ in range(n)]
    sk_of = dict(zip(bls.keygen(sks), sks))
    com = T.Committee(sorted(sk_of), [1] * n, 0, [[0, 1, 2, 3]] * n)
    bls.register_keys(list(com.keys))
    q = com.quorum_threshold()
    parents = T.bls_certificate_digests(eng, T.BlsCertificate.genesis(com))
    headers = [T.Header(author=com.keys[a % n], round=1 + a // n, epoch=0, payload=[(rnd.randbytes(32), a % 4)],
                        parents=list(parents), signature=bytes(48)) for a in range(7)]
    for h, d in zip(headers, T.bls_header_digests(eng, headers)):
        h.id = d
    for h, s in zip(headers, bls.sign([sk_of[h.author] for h in headers], [h.id for h in headers])):
        h.signature = s
    voters = [sorted(rnd.sample(range(n), q)) for _ in range(7)]
    votes = [T.Vote(headers[a].id, headers[a].round, 0, headers[a].author, com.keys[v], bytes(48))
             for a in range(7) for v in voters[a]]
    for v, s in zip(votes, bls.sign([sk_of[v.author] for v in votes], T.bls_vote_digests(eng, votes))):
        v.signature = s
    certs = [T.BlsCertificate.new(eng, com, headers[a], [(v.author, v.signature) for v in votes[a * q:(a + 1) * q]])
             for a in range(7)]
    certs[4] = copy.deepcopy(certs[4])
    certs[4].aggregated_signature = certs[2].aggregated_signature
    want = TB._oracle_codes({"com": com}, [], [], certs)[2]
    ok, bad = T.bls_validate_certificates(eng, com, certs)
    return {"q": q, "want_invalid": [i for i, c in enumerate(want) if c], "ok": bool(ok), "invalid": [int(i) for i in bad],
            "path": bls.last_path(), "kb": list(bls.last_key_batch())}


def main():
    import narwhal_amd
    from narwhal_amd.bls import Bls
    scenario = sys.argv[1]
    layout = sys.argv[2] if len(sys.argv) > 2 else "mixed"
    e = narwhal_amd.Engine(device=0)
    bls = Bls(e)
    out = {"min_fresh": bls.key_batch_min()}
    if scenario != "default_off":
        bls.set_key_batch_min(1)
    out.update(globals()["sc_" + scenario](bls, layout))
    e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
