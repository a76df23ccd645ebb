"""Child process of tests/test_gpu_bls_wave_batch.py.  The wave batch check's settings
(NWV_BLS_WAVE_MAX, NWV_BLS_BATCH_GROUP, NWV_BLS_PACK, NWV_BLS_DEVICE_REPLICAS, NWV_BLS_SHARD_MIN)
are read once per process, so every configuration runs in a fresh one: the parent sets the
environment, this runs one scenario (argv[1], with the key layout in argv[2] where one applies) on
a context with nwv_bls_set_wave_batch_min(1) and prints one JSON line.  The oracle is
bls_ffi.fast_aggregate_verify."""
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


def neg_g1(sig):
    """-P of a compressed G1 point: the encoding's sign bit flipped"""
    b = bytearray(sig)
    b[0] ^= 0x20
    return bytes(b)


def oracle(keys, items):
    return [int(B.fast_aggregate_verify(s, [keys[k] for k in ks], m)) for s, ks, m in items]


class Rig:
    """a 10-key committee plus one stray key (index 10) that is never registered"""

    def __init__(self, bls, layout, seed):
        self.bls = bls
        self.rnd = random.Random(seed)
        self.sks = [self.rnd.randrange(1, r).to_bytes(32, "big") for _ in range(11)]
        self.keys = bls.keygen(self.sks)
        self.layout = layout
        if layout in ("registered", "mixed"):
            bls.register_keys(self.keys[:10])

    def valid(self, n):
        """n valid items: one-key items over the committee (every second one over the stray key in
        the mixed layout), every fourth a three-signer aggregate"""
        who, msgs = [], []
        for i in range(n):
            if self.layout == "mixed" and i % 2:
                who.append([10])
            elif i % 4 == 3:
                who.append(sorted(self.rnd.sample(range(10), 3)))
            else:
                who.append([i % 10])
            msgs.append(self.rnd.randbytes(32))
        flat = self.bls.sign([self.sks[k] for ks in who for k in ks], [m for ks, m in zip(who, msgs) for _ in ks])
        items, at = [], 0
        for ks, m in zip(who, msgs):
            rc, agg = B.aggregate(flat[at:at + len(ks)])
            assert rc == 0
            at += len(ks)
            items.append((agg, ks, m))
        return items

    def run(self, items, keys=None):
        keys = keys or self.keys
        got = self.bls.verify_many(keys, [i[0] for i in items], [i[1] for i in items], [i[2] for i in items])
        return {"got": [int(x) for x in got], "want": oracle(keys, items), "path": self.bls.last_path(),
                "batch": list(self.bls.last_batch())}


def sc_sizes(bls, layout):
    rig = Rig(bls, layout, 71)
    return {"runs": {str(n): rig.run(rig.valid(n)) for n in (1, 5, 6, 16, 23)}}


def sc_forgery(bls, layout):
    rig = Rig(bls, layout, 72)
    items = rig.valid(23)
    s, ks, m = items[12]  # the middle group of five (items 10..14 at group size 5)
    items[12] = (s, ks, m[:-1] + bytes([m[-1] ^ 1]))
    return rig.run(items)


def sc_two_rejected(bls, layout):
    """23 items at group size 5, two forgeries a run: in groups 0 and 3 (the accepted groups 1 and 2
    between them share the re-check launch), then in group 0 and the partial last group"""
    rig = Rig(bls, layout, 77)
    valid = rig.valid(23)
    runs = {}
    for name, bad in (("apart", (2, 17)), ("to_the_end", (2, 21))):
        items = list(valid)
        for k in bad:
            s, ks, m = items[k]
            items[k] = (s, ks, m[:-1] + bytes([m[-1] ^ 1]))
        runs[name] = rig.run(items)
    return {"runs": runs}


def sc_cancel(bls, layout):
    rig = Rig(bls, layout, 73)
    items = rig.valid(16)
    a, b, D = 6, 8, items[15][0]  # both in the second group
    rc1, sa = B.aggregate([items[a][0], D])
    rc2, sb = B.aggregate([items[b][0], neg_g1(D)])
    assert rc1 == 0 and rc2 == 0
    same_sum = B.aggregate([sa, sb])[1] == B.aggregate([items[a][0], items[b][0]])[1]
    items[a] = (sa,) + items[a][1:]
    items[b] = (sb,) + items[b][1:]
    out = rig.run(items)
    out.update(a=a, b=b, same_sum=same_sum)
    return out


def sc_pre(bls, layout):
    """every category that fails before the pairing equation, beside valid items; items 5..9 are a
    whole group of them"""
    rig = Rig(bls, layout, 74)
    keys = rig.keys + [C.not_in_g2(), C.IDENTITY_G2, C.negate_g2(rig.keys[0])]  # 11, 12, 13
    v = rig.valid(12)
    agg, who, d = v[0]
    bad = [(agg, [], d),                       # empty key list
           (agg, who + [11], d),               # a key outside G2
           (agg, who + [12], d),               # identity key
           (agg, [0, 13], d),                  # identity key sum
           (C.not_in_g1(), who, d),            # signature outside G1
           (C.IDENTITY_G1, who, d),            # identity signature
           ] + [(b, who, d) for b in C.bad_encodings_g1(agg)]
    items = v[:5] + bad[:5] + v[5:9] + bad[5:] + v[9:]
    out = rig.run(items, keys)
    out["n_bad"] = len(bad)
    out["group1_want"] = out["want"][5:10]
    return out


def sc_sharded(bls, layout):
    """three shards of ten items each (NWV_BLS_DEVICE_REPLICAS=3, NWV_BLS_SHARD_MIN=8), one forgery
    in every shard"""
    rig = Rig(bls, layout, 75)
    items = rig.valid(30)
    for k in (3, 14, 27):
        s, ks, m = items[k]
        items[k] = (s, ks, m[:-1] + bytes([m[-1] ^ 1]))
    return rig.run(items)


def sc_default_off(bls, layout):
    """no environment: 1,100 one-key items over a registered committee, first with the setting at
    its default, then with it on"""
    rig = Rig(bls, "registered", 76)
    n = 1100
    who = [[i % 10] for i in range(n)]
    msgs = [rig.rnd.randbytes(32) for _ in range(n)]
    sigs = bls.sign([rig.sks[k[0]] for k in who], msgs)
    out = {"min_fresh": bls.wave_batch_min()}
    bls.set_wave_batch_min(0)
    out["min_after_zero"] = bls.wave_batch_min()
    out["off"] = {"got": [int(x) for x in bls.verify_many(rig.keys, sigs, who, msgs)], "path": bls.last_path(),
                  "batch": list(bls.last_batch())}
    bls.set_wave_batch_min(1)
    out["min_set"] = bls.wave_batch_min()
    out["on"] = {"got": [int(x) for x in bls.verify_many(rig.keys, sigs, who, msgs)], "path": bls.last_path(),
                 "batch": list(bls.last_batch())}
    out["want"] = [int(x) for x in B.verify_items(rig.keys, sigs, who, msgs)]
    return out


def main():
    import narwhal_amd
    from narwhal_amd.bls import Bls
    scenario = sys.argv[1]
    layout = sys.argv[2] if len(sys.argv) > 2 else "registered"
    e = narwhal_amd.Engine(device=0)
    bls = Bls(e)
    out = {"min_fresh": bls.wave_batch_min()}
    if scenario != "default_off":
        bls.set_wave_batch_min(1)
    out.update(globals()["sc_" + scenario](bls, layout))
    e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
