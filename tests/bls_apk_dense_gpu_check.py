"""Child process of tests/test_gpu_bls_apk_dense.py.  The dense key-sum stage's settings
(NWV_BLS_WAVE_MAX, NWV_BLS_APK_LANES, NWV_BLS_KEY_GROUP, NWV_BLS_DEVICE_REPLICAS, ...) are read once
per process, so every configuration runs in a fresh one: the parent sets the environment, this runs
one scenario (argv[1]) and prints one JSON line.  Every call runs twice, with
nwv_bls_set_apk_dense_min at the scenario's value and at 0; the oracle is
bls_ffi.fast_aggregate_verify."""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import bls_ffi as B  # noqa: E402

r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def sk_bytes(x):
    return (x % r).to_bytes(32, "big")


class Rig:
    """secret keys as integers, so that a list's aggregate signature is one signature by the sum of
    its secret keys (with multiplicity); `registered` of them go into the key cache"""

    def __init__(self, bls, seed, sks=None, n_keys=7, registered=None):
        self.bls = bls
        self.rnd = random.Random(seed)
        self.sk = sks or [self.rnd.randrange(1, r) for _ in range(n_keys)]
        self.keys = bls.keygen([sk_bytes(s) for s in self.sk])
        reg = range(len(self.sk)) if registered is None else registered
        bls.register_keys([self.keys[k] for k in reg])

    def sign(self, who, msgs=None):
        """items (sig, key numbers, msg); an empty list or a zero secret-key sum is signed by key 0"""
        msgs = msgs or [self.rnd.randbytes(32) for _ in who]
        sums = [sum(self.sk[k] for k in ks) % r or self.sk[0] for ks in who]
        sigs = self.bls.sign([sk_bytes(s) for s in sums], msgs)
        return [(s, list(ks), m) for s, ks, m in zip(sigs, who, msgs)]

    def run(self, items, keys=None, dense_min=1):
        keys = keys or self.keys
        out = {}
        for tag, v in (("on", dense_min), ("off", 0)):
            self.bls.set_apk_dense_min(v)
            got = self.bls.verify_many(keys, [i[0] for i in items], [i[1] for i in items], [i[2] for i in items])
            out[tag] = {"got": [int(x) for x in got], "path": self.bls.last_path(),
                        "dense": list(self.bls.last_apk_dense()), "kb": list(self.bls.last_key_batch()),
                        "batch": list(self.bls.last_batch())}
        out["want"] = [int(B.fast_aggregate_verify(s, [keys[k] for k in ks], m)) for s, ks, m in items]
        return out


def by_complement(ks, nk):
    return all(a < b for a, b in zip(ks, ks[1:])) and len(ks) > nk // 2


def sc_sizes(bls):
    """NWV_BLS_APK_LANES = L: 1, 64 / L - 1, 64 / L, 64 / L + 1 and 33 items with list lengths 2, 3,
    L - 1, L, L + 1 and 7 in turn, over committees of 4 and of 7 registered keys (ascending lists,
    shuffled ones, and lists with repeats where the length exceeds the committee)"""
    L = int(os.environ["NWV_BLS_APK_LANES"])
    lens = sorted({2, 3, L - 1, L, L + 1, 7})
    rig = Rig(bls, 500 + L)
    runs = []
    for nk in (4, 7):
        for n in (1, 64 // L - 1, 64 // L, 64 // L + 1, 33):
            who = []
            for i in range(n):
                m = lens[(i + n) % len(lens)]
                if m > nk:
                    ks = [rig.rnd.randrange(nk) for _ in range(m)]
                else:
                    ks = sorted(rig.rnd.sample(range(nk), m))
                    if i % 3 == 2:
                        rig.rnd.shuffle(ks)
                who.append(ks)
            runs.append(dict(rig.run(rig.sign(who), rig.keys[:nk]), nk=nk, n=n,
                             comp=sum(by_complement(ks, nk) for ks in who)))
    return {"lanes": L, "runs": runs}


def sc_paths(bls):
    """four registered keys (0..3) and a valid key that is not registered (4)"""
    rig = Rig(bls, 520, n_keys=5, registered=range(4))
    who = [[0, 1, 3], [0, 1, 2, 3], [1, 2], [3, 1, 0], [0, 1, 1, 2], [2], []]
    items = rig.sign(who)
    a = rig.run(items, rig.keys[:4])
    # the same items over a table that holds the unregistered key, and an item that names it
    b = rig.run(items + rig.sign([[0, 4]]), rig.keys)
    return {"registered_table": a, "table_with_unregistered_key": b}


def sc_identity(bls):
    """committees of sk and r - sk: a = 0, -a = 1, b = 2, -b = 3"""
    rnd = random.Random(530)
    a, b = rnd.randrange(1, r), rnd.randrange(1, r)
    rig = Rig(bls, 531, sks=[a, r - a, b, r - b])
    k = rig.keys
    return {"a_na_b": rig.run(rig.sign([[0, 1], [0, 2]]), [k[0], k[1], k[2]]),
            "a_na": rig.run(rig.sign([[0, 1]]), [k[0], k[1]]),
            "a_na_b_nb": rig.run(rig.sign([[0, 2, 3]]), k)}


def sc_pairing(bls):
    """nine valid 5-of-7 certificates; then certificate 4 with one signer swapped in its list for
    an absent key (still ascending, still summed by complement).  argv[2]: per_item, key_batch or
    wave_batch -- the pairing path that reads the sums"""
    mode = sys.argv[2]
    if mode == "key_batch":
        bls.set_key_batch_min(1)
    if mode == "wave_batch":
        bls.set_wave_batch_min(1)
    rig = Rig(bls, 540)
    who = [sorted(rig.rnd.sample(range(7), 5)) for _ in range(9)]
    items = rig.sign(who)
    good = rig.run(items)
    absent = [k for k in range(7) if k not in who[4]]
    swapped = sorted(who[4][1:] + absent[:1])
    items[4] = (items[4][0], swapped, items[4][2])
    return {"good": good, "swapped": rig.run(items), "swapped_by_complement": by_complement(swapped, 7)}


def sc_edges(bls):
    """NWV_BLS_WAVE_MAX=8: the default, the threshold at n - 1 and n, calls of at most 8 items"""
    rig = Rig(bls, 550, n_keys=4)
    out = {"min_fresh": bls.apk_dense_min()}
    items = rig.sign([sorted(rig.rnd.sample(range(4), 3)) for _ in range(12)])
    out["at_12_items_11"] = rig.run(items[:11], dense_min=12)
    out["at_12_items_12"] = rig.run(items, dense_min=12)
    out["at_1_items_8"] = rig.run(items[:8], dense_min=1)
    out["at_1_items_9"] = rig.run(items[:9], dense_min=1)
    bls.set_apk_dense_min(12)
    out["min_set"] = bls.apk_dense_min()
    bls.set_apk_dense_min(0)
    out["min_after_zero"] = bls.apk_dense_min()
    return out


def sc_sharded(bls):
    """three shares of ten items (NWV_BLS_DEVICE_REPLICAS=3, NWV_BLS_SHARD_MIN=8): certificates,
    one-key items, a shuffled list, one forgery a share"""
    rig = Rig(bls, 560)
    who = []
    for i in range(30):
        ks = sorted(rig.rnd.sample(range(7), 5)) if i % 3 else [i % 7]
        if i % 7 == 5:
            rig.rnd.shuffle(ks)
        who.append(ks)
    items = rig.sign(who)
    for k in (3, 14, 27):
        s, ks, m = items[k]
        items[k] = (s, ks, m[:-1] + bytes([m[-1] ^ 1]))
    return rig.run(items)


def main():
    import narwhal_amd
    from narwhal_amd.bls import Bls
    e = narwhal_amd.Engine(device=0)
    bls = Bls(e)
    out = globals()["sc_" + sys.argv[1]](bls)
    e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
