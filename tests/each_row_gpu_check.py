"""Child process of tests/test_gpu_each_row.py: run with NWV_DEVICE_REPLICAS=3 (read by nwv_init), so
one GPU carries three independent device objects and an all-devices context places or splits every
Ed25519 call over them (narwhal_amd/csrc/shard.h, place.h).  verify_each of 200 signatures is one
range on one device and takes the row kernel (k_ed_each_row) there; 40,000 signatures split into
ranges of at least the shard minimum, each above each_row_max, and keep the lane pipeline.  Verdict
bits against the oracle's.  Prints one JSON line."""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import oracle_ffi as of  # noqa: E402  (checker)

ED = 0


def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def _oracle_bits(items):
    pk, sig, msg, offs, lens = of.pack(items)
    words = of.verify_each_mt(pk, sig, msg, offs, lens, _threads())
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:len(items)].astype(bool)


def _batch(eng, n, seed, nbad):
    rnd = random.Random(seed)
    seeds = [rnd.randbytes(32) for _ in range(16)]
    use = [seeds[i % 16] for i in range(n)]
    msgs = [rnd.randbytes(32) for _ in range(n)]
    pk, sg = eng.sign_many(use, msgs)
    items = [(pk[32 * i:32 * i + 32].tobytes(), sg[64 * i:64 * i + 64].tobytes(), msgs[i]) for i in range(n)]
    for i in sorted({0, 63, 64, n - 1} | set(rnd.sample(range(n), nbad))):
        p, s, m = items[i]
        s = bytearray(s)
        s[45] ^= 0x04
        items[i] = (p, bytes(s), m)
    return items


def _each_by_device(eng):
    return [eng.device_counters(ED, i)["each"] for i in range(eng.device_count)]


def main():
    import narwhal_amd
    out = {}
    eng = narwhal_amd.Engine(device=None, n_devices=0)
    eng.set_each_row_max(4096)
    out["devices"] = eng.device_count
    for name, n, nbad in (("small", 200, 10), ("large", 40000, 100)):
        items = _batch(eng, n, n, nbad)
        want = _oracle_bits(items)
        r0, d0, g0 = eng.diag_each_row(), _each_by_device(eng), \
            [eng.device_counters(ED, i)["ranges"] for i in range(eng.device_count)]
        got = np.array(eng.verify_each(items), dtype=bool)
        r1, d1 = eng.diag_each_row(), _each_by_device(eng)
        g1 = [eng.device_counters(ED, i)["ranges"] for i in range(eng.device_count)]
        out[name + "_equal"] = bool((got == want).all())
        out[name + "_bad"] = int((~want).sum())
        out[name + "_rows"] = [r1[0] - r0[0], r1[1] - r0[1]]
        out[name + "_each_by_device"] = [b - a for a, b in zip(d0, d1)]
        out[name + "_ranges"] = sum(b - a for a, b in zip(g0, g1))
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
