"""Child process of tests/test_gpu_grouped.py: the library reads NWV_GROUP_MAX_N once per process,
so the pass-through above it is checked in a process of its own.  Runs grouped calls of the sizes
given (8 unregistered keys, signature i by key i % 8) and prints one JSON line: per size, the
verdict and the nwv_diag_grouped deltas of the call."""
import argparse
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65,64")
    a = ap.parse_args()
    import narwhal_amd
    from narwhal_amd import _lib
    import oracle_ffi as of
    eng = narwhal_amd.Engine(device=0)
    rnd = random.Random(9)
    seeds = [rnd.randbytes(32) for _ in range(8)]
    keys = [of.pubkey(s) for s in seeds]
    out = {}
    for n in (int(x) for x in a.sizes.split(",")):
        msgs = [rnd.randbytes(32) for _ in range(n)]
        _, sg = eng.sign_many([seeds[i % 8] for i in range(n)], msgs)
        items = [(keys[i % 8], sg[64 * i:64 * i + 64].tobytes(), msgs[i]) for i in range(n)]
        g0 = eng.diag_grouped()
        ok, bits = eng.verify_batch_grouped_arrays(*_lib.soa(items))
        g1 = eng.diag_grouped()
        bad = list(items)
        bad[n - 1] = (bad[n - 1][0], bad[n - 1][1][:40] + bytes([bad[n - 1][1][40] ^ 1]) + bad[n - 1][1][41:], bad[n - 1][2])
        ok_bad, bits_bad = eng.verify_batch_grouped_arrays(*_lib.soa(bad))
        out[str(n)] = {"ok": bool(ok) and all(bool(b) for b in bits), "delta": {k: g1[k] - g0[k] for k in g1},
                       "bad_rejected": not ok_bad,
                       "bad_bits_are_the_oracles": [bool(b) for b in bits_bad] == [of.verify(*it) for it in bad]}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
