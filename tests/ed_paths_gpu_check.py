"""Child process of tests/test_gpu_ed_paths.py (NWV_LANES=1): one engine on device 0 whose single
lane serves, in turn, a batch on every Ed25519 path (ed_plan.h): tiny, MSM, comb, MSM with the comb
pass, the grouped trait call, a typed call in the one-launch form, then a staged keyed batch.  Every
batch has one forged signature at its last index; verdict bits against the oracle's, and the
counters that say which path ran.  Prints one JSON line."""
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
import types_util as tu  # noqa: E402
from types_util import nt  # noqa: E402

from narwhal_amd import _lib  # noqa: E402
from narwhal_amd import types as T  # noqa: E402

ED = 0
NMAX = 129


def main():
    import narwhal_amd
    out = {"lanes_env": os.environ.get("NWV_LANES")}
    e = narwhal_amd.Engine(device=0)
    e.set_latency_max(ED, 0)  # no latency class: the reserved lanes stay unused
    e.set_comb_batch_max(128)
    e.set_comb_pass_max(256)
    e.set_typed_fused(True)
    out["limits"] = [e.latency_max(ED), e.comb_batch_max, e.comb_pass_max]
    fx = nt.CommitteeFixture(4, of.pubkey, of.sign, seed=41)
    seeds = fx.seeds
    keys = [of.pubkey(s) for s in seeds]
    e.keycache_register(keys)

    # one pool of signatures by the four keys; a batch of n is its first n with the last one forged.
    # The oracle's verdicts are computed once here and only compared against below.
    rnd = random.Random(2041)
    kidx = [i % 4 for i in range(NMAX)]
    msgs = [rnd.randbytes(32 + i % 5) for i in range(NMAX)]
    sigs = [of.sign(seeds[k], m) for k, m in zip(kidx, msgs)]
    valid = [of.verify(keys[k], s, m) for k, s, m in zip(kidx, sigs, msgs)]

    def forged(i):
        s = bytearray(sigs[i])
        s[45] ^= 0x04
        return bytes(s)

    batch, want = {}, {}
    for n in (64, 65, 129):
        batch[n] = sigs[:n - 1] + [forged(n - 1)]
        want[n] = valid[:n - 1] + [of.verify(keys[kidx[n - 1]], batch[n][-1], msgs[n - 1])]
    out["oracle_shape"] = {str(n): [all(want[n][:-1]), want[n][-1]] for n in want}

    def snap():
        return e.diag_counters_ex(), e.diag_comb_pass(), e.diag_typed_fused()

    def delta(a, b):
        d = {k: b[0][k] - a[0][k] for k in b[0]}
        d["comb_pass"] = [b[1][0] - a[1][0], b[1][1] - a[1][1]]
        d["typed_fused"] = [y - x for x, y in zip(a[2], b[2])]
        return d

    calls = []

    def keyed(n, want_bits=True):
        ok, bits = e.verify_batch_keyed(keys, kidx[:n], batch[n], msgs[:n], want_bits=want_bits)
        return ok is False and (bits == want[n] if want_bits else bits is None)

    def unkeyed(n):
        ok, bits = e.verify_batch([(keys[kidx[i]], batch[n][i], msgs[i]) for i in range(n)])
        return ok is False and bits == want[n]

    def grouped(n):
        pk, sig, arena, offs, lens = _lib.soa([(keys[kidx[i]], batch[n][i], msgs[i]) for i in range(n)])
        ok, bits = e.verify_batch_grouped_arrays(pk, sig, arena, offs, lens)
        return ok is False and list(bits) == want[n]

    def typed():
        # the 4-key certificate shape of typed_fused_gpu_check.py (3 + 1 signatures), one vote forged
        r2 = random.Random(5)
        parents = sorted({r2.randbytes(32) for _ in range(4)})
        h = fx.header(author_idx=0, round_=3, parents=parents, payload=[(r2.randbytes(32), 1)])
        x = tu.oracle_certificate(fx, h, [1, 2, 3])
        s = bytearray(x["sigs"][-1])
        s[45] ^= 0x04
        x["sigs"][-1] = bytes(s)
        code = nt.certificate_verify(fx.committee, x, lambda pk, sg, m: of.verify(pk, sg, m))
        got = T.verify_certificates(e, tu.committee(fx.committee), [tu.certificate(x)])
        return list(got) == [code] and code == nt.INVALID_SIGNATURE

    plan = [("keyed 64", lambda: keyed(64)), ("un-keyed 64", lambda: unkeyed(64)),
            ("keyed 65", lambda: keyed(65)), ("un-keyed 65", lambda: unkeyed(65)),
            ("keyed 129", lambda: keyed(129)), ("un-keyed 129", lambda: unkeyed(129)),
            ("keyed 64, no bits", lambda: keyed(64, want_bits=False)), ("grouped 65", lambda: grouped(65)),
            ("typed", typed), ("keyed 65 again", lambda: keyed(65))]
    for name, fn in plan:
        a = snap()
        equal = fn()
        calls.append({"call": name, "equal": bool(equal), "delta": delta(a, snap())})
    out["calls"] = calls

    # a staged keyed batch of 64 by the same keys, staged through the same lane: mode 1, mode 0, fetch
    a = snap()
    n = 64
    arena, offs, lens = _lib.pack_messages(msgs[:n])
    st = e.stage_keyed(np.frombuffer(b"".join(keys), dtype=np.uint8), np.array(kidx[:n], dtype=np.uint32),
                       np.frombuffer(b"".join(batch[n]), dtype=np.uint8), arena, offs, lens)
    st.run(1)
    st.run(0)
    ok, bits = st.fetch()
    st.free()
    d = delta(a, snap())
    out["staged"] = {"equal": ok is False and list(bits) == want[n], "tiny": d["tiny"], "comb": d["comb"]}
    q = e.diag_qos(ED, 0)
    out["lanes"] = {k: q[k] for k in ("ordinary_open", "reserved_open", "latency_calls")}
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
