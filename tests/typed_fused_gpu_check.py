"""Child process of tests/test_gpu_typed_fused.py: typed calls (header / vote / certificate
verification) with nwv_set_typed_fused on and off against the oracle restatement
(oracle/narwhal_types.py), the digests against hashlib, and the diagnostics that say which form ran.
--part main: one device, both settings.  --part fallback: contexts and calls that must take the
two-launch form.  --part replicas (NWV_DEVICE_REPLICAS=3): three device objects, three threads.
Prints one JSON line; every "bad" list is empty when all is well."""
import argparse
import hashlib
import json
import os
import random
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import oracle_ffi as of  # noqa: E402  (checker)
import types_util as tu  # noqa: E402
from types_util import nt  # noqa: E402

from narwhal_amd import _lib  # noqa: E402
from narwhal_amd import types as T  # noqa: E402

L = 2**252 + 27742317777372353535851937790883648493


def _ver(pk, sig, msg):
    return of.verify(pk, sig, msg)


def _b2(m):
    return hashlib.blake2b(m, digest_size=32).digest()


def _engine(on, **kw):
    import narwhal_amd
    e = narwhal_amd.Engine(**kw)
    e.set_typed_fused(on)
    return e


def _forge(sig, kind, seed, other_msg):
    """a forgery of a valid signature: of R, of s, of s + l (non-canonical), or over another message"""
    if kind == "R":
        return bytes([sig[0] ^ 2]) + sig[1:]
    if kind == "s":
        return sig[:40] + bytes([sig[40] ^ 1]) + sig[41:]
    if kind == "s+l":
        s = int.from_bytes(sig[32:], "little") + L
        return sig[:32] + s.to_bytes(32, "little")
    return of.sign(seed, other_msg)


def _cert(fx, h, n_signers, rnd):
    a = fx.authorities.index(h["author"])
    signers = [i for i in range(len(fx.authorities)) if i != a]
    rnd.shuffle(signers)
    return tu.oracle_certificate(fx, h, signers[:n_signers])


def _header(fx, rnd, n_parents, n_payload, author=None):
    a = rnd.randrange(len(fx.authorities)) if author is None else author
    parents = sorted({rnd.randbytes(32) for _ in range(n_parents)})
    return fx.header(author_idx=a, round_=rnd.randint(1, 9), parents=parents,
                     payload=[(rnd.randbytes(32), rnd.randint(0, 3)) for _ in range(n_payload)])


def id_digest_cases(fx, rnd):
    """the three id / digest / signature cases of a header: (header, expected code)"""
    a = rnd.randrange(len(fx.authorities))
    h = _header(fx, rnd, 3, 1, author=a)
    wrong = rnd.randbytes(32)
    return [(dict(h, id=wrong, signature=of.sign(fx.seeds[a], wrong)), nt.INVALID_HEADER_ID),  # valid over id
            (dict(h, id=wrong), nt.INVALID_HEADER_ID),                                          # valid over the digest
            (dict(h, signature=_forge(h["signature"], "s", None, None)), nt.INVALID_SIGNATURE)]


def cases(fx, rnd, signer_counts):
    """headers, votes and certificates of every kind the issue lists, as oracle dicts"""
    from test_gpu_types import _mutations
    c = fx.committee
    muts = _mutations(fx, rnd)
    H = [h for h, _ in muts if h is not None]
    C = [x for _, x in muts]
    # preimage lengths across the 128-byte block edges: 48 + 36 payload + 32 parents
    for npar in range(5):
        for npay in range(4):
            H.append(_header(fx, rnd, npar, npay))
    H.append(_header(fx, rnd, 100, 2))
    for hh, _ in id_digest_cases(fx, rnd):
        H.append(hh)
        C.append(dict(_cert(fx, hh, c.quorum_threshold(), rnd), header=hh))
    for q in signer_counts:
        h = _header(fx, rnd, 4, 1)
        C.append(_cert(fx, h, q, rnd))
        for kind in ("R", "s", "s+l", "msg"):
            x = _cert(fx, h, q, rnd)
            k = rnd.randrange(len(x["sigs"]))
            pk = c.keys[x["signed"][k]]
            seed = fx.seeds[fx.authorities.index(pk)]
            x["sigs"][k] = _forge(x["sigs"][k], kind, seed, rnd.randbytes(32))
            C.append(x)
            a = fx.authorities.index(h["author"])
            H.append(dict(h, signature=_forge(h["signature"], kind, fx.seeds[a], rnd.randbytes(32))))
    C.append({"header": {"author": c.keys[0], "round": 0, "epoch": c.epoch, "payload": [], "parents": [],
                         "id": bytes(32), "signature": bytes(64)}, "signed": [], "sigs": []})  # genesis
    C.append(dict(C[0], header=dict(C[0]["header"], epoch=c.epoch + 1)))  # wrong epoch
    h = _header(fx, rnd, 2, 0)
    V = fx.votes(h)[:8]
    V[1] = dict(V[1], epoch=c.epoch + 1)
    V[2] = dict(V[2], author=of.pubkey(b"\x01" * 32))
    for k, kind in enumerate(("R", "s", "s+l", "msg")):
        i = 3 + k
        if i < len(V):
            seed = fx.seeds[fx.authorities.index(V[i]["author"])]
            V[i] = dict(V[i], signature=_forge(V[i]["signature"], kind, seed, rnd.randbytes(32)))
    return H, V, C


def want_of(fx, H, V, C):
    c = fx.committee
    return ([nt.header_verify(c, h, _ver) for h in H], [nt.vote_verify(c, v, _ver) for v in V],
            [nt.certificate_verify(c, x, _ver) for x in C])


def check_items(e, fx, H, V, C, want, bad, tag):
    """every item alone (the per-call paths) and all of them in one mixed call"""
    c = tu.committee(fx.committee)
    TH, TV, TC = [tu.header(h) for h in H], [tu.vote(v) for v in V], [tu.certificate(x) for x in C]
    for i, x in enumerate(TH):
        got = T.verify_headers(e, c, [x])[0]
        if got != want[0][i]:
            bad.append([tag, "header", i, got, want[0][i]])
    for i, x in enumerate(TV):
        got = T.verify_votes(e, c, [x])[0]
        if got != want[1][i]:
            bad.append([tag, "vote", i, got, want[1][i]])
    for i, x in enumerate(TC):
        got = T.verify_certificates(e, c, [x])[0]
        if got != want[2][i]:
            bad.append([tag, "certificate", i, got, want[2][i]])
    got = T.verify_mixed(e, c, TH, TV, TC)
    if [list(g) for g in got] != [list(w) for w in want]:
        bad.append([tag, "mixed"])


def main_part():
    out, bad = {}, []
    on, off = _engine(True, device=0), _engine(False, device=0)
    out["setting"] = [on.typed_fused, off.typed_fused]
    for size, counts, seed in ((4, (3,), 41), (34, (23,), 42), (94, (63, 64, 65), 43)):
        rnd = random.Random(seed)
        fx = nt.CommitteeFixture(size, of.pubkey, of.sign, seed=seed)
        H, V, C = cases(fx, rnd, counts)
        want = want_of(fx, H, V, C)
        out[f"codes_{size}"] = sorted(set(want[0]) | set(want[1]) | set(want[2]))
        for e, tag in ((on, f"on{size}"), (off, f"off{size}")):
            check_items(e, fx, H, V, C, want, bad, tag)
        # the three id / digest / signature cases give the stated codes
        rnd2 = random.Random(seed + 100)
        for e, tag in ((on, "on"), (off, "off")):
            for k, (hh, code) in enumerate(id_digest_cases(fx, rnd2)):
                got = T.verify_headers(e, tu.committee(fx.committee), [tu.header(hh)])[0]
                if got != code:
                    bad.append([tag, "id-case", size, k, got, code])
    out["bad"] = bad
    # path selection: a C1 certificate (4 keys, 3 + 1 signatures)
    fx = nt.CommitteeFixture(4, of.pubkey, of.sign, seed=41)
    c = tu.committee(fx.committee)
    rnd = random.Random(5)
    x = tu.certificate(_cert(fx, _header(fx, rnd, 4, 1), 3, rnd))
    x94fx = nt.CommitteeFixture(94, of.pubkey, of.sign, seed=43)
    x94 = tu.certificate(_cert(x94fx, _header(x94fx, rnd, 4, 1), 64, rnd))
    c94 = tu.committee(x94fx.committee)
    for e, tag in ((on, "on"), (off, "off")):
        c0, f0 = e.diag_counters_ex(), e.diag_typed_fused()
        r = T.verify_certificates(e, c, [x])
        c1, f1 = e.diag_counters_ex(), e.diag_typed_fused()
        r94 = T.verify_certificates(e, c94, [x94])
        c2, f2 = e.diag_counters_ex(), e.diag_typed_fused()
        d1 = e.device_counters(0, 0)
        out[f"c1_{tag}"] = {"result": r, "counters": {k: c1[k] - c0[k] for k in c1},
                            "fused": [b - a for a, b in zip(f0, f1)]}
        out[f"c94_{tag}"] = {"result": r94, "counters": {k: c2[k] - c1[k] for k in c2},
                             "fused": [b - a for a, b in zip(f1, f2)]}
        out[f"device_counters_{tag}"] = [d1.get("tiny"), d1.get("comb"), c2["tiny"], c2["comb"]]
    out["off_fused_total"] = list(off.diag_typed_fused())
    # digests in both modes against hashlib: the engine call's outputs (short, side, unused short,
    # every length across the block edges) and nwv_header_digest_many
    dbad = []
    rnd = random.Random(77)
    seeds = fx.seeds
    keys = [of.pubkey(s) for s in seeds]
    pre = [rnd.randbytes(n) for n in (0, 1, 79, 80, 81, 127, 128, 129, 255, 256, 257, 384, 3300)] + \
          [rnd.randbytes(80) for _ in range(40)]
    short = [len(p) <= 128 and i % 3 != 2 for i, p in enumerate(pre)]
    lits = [rnd.randbytes(32) for _ in range(3)]
    kidx, sigs, midx = [], [], []
    for i, p in enumerate(pre):
        if short[i] and i % 2 == 0:  # (every other short preimage stays unused)
            for k in (i % 4, (i + 1) % 4):
                kidx.append(k)
                sigs.append(of.sign(seeds[k], _b2(p)))
                midx.append(i)
    for j, m in enumerate(lits):
        kidx.append(j)
        sigs.append(of.sign(seeds[j], m))
        midx.append(len(pre) + j)
    sigs[1] = _forge(sigs[1], "s", None, None)
    wantv = [of.verify(keys[k], s, (_b2(pre[m]) if m < len(pre) else lits[m - len(pre)])) for k, s, m in zip(kidx, sigs, midx)]
    for e, tag in ((on, "on"), (off, "off")):
        e.keycache_register(keys)
        f0 = e.diag_typed_fused()
        dig, ok, verdicts = e.verify_batch_typed(pre, short, lits, keys, kidx, sigs, midx)
        f1 = e.diag_typed_fused()
        if dig != [_b2(p) for p in pre]:
            dbad.append([tag, "typed digests", [i for i, (a, p) in enumerate(zip(dig, pre)) if a != _b2(p)]])
        if verdicts != wantv or ok:
            dbad.append([tag, "typed verdicts"])
        out[f"typed_call_{tag}"] = [b - a for a, b in zip(f0, f1)]
        # a signature over a side preimage's digest: the two-launch form, same answers
        sh2 = list(short)
        sh2[midx[0]] = False
        dig2, ok2, v2 = e.verify_batch_typed(pre, sh2, lits, keys, kidx, sigs, midx)
        f2 = e.diag_typed_fused()
        if dig2 != dig or v2 != wantv:
            dbad.append([tag, "side-signed"])
        out[f"side_signed_{tag}"] = [b - a for a, b in zip(f1, f2)]
        hs = [tu.header(_header(fx, rnd, npar, npay)) for npar in (0, 1, 2, 3, 4, 100) for npay in range(4)]
        if T.header_digests(e, hs) != [nt.header_digest(h.author, h.round, h.epoch, h.payload, h.parents) for h in hs]:
            dbad.append([tag, "header_digest_many"])
    out["digest_bad"] = dbad
    # two threads on one engine, each its own items, many calls
    fx34 = nt.CommitteeFixture(34, of.pubkey, of.sign, seed=42)
    c34 = tu.committee(fx34.committee)
    jobs = []
    for t in range(2):
        rnd = random.Random(200 + t)
        H, V, C = cases(fx34, rnd, (23,))
        jobs.append((H, V, C, want_of(fx34, H, V, C)))
    res = [None, None]

    def work(t):
        H, V, C, want = jobs[t]
        TH, TV, TC = [tu.header(h) for h in H], [tu.vote(v) for v in V], [tu.certificate(x) for x in C]
        okay = True
        for _ in range(3):
            okay = okay and [list(g) for g in T.verify_mixed(on, c34, TH, TV, TC)] == [list(w) for w in want]
            okay = okay and all(T.verify_certificates(on, c34, [x])[0] == w for x, w in zip(TC, want[2]))
        res[t] = okay

    th = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    out["threads"] = res
    on.close()
    off.close()
    return out


def fallback_part():
    out, bad = {}, []
    fx = nt.CommitteeFixture(4, of.pubkey, of.sign, seed=41)
    rnd = random.Random(9)
    H, V, C = cases(fx, rnd, (3,))
    want = want_of(fx, H, V, C)
    for flag, tag in ((_lib.NWV_FLAG_NO_TINY, "no_tiny"), (_lib.NWV_FLAG_MSM_ALWAYS, "msm_always")):
        e = _engine(True, device=0, flags=flag)
        check_items(e, fx, H, V, C, want, bad, tag)
        out[tag] = list(e.diag_typed_fused())
        e.close()
    e = _engine(True, device=0)
    # an unregistered signer: the committee's keys have tables, the extra key of this call has none
    seeds = fx.seeds + [b"\x55" * 32]
    keys = [of.pubkey(s) for s in seeds]
    e.keycache_register(keys[:4])
    pre = [rnd.randbytes(80) for _ in range(3)]
    kidx = [0, 4, 2]
    sigs = [of.sign(seeds[k], hashlib.blake2b(p, digest_size=32).digest()) for k, p in zip(kidx, pre)]
    f0 = e.diag_typed_fused()
    dig, ok, v = e.verify_batch_typed(pre, [True] * 3, [], keys, kidx, sigs, [0, 1, 2])
    f1 = e.diag_typed_fused()
    out["unregistered"] = {"ok": ok, "verdicts": v, "digests": dig == [_b2(p) for p in pre],
                           "fused": [b - a for a, b in zip(f0, f1)]}
    # a round above the comb limit: 100 certificates x (1 + 67) signatures and their headers and votes
    fx100 = nt.CommitteeFixture(100, of.pubkey, of.sign, seed=100)
    c100 = tu.committee(fx100.committee)
    q = fx100.committee.quorum_threshold()
    parents = sorted(rnd.randbytes(32) for _ in range(q))
    Hs, Cs = [], []
    for a in range(100):
        h = fx100.header(author_idx=a, parents=parents, payload=[(rnd.randbytes(32), a % 4)])
        Hs.append(h)
        Cs.append(tu.oracle_certificate(fx100, h, [i for i in range(100) if i != a][:q]))
    s = Cs[7]["sigs"][5]
    Cs[7] = dict(Cs[7], sigs=Cs[7]["sigs"][:5] + [_forge(s, "s", None, None)] + Cs[7]["sigs"][6:])
    Hs[41] = dict(Hs[41], signature=bytes(64))
    Cs[41] = dict(Cs[41], header=Hs[41])
    Vs = fx100.votes(Hs[0]) + fx100.votes(Hs[1])[:1]  # 100 votes: 100 + 100 + 100 x 68 = 7,000 signatures
    want100 = want_of(fx100, Hs, Vs, Cs)
    f0, c0 = e.diag_typed_fused(), e.diag_counters_ex()
    got = T.verify_mixed(e, c100, [tu.header(h) for h in Hs], [tu.vote(v) for v in Vs], [tu.certificate(x) for x in Cs])
    f1, c1 = e.diag_typed_fused(), e.diag_counters_ex()
    out["round"] = {"equal": [list(g) for g in got] == [list(w) for w in want100],
                    "signatures": 100 + len(Vs) + sum(1 + len(x["sigs"]) for x in Cs),
                    "rejected": [want100[0].count(14), want100[2].count(14)],
                    "fused": [b - a for a, b in zip(f0, f1)], "counters": {k: c1[k] - c0[k] for k in c1}}
    e.close()
    out["bad"] = bad
    return out


def replicas_part():
    out = {}
    e = _engine(True, device=None, n_devices=0)
    out["devices"] = e.device_count
    fx = nt.CommitteeFixture(34, of.pubkey, of.sign, seed=42)
    c = tu.committee(fx.committee)
    jobs = []
    for t in range(3):
        rnd = random.Random(300 + t)
        H, V, C = cases(fx, rnd, (23,))
        jobs.append((H, V, C, want_of(fx, H, V, C)))
    res = [None] * 3
    gate = threading.Barrier(3)

    def work(t):
        H, V, C, want = jobs[t]
        TH, TV, TC = [tu.header(h) for h in H], [tu.vote(v) for v in V], [tu.certificate(x) for x in C]
        gate.wait(timeout=60)
        okay = [list(g) for g in T.verify_mixed(e, c, TH, TV, TC)] == [list(w) for w in want]
        okay = okay and all(T.verify_certificates(e, c, [x])[0] == w for x, w in zip(TC, want[2]))
        okay = okay and all(T.verify_headers(e, c, [x])[0] == w for x, w in zip(TH, want[0]))
        res[t] = okay

    th = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(3)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    out["alive"] = [x.is_alive() for x in th]
    out["equal"] = res
    out["fused"] = list(e.diag_typed_fused())
    out["tiny_by_device"] = [e.device_counters(0, i).get("tiny") for i in range(e.device_count)]
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["main", "fallback", "replicas"])
    a = ap.parse_args()
    print(json.dumps({"main": main_part, "fallback": fallback_part, "replicas": replicas_part}[a.part]()))


if __name__ == "__main__":
    main()
