"""Child process of tests/test_gpu_zcoeff.py: cancelling-forgery sets (tests/zcoeff.py) through every
seeded Ed25519 batch call of the engine, so that the device's coefficients z_i -- their full width,
their index and their seed -- are pinned on every kernel form of the batch MSM.  The library reads
its environment knobs once per process, so the parent starts one child per setting.

A "case" is three checks: the valid batch accepts; the cancelling batch with P = all indices accepts
under seed S, without and with verdict bits (bits all ones, no per-signature pass ran); the same
batch under another seed rejects, and its bits equal the oracle's (at most ORACLE_MAX signatures;
beyond that "every touched position false", which the construction guarantees).

  --parts default   distinct keys, default plan, n on both sides of every switch of msm_plan / msm_launch
          keyed     100 keys, key cache on / off, fused key sum on / off
          other     digests call, aggregate call, sparse pairs, staged batches, tiny / comb paths
          forms     n = 1,025 and 4,097 (and FORMS_WIDE_N under NWV_MSM_TAIL_S) with --flags
          staged    the staged cases alone (run under NWV_STAGE_CHAIN=0: captured graph replay)
          shard     NWV_DEVICE_REPLICAS=3, NWV_SHARD_MIN=1024: per-range seeds and local indices

Prints one JSON line."""
import argparse
import ctypes
import json
import os
import random
import sys
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import zcoeff as zc  # noqa: E402

S = bytes(range(1, 33))
S_OTHER = bytes(range(2, 34))
S_LAST = S[:31] + bytes([S[31] ^ 0x80])  # differs from S in its last bit only
ORACLE_MAX = 1100

# msm_plan gives a batch of at most 2,048 bucket entries two entries per bucket lane (seg = 2).
# Distinct keys: entries = (n + 1) nw + n nw_z.  At these sizes the cheapest layout is 22 windows
# of 5 or 6 bits below 2^129 and 25 of 5 bits above (nw = 47, nw_z = 22), so entries = 69 n + 47 and
# the largest n with seg = 2 is 29 (exactly 2,048 entries); 30 has 2,117.  The parent checks the
# constant against plan(), and every case checks plan() against the engine's own (msm_stats).
SEG2_MAX_N = 29
DEFAULT_SIZES = [2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8192, 16384, 16385, SEG2_MAX_N, SEG2_MAX_N + 1]
FORMS_SIZES = [1025, 4097]
# NWV_MSM_TAIL_S=64 reaches k_msm_tail_wide only where a window is at least 11 bits wide (1,024
# buckets: C = 16 per chunk, (lg C + 1) S_w = 320 > 256); the plans of 1,025 and 4,097 signatures stop
# at 9 and 10 bits (192 and 256 items: k_msm_tail with 64 chunks a window).  8,192 is the smallest
# size of the default list whose plan has an 11-bit window.
FORMS_WIDE_N = 8192
SPARSE_N = 1025
SPARSE_PAIRS = [(0, 1), (0, 64), (63, 64), (0, 256), (0, 1024), (517, 518)]


# ---- msm_plan (nwv_host.hip) restated: window widths, entries, seg, tail chunks ----------------
def _layout(c_lo, c_hi, narrow_top, z_only):
    lo_bits, hi_bits = 129, 125
    nz = -(-lo_bits // c_lo)
    nh = 0 if z_only else -(-hi_bits // c_hi)
    if nz + nh > 48:
        return None

    def split(count, total, narrow):
        q, r = divmod(total, count)
        if narrow:
            return [q + 1 if k < r else q for k in range(count)]
        return [total * (k + 1) // count - total * k // count for k in range(count)]

    return nz, split(nz, lo_bits, narrow_top and not z_only) + (split(nh, hi_bits, narrow_top) if nh else [])


def plan(n, na, split=False, env=None):
    """the plan of n signatures with na points before B (n for distinct keys; the m distinct keys,
    or 2 m + 1 over the key cache = split)"""
    env = os.environ if env is None else env
    narrow = n > int(env.get("NWV_TAIL_QUAD_MAX_N", "16384"))
    best = None
    for c_lo in range(6, 16):
        for c_hi in range(3, 16):
            if split and c_hi > 3:
                break
            lay = _layout(c_lo, c_hi, narrow, split)
            if lay is None:
                continue
            nz, widths = lay
            entries = (na + 1) * len(widths) + n * nz
            buckets = sum(1 << (w - 1) for w in widths)
            cost = 7 * entries + 18 * buckets
            if best is None or cost < best[0]:
                best = (cost, nz, widths, entries, buckets)
    _, nz, widths, entries, buckets = best
    seg = min(64, max(8, entries // (256 * 4 * 2 * 64)))
    if entries <= 2048:
        seg = 2
    if "NWV_MSM_SEG" in env:
        seg = max(1, int(env["NWV_MSM_SEG"]))
    tail_s = 1
    while ((1 << (max(widths) - 1)) // tail_s) > 256:
        tail_s <<= 1
    if "NWV_MSM_TAIL_S" in env:
        while tail_s < 64 and (tail_s << 1) <= int(env["NWV_MSM_TAIL_S"]):
            tail_s <<= 1
    items = 0
    for w in widths:
        nb = 1 << (w - 1)
        sw = min(tail_s, nb)
        items = max(items, ((nb // sw).bit_length()) * sw)  # (lg C + 1) S_w, C a power of two
    pts = na + 1 + n
    chunk_pts = max(8192, (pts + 63) // 64)
    return {"points": pts, "windows": len(widths), "windows_z": nz, "buckets": buckets, "entries": entries,
            "chunks": -(-pts // chunk_pts), "seg": seg, "widths": widths, "tail_S": tail_s, "tail_items": items,
            "narrow_top": narrow and not split}


def seg2_max_n():
    n = 1
    while plan(n + 1, n + 1, env={})["entries"] <= 2048:
        n += 1
    return n


# ---- inputs ------------------------------------------------------------------------------------
def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def oracle_bits(items):
    import oracle_ffi as of
    pk, sig, msg, offs, lens = of.pack(items)
    words = of.verify_each_mt(pk, sig, msg, offs, lens, _threads())
    return [bool(b) for b in np.unpackbits(words.view(np.uint8), bitorder="little")[:len(items)]]


def signed(eng, n, m, seed):
    """n signatures over 32-byte messages by m keys (signature i by key i % m) -> keys, kidx, sigs, msgs"""
    rng = np.random.default_rng(seed)
    kseeds = [rng.bytes(32) for _ in range(m)]
    msgs = [rng.bytes(32) for _ in range(n)]
    pk, sg = eng.sign_many([kseeds[i % m] for i in range(n)], msgs)
    keys = [pk[32 * i:32 * i + 32].tobytes() for i in range(m)]
    return keys, [i % m for i in range(n)], [sg[64 * i:64 * i + 64].tobytes() for i in range(n)], msgs


def three_checks(eng, run, oracle_items, sigs, P=None, zs=None, counter="msm", seed_accepts=True, tag=0):
    """run(sigs, seed, want_bits) -> (ok, bits or None); oracle_items(sigs) -> (pk, sig, msg) list.
    seed_accepts False: a path without coefficients -- the set is rejected under S as well."""
    n = len(sigs)
    P = list(range(n)) if P is None else list(P)
    r = {"n": n, "touched": len(P)}
    c0 = eng.diag_counters_ex()
    ok, bits = run(sigs, S, True)
    r["valid_accepts"] = bool(ok) and all(bits)
    forged = zc.cancelling(sigs, P, S, random.Random(1000 * n + tag), zs=zs)
    touched = set(P)
    r["touched_differ"] = all((forged[i] != sigs[i]) == (i in touched) for i in range(n))
    if n <= ORACLE_MAX:
        want = oracle_bits(oracle_items(forged))
        r["oracle_rejects_touched"] = [i for i in range(n) if not want[i]] == sorted(P)
    else:
        want = [i not in touched for i in range(n)]
    c1 = eng.diag_counters_ex()
    ok_nb, _ = run(forged, S, False)
    ok_b, bits = run(forged, S, True)
    c2 = eng.diag_counters_ex()
    if seed_accepts:
        r["seed_accepts_nobits"] = bool(ok_nb)
        r["seed_accepts_bits"] = bool(ok_b) and all(bits)
        r["no_fallback"] = c2["each"] == c1["each"]
    else:
        r["seed_rejects_nobits"] = not ok_nb
        r["seed_rejects_bits"] = (not ok_b) and list(bits) == want
    ok_nb, _ = run(forged, S_OTHER, False)
    r["other_rejects_nobits"] = not ok_nb
    ok_b, bits = run(forged, S_LAST, True)
    r["other_rejects_bits"] = (not ok_b) and list(bits) == want
    c3 = eng.diag_counters_ex()
    r["runs"] = {k: c3[k] - c0[k] for k in c3}
    r["path_ran"] = r["runs"][counter] == 5
    return r


def guarded(out, key, fn):
    try:
        out[key] = fn()
    except Exception:  # the parent reports it against the case's own test
        out[key] = {"error": traceback.format_exc()[-1500:]}


def batch_run(eng, pks, msgs):
    def run(sigs, seed, want_bits):
        return eng.verify_batch(list(zip(pks, sigs, msgs)), seed=seed, want_bits=want_bits)
    return run


def keyed_run(eng, keys, kidx, msgs):
    def run(sigs, seed, want_bits):
        return eng.verify_batch_keyed(keys, kidx, sigs, msgs, seed=seed, want_bits=want_bits)
    return run


def staged_stats(eng, pks, sigs, msgs):
    from narwhal_amd import _lib
    st = eng.stage(*_lib.soa(list(zip(pks, sigs, msgs))))
    try:
        return st.msm_stats()
    finally:
        st.free()


def plan_matches(stats, p):
    return all(stats[k] == p[k] for k in ("points", "windows", "windows_z", "buckets", "chunks", "seg"))


# ---- parts -------------------------------------------------------------------------------------
def part_default(out):
    import narwhal_amd
    eng = narwhal_amd.Engine(device=0)
    keys, _, sigs, msgs = signed(eng, max(DEFAULT_SIZES), max(DEFAULT_SIZES), 1)
    out["seg2_max_n"] = seg2_max_n()
    for n in DEFAULT_SIZES:
        def one(n=n):
            pk, sg, ms = keys[:n], sigs[:n], msgs[:n]
            r = three_checks(eng, batch_run(eng, pk, ms), lambda f: list(zip(pk, f, ms)), sg)
            p = plan(n, n)
            r["plan"] = {k: p[k] for k in ("windows", "windows_z", "entries", "chunks", "seg", "narrow_top")}
            r["plan_matches_engine"] = plan_matches(staged_stats(eng, pk, sg, ms), p)
            return r
        guarded(out, f"default_{n}", one)
    eng.close()


KEYED_CASES = [("kc", 300), ("kc", 8192), ("kc", 8193), ("nokc", 300), ("nokc", 8092), ("nokc", 8093)]


def part_keyed(out):
    import narwhal_amd
    from narwhal_amd import _lib
    for fused in (True, False):
        for cache in ("kc", "nokc"):
            flags = _lib.NWV_FLAG_MSM_ALWAYS | (0 if fused else _lib.NWV_FLAG_NO_FUSED_KEYSUM) | \
                (0 if cache == "kc" else _lib.NWV_FLAG_NO_KEYCACHE)
            eng = narwhal_amd.Engine(device=0, flags=flags)
            keys, kidx, sigs, msgs = signed(eng, 8193, 100, 2)
            for c, n in KEYED_CASES + [(cache, 64)]:
                if c != cache:
                    continue

                def one(n=n):
                    if n == 64:  # 4 keys: the key sums run inside the hash workgroup
                        k4, ki, sg, ms = signed(eng, 64, 4, 3)
                    else:
                        k4, ki, sg, ms = keys, kidx[:n], sigs[:n], msgs[:n]
                    return three_checks(eng, keyed_run(eng, k4, ki, ms),
                                        lambda f: [(k4[ki[i]], f[i], ms[i]) for i in range(n)], sg)
                guarded(out, f"keyed_{cache}_{'fused' if fused else 'nofused'}_{n}", one)
            eng.close()


def case_digests(eng):
    import oracle_ffi as of
    rnd = random.Random(40)
    pre = [rnd.randbytes(rnd.choice([80, 127, 128, 129, 2200])) for _ in range(40)]
    dig = [of.blake2b256(x) for x in pre]
    n, m = 700, 100
    didx = [rnd.randrange(40) for _ in range(n)]
    msgs = [dig[j] for j in didx]
    kseeds = [rnd.randbytes(32) for _ in range(m)]
    pk, sg = eng.sign_many([kseeds[i % m] for i in range(n)], msgs)
    keys = [pk[32 * i:32 * i + 32].tobytes() for i in range(m)]
    kidx = [i % m for i in range(n)]
    sigs = [sg[64 * i:64 * i + 64].tobytes() for i in range(n)]
    digests_ok = []

    def run(s, seed, want_bits):
        d, ok, bits = eng.verify_batch_keyed_digests(pre, keys, kidx, s, didx, seed=seed)
        digests_ok.append(d == dig)
        return ok, bits

    r = three_checks(eng, run, lambda f: [(keys[kidx[i]], f[i], msgs[i]) for i in range(n)], sigs)
    r["digests_equal"] = all(digests_ok)
    return r


def case_aggregate(eng):
    """two aggregates of three signatures, one message each: signature j of aggregate a is index
    3 a + j of the batch"""
    from narwhal_amd import _lib
    rng = np.random.default_rng(6)
    kseeds = [rng.bytes(32) for _ in range(6)]
    m = [rng.bytes(32), rng.bytes(32)]
    pk, sg = eng.sign_many(kseeds, [m[0]] * 3 + [m[1]] * 3)
    pks = [pk[32 * i:32 * i + 32].tobytes() for i in range(6)]
    sigs = [sg[64 * i:64 * i + 64].tobytes() for i in range(6)]

    def call(s, seed):
        arr = lambda *xs: (ctypes.c_char_p * len(xs))(*xs)  # noqa: E731
        sz = lambda *xs: (ctypes.c_size_t * len(xs))(*xs)  # noqa: E731
        return eng.lib.nwv_ed25519_aggregate_batch_verify(
            eng._h, 2, arr(b"".join(s[:3]), b"".join(s[3:])), sz(3, 3), arr(b"".join(pks[:3]), b"".join(pks[3:])),
            sz(3, 3), arr(m[0], m[1]), sz(32, 32), 2, seed)

    c0 = eng.diag_counters_ex()["msm"]
    r = {"valid_accepts": call(sigs, S) == _lib.NWV_OK}
    for name, P in (("all", range(6)), ("second", [4, 5]), ("across", [2, 3])):
        forged = zc.cancelling(sigs, P, S, random.Random(name))
        want = oracle_bits(list(zip(pks, forged, [m[0]] * 3 + [m[1]] * 3)))
        r[name] = {"oracle_rejects_touched": [i for i in range(6) if not want[i]] == list(P),
                   "seed_accepts": call(forged, S) == _lib.NWV_OK,
                   "other_rejects": call(forged, S_OTHER) == _lib.NWV_ERR_SIGNATURE,
                   "last_bit_rejects": call(forged, S_LAST) == _lib.NWV_ERR_SIGNATURE}
    r["msm_runs"] = eng.diag_counters_ex()["msm"] - c0
    return r


def case_staged(eng, keyed):
    """n = 4,096 resident on the device: run(mode 1) under S, another seed, S again -- the second
    and third runs replay (their seed reaches the device through the pinned ring)"""
    from narwhal_amd import _lib
    n = 4096
    keys, kidx, sigs, msgs = signed(eng, n, 100 if keyed else n, 8)
    arena, offs, lens = _lib.pack_messages(msgs)

    def stage(s):
        sg = np.frombuffer(b"".join(s), dtype=np.uint8)
        if keyed:
            return eng.stage_keyed(np.frombuffer(b"".join(keys), dtype=np.uint8), np.asarray(kidx, dtype=np.uint32),
                                   sg, arena, offs, lens)
        return eng.stage(np.frombuffer(b"".join(keys), dtype=np.uint8), sg, arena, offs, lens)

    r = {}
    st = stage(sigs)
    st.run(mode=1, seed=S)
    allv, bits = st.fetch()
    st.free()
    r["valid_accepts"] = bool(allv) and bool(bits.all())
    st = stage(zc.cancelling(sigs, range(n), S, random.Random(4096 + keyed)))
    verdicts = []
    for seed in (S, S_LAST, S, S_OTHER):
        st.run(mode=1, seed=seed)
        allv, bits = st.fetch()
        verdicts.append([bool(allv), int(bits.sum())])
        if seed == S:
            r["tally_after_%d" % len(verdicts)] = list(st.run_tally())
    st.free()
    r["verdicts"] = verdicts
    return r


def case_nocoeff(n):
    """a registered committee's keyed batch on the one-launch path (n <= 64) or the comb path: no
    coefficients, so a set that cancels in the MSM is rejected signature by signature"""
    import narwhal_amd
    eng = narwhal_amd.Engine(device=0)
    eng.set_comb_batch_max(4096)
    keys, kidx, sigs, msgs = signed(eng, n, 10, 50 + n)
    eng.keycache_register(keys)
    r = three_checks(eng, keyed_run(eng, keys, kidx, msgs), lambda f: [(keys[kidx[i]], f[i], msgs[i]) for i in range(n)],
                     sigs, counter="tiny" if n <= 64 else "comb", seed_accepts=False)
    eng.close()
    return r


def part_staged(out):
    import narwhal_amd
    from narwhal_amd import _lib
    eng = narwhal_amd.Engine(device=0, flags=_lib.NWV_FLAG_MSM_ALWAYS)
    guarded(out, "staged", lambda: case_staged(eng, False))
    guarded(out, "staged_keyed", lambda: case_staged(eng, True))
    eng.close()


def part_other(out):
    import narwhal_amd
    from narwhal_amd import _lib
    eng = narwhal_amd.Engine(device=0, flags=_lib.NWV_FLAG_MSM_ALWAYS)
    guarded(out, "digests", lambda: case_digests(eng))
    guarded(out, "aggregate", lambda: case_aggregate(eng))
    keys, _, sigs, msgs = signed(eng, SPARSE_N, SPARSE_N, 9)
    run = batch_run(eng, keys, msgs)
    for k, pair in enumerate(SPARSE_PAIRS):
        guarded(out, "sparse_%d_%d" % pair,
                lambda: three_checks(eng, run, lambda f: list(zip(keys, f, msgs)), sigs, P=pair, tag=k))
    eng.close()
    part_staged(out)
    for n in (4, 64, 65, 1000):
        guarded(out, f"nocoeff_{n}", lambda: case_nocoeff(n))


def part_forms(out, flags):
    import narwhal_amd
    from narwhal_amd import _lib
    eng = narwhal_amd.Engine(device=0, flags=_lib.NWV_FLAG_MSM_ALWAYS | flags)
    sizes = FORMS_SIZES + ([FORMS_WIDE_N] if "NWV_MSM_TAIL_S" in os.environ else [])
    keys, _, sigs, msgs = signed(eng, max(sizes), max(sizes), 10)
    for n in sizes:
        def one(n=n):
            pk, sg, ms = keys[:n], sigs[:n], msgs[:n]
            r = three_checks(eng, batch_run(eng, pk, ms), lambda f: list(zip(pk, f, ms)), sg)
            p = plan(n, n)
            r["plan"] = {k: p[k] for k in ("widths", "seg", "tail_S", "tail_items", "narrow_top", "chunks")}
            r["plan_matches_engine"] = plan_matches(staged_stats(eng, pk, sg, ms), p)
            return r
        guarded(out, f"forms_{n}", one)
    eng.close()


def part_shard(out):
    """every range verifies with seed' = shard_seed(S, lo) and indices local to the range"""
    import narwhal_amd
    from ed_shard_gpu_check import _ranges
    eng = narwhal_amd.Engine(device=None, n_devices=0)
    n = 3137
    rg = _ranges(n, eng.device_count, int(os.environ.get("NWV_SHARD_MIN", "16384")))
    out["devices"], out["ranges"] = eng.device_count, rg
    for keyed in (False, True):
        def one(keyed=keyed):
            keys, kidx, sigs, msgs = signed(eng, n, 100 if keyed else n, 11 + keyed)
            run = keyed_run(eng, keys, kidx, msgs) if keyed else batch_run(eng, keys, msgs)
            c0 = eng.diag_counters_ex()
            ok, bits = run(sigs, S, True)
            r = {"valid_accepts": bool(ok) and all(bits)}
            local = list(sigs)
            for lo, hi in rg:
                local[lo:hi] = zc.cancelling(sigs[lo:hi], range(hi - lo), zc.shard_seed(S, lo), random.Random(lo))
            r["touched_differ"] = all(a != b for a, b in zip(local, sigs))
            c1 = eng.diag_counters_ex()
            r["local_accepts_nobits"] = bool(run(local, S, False)[0])
            ok, bits = run(local, S, True)
            r["local_accepts_bits"] = bool(ok) and all(bits)
            r["no_fallback"] = eng.diag_counters_ex()["each"] == c1["each"]
            r["local_other_rejects"] = not run(local, S_OTHER, False)[0]
            ok, bits = run(local, S_LAST, True)
            r["local_last_bit_rejects"] = (not ok) and not any(bits)
            # built as one range would use them (the caller's seed, global indices): every range
            # but the first has another seed and other indices, and the first's share of the sum
            # does not vanish alone
            glob = zc.cancelling(sigs, range(n), S, random.Random(n))
            r["global_rejects_nobits"] = not run(glob, S, False)[0]
            ok, bits = run(glob, S, True)
            r["global_rejects_bits"] = (not ok) and not any(bits)
            # the same coefficients passed explicitly (zs): the shard rule spelled out once more
            zs = {}
            for lo, hi in rg:
                zs.update(zip(range(lo, hi), zc.z_many(zc.shard_seed(S, lo), range(hi - lo))))
            one_sum = zc.cancelling(sigs, range(n), S, random.Random(n + 1), zs=zs)
            r["one_sum_over_ranges_rejects"] = not run(one_sum, S, False)[0]  # each range's sum must vanish
            c2 = eng.diag_counters_ex()
            r["msm_runs"] = c2["msm"] - c0["msm"]
            return r
        guarded(out, "shard_keyed" if keyed else "shard_batch", one)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", required=True)
    ap.add_argument("--flags", type=int, default=0)
    a = ap.parse_args()
    out = {}
    for part in a.parts.split(","):
        if part == "forms":
            part_forms(out, a.flags)
        else:
            {"default": part_default, "keyed": part_keyed, "other": part_other, "staged": part_staged,
             "shard": part_shard}[part](out)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
