"""Inputs for the key cache / comb table tests (tests/test_gpu_keycache.py, its child process
tests/keycache_gpu_check.py): keyed batches whose wrong answer would be a slot or a table shared by
two keys.  Pure Python over the oracle (no engine), so the conditions on the inputs are checked on
a machine without a GPU (tests/test_keycache_cases_host.py).

A case is (keys, key_idx, sigs, msgs, want): the key list, the key of every signature, the
signatures, the messages, and the oracle's verdicts.  A committee is (signing seeds, public keys).
Every builder returns a new case and leaves its argument alone."""
import random

import oracle_ffi as of
from test_gpu_comb import MSG_LENS, _forge_set
from test_gpu_tiny import _forge


def committee(m, seed):
    rnd = random.Random(seed)
    seeds = [rnd.randbytes(32) for _ in range(m)]
    return seeds, [of.pubkey(s) for s in seeds]


def verdicts(keys, kidx, sigs, msgs):
    return [of.verify(keys[k], s, m) for k, s, m in zip(kidx, sigs, msgs)]


def valid(com, n, seed, signers=None):
    """n honest signatures by the committee (by its members `signers` only, if given)"""
    seeds, keys = com
    rnd = random.Random(seed)
    who = list(signers) if signers is not None else list(range(len(keys)))
    kidx = [rnd.choice(who) for _ in range(n)]
    msgs = [rnd.randbytes(rnd.choice(MSG_LENS)) for _ in range(n)]
    sigs = [of.sign(seeds[k], m) for k, m in zip(kidx, msgs)]
    return list(keys), kidx, sigs, msgs, verdicts(keys, kidx, sigs, msgs)


def wrong_signer(case, positions, to=None):
    """key_idx[i] renamed to another key of the list (to[j] for positions[j], else the next index
    with other bytes); the signature is untouched"""
    keys, kidx, sigs, msgs, _ = case
    kidx = list(kidx)
    for j, i in enumerate(positions):
        if to is not None:
            t = to[j]
        else:
            t = next(k % len(keys) for k in range(kidx[i] + 1, kidx[i] + len(keys))
                     if keys[k % len(keys)] != keys[kidx[i]])
        assert keys[t] != keys[kidx[i]]
        kidx[i] = t
    return list(keys), kidx, list(sigs), list(msgs), verdicts(keys, kidx, sigs, msgs)


def swapped_key_bytes(case, a, b):
    """entries a and b of the key list exchanged, key_idx as it was: every signature by either fails"""
    keys, kidx, sigs, msgs, _ = case
    keys = list(keys)
    assert keys[a] != keys[b]
    keys[a], keys[b] = keys[b], keys[a]
    return keys, list(kidx), list(sigs), list(msgs), verdicts(keys, kidx, sigs, msgs)


def one_byte_variants(seed, pad=0):
    """K a signing key; keys = [K, K_0 .. K_31, K_sign], K_j = K with bit 0 of byte j flipped (many
    do not decode), K_sign = K with bit 255 flipped.  33 signatures by K named under K_j / K_sign,
    then 5 (+ pad) honest ones under K."""
    rnd = random.Random(seed)
    sk = rnd.randbytes(32)
    K = of.pubkey(sk)
    keys = [K] + [K[:j] + bytes([K[j] ^ 1]) + K[j + 1:] for j in range(32)] + [K[:31] + bytes([K[31] ^ 0x80])]
    assert len(set(keys)) == 34
    kidx = list(range(1, 34)) + [0] * (5 + pad)
    msgs = [rnd.randbytes(rnd.choice(MSG_LENS)) for _ in kidx]
    sigs = [of.sign(sk, m) for m in msgs]
    return keys, kidx, sigs, msgs, verdicts(keys, kidx, sigs, msgs)


def duplicate_key_list(case):
    """the busiest signer's bytes appended to the key list as a second index (the last), named by
    every other one of that signer's signatures"""
    keys, kidx, sigs, msgs, _ = case
    d = max(set(kidx), key=lambda k: (kidx.count(k), -k))
    assert kidx.count(d) >= 2
    keys, kidx = list(keys) + [keys[d]], list(kidx)
    for j, i in enumerate([i for i, k in enumerate(kidx) if k == d]):
        if j % 2:
            kidx[i] = len(keys) - 1
    return keys, kidx, list(sigs), list(msgs), verdicts(keys, kidx, sigs, msgs)


def forged(case, seed, extra=(), wrong=0):
    """R / s / message / s + l forgeries in turn (test_gpu_comb._forge_set above 64 signatures:
    indices 0, 63, 64, n - 1 and n // 7 others; below, 1 + n // 5 random indices as test_gpu_tiny
    does), the indices `extra` forged too, then wrong_signer at the first `wrong` positions that
    are still honest"""
    keys, kidx, sigs, msgs, _ = case
    sigs, msgs = list(sigs), list(msgs)
    n = len(sigs)
    if n > 64:
        bad, _ = _forge_set(keys, kidx, sigs, msgs, seed)
    else:
        bad = sorted(random.Random(seed).sample(range(n), min(n, 1 + n // 5)))
        for j, i in enumerate(bad):
            sigs[i], msgs[i] = _forge(sigs[i], msgs[i], j % 4)
    for j, i in enumerate(x for x in extra if x < n and x not in bad):
        sigs[i], msgs[i] = _forge(sigs[i], msgs[i], j % 4)
    out = list(keys), list(kidx), sigs, msgs, verdicts(keys, kidx, sigs, msgs)
    return wrong_signer(out, honest_positions(out, wrong)) if wrong else out


def signed_by(case, com, i, k):
    """signature i made again, honestly, by member k of the committee the key list starts with"""
    keys, kidx, sigs, msgs, _ = case
    assert keys[k] == com[1][k]
    kidx, sigs = list(kidx), list(sigs)
    kidx[i], sigs[i] = k, of.sign(com[0][k], msgs[i])
    return list(keys), kidx, sigs, list(msgs), verdicts(keys, kidx, sigs, msgs)


def joined(*coms):
    """one committee out of several, in order"""
    return sum((c[0] for c in coms), []), sum((c[1] for c in coms), [])


def forge_one(case, i, kind=1):
    keys, kidx, sigs, msgs, _ = case
    sigs, msgs = list(sigs), list(msgs)
    sigs[i], msgs[i] = _forge(sigs[i], msgs[i], kind)
    return list(keys), list(kidx), sigs, msgs, verdicts(keys, kidx, sigs, msgs)


def honest_positions(case, k):
    """the first k positions whose oracle verdict is True (where a wrong signer adds a rejection)"""
    out = [i for i, w in enumerate(case[4]) if w][:k]
    assert len(out) == k
    return out
