"""The conditions on the inputs of tests/test_gpu_keycache.py, with the oracle alone
(tests/keycache_cases.py): a renamed or swapped position is rejected and nothing else is, the 33
one-byte variants of a key reject its signatures while the 5 under the key itself verify, and a
key list that repeats a key's bytes changes no verdict."""
import pytest

import keycache_cases as kc
import oracle_ffi as of

COM = kc.committee(10, 1)


def _rejected(case):
    return [i for i, w in enumerate(case[4]) if not w]


@pytest.mark.parametrize("n", [8, 64, 65, 300])
def test_valid_and_forged(n):
    case = kc.valid(COM, n, n)
    keys, kidx, sigs, msgs, want = case
    assert len(kidx) == len(sigs) == len(msgs) == len(want) == n and all(want)
    assert {len(m) for m in kc.valid(COM, 300, 2)[3]} == set(kc.MSG_LENS)
    f = kc.forged(case, 3 * n, extra=(5, 6))
    bad = _rejected(f)
    assert ({5, 6} if n <= 64 else {0, 5, 6, 63, 64, n - 1}) <= set(bad)
    assert len(bad) >= (1 + n // 5 if n <= 64 else 4 + n // 7) and len(bad) < n
    assert f[0] == keys and f[1] == kidx
    assert [i for i in range(n) if (f[2][i], f[3][i]) != (sigs[i], msgs[i])] == bad
    g = kc.forged(case, 3 * n, extra=(5, 6), wrong=2)
    assert sorted(set(_rejected(g)) - set(bad)) == kc.honest_positions(f, 2)
    assert case == kc.valid(COM, n, n)  # the builders leave their argument alone


@pytest.mark.parametrize("n", [8, 64, 65, 300])
def test_wrong_signer_rejects_exactly_the_renamed(n):
    case = kc.valid(COM, n, 10 + n)
    pos = [0, n // 2, n - 1]
    w = kc.wrong_signer(case, pos)
    assert _rejected(w) == pos
    assert w[0] == case[0] and w[2] == case[2] and w[3] == case[3]  # keys, signatures, messages untouched
    assert all(w[1][i] != case[1][i] for i in pos)
    w = kc.wrong_signer(case, [1], to=[(case[1][1] + 3) % 10])
    assert _rejected(w) == [1] and w[1][1] == (case[1][1] + 3) % 10


@pytest.mark.parametrize("n", [8, 64, 65, 300])
def test_swapped_key_bytes_rejects_both_signers(n):
    case = kc.valid(COM, n, 20 + n)
    a, b = case[1][0], next(k for k in case[1] if k != case[1][0])
    s = kc.swapped_key_bytes(case, a, b)
    hit = [i for i, k in enumerate(case[1]) if k in (a, b)]
    assert len(hit) >= 2 and _rejected(s) == hit
    assert sorted(s[0]) == sorted(case[0]) and s[1] == case[1] and s[2] == case[2]


@pytest.mark.parametrize("pad", [0, 32])
def test_one_byte_variants(pad):
    keys, kidx, sigs, msgs, want = kc.one_byte_variants(7, pad)
    assert len(keys) == 34 and len(sigs) == 38 + pad
    assert want == [False] * 33 + [True] * (5 + pad)
    assert sorted(kidx[:33]) == list(range(1, 34)) and set(kidx[33:]) == {0}
    for j in range(32):
        assert bytes(x ^ y for x, y in zip(keys[0], keys[1 + j])) == bytes(j) + b"\x01" + bytes(31 - j)
    assert bytes(x ^ y for x, y in zip(keys[0], keys[33])) == bytes(31) + b"\x80"
    # the same signatures under K itself all verify: only the key's name rejects them
    assert all(of.verify(keys[0], s, m) for s, m in zip(sigs, msgs))
    ok = [bool(of.lib().or_point_decompress_ok(k)) for k in keys]
    assert ok[0] and ok[33] and not all(ok) and any(ok[1:33])  # some variants decode, some do not


@pytest.mark.parametrize("n", [8, 100])
def test_duplicate_key_list_is_all_valid(n):
    case = kc.valid(COM, n, 30 + n)
    d = kc.duplicate_key_list(case)
    keys, kidx = d[0], d[1]
    assert all(d[4]) and len(keys) == 11 and keys[10] in keys[:10]
    first = keys.index(keys[10])
    assert kidx.count(10) >= 1 and kidx.count(first) >= 1
    assert [k if k != 10 else first for k in kidx] == case[1]
    for idx in (first, 10):  # one forged signature under each of the two indices
        i = kidx.index(idx)
        assert _rejected(kc.forge_one(d, i)) == [i]
