"""The comb pass kernel's per-signature arithmetic (narwhal_amd/csrc/comb_kernels.hip
k_ed_comb_pass4 / k_ed_comb_pass16, lane functions in comb.h) run on the host
(tests/hostemu/comb_pass_hostemu.cpp) in the kernel's own order: sixteen signatures a workgroup
hashed side by side, their R's decompressed four a wave, each signature's comb sum walked by L
lanes over 64 / L digit positions each and joined level by level, for both L the library ships.
Verdicts against the oracle's ZIP-215 verdicts; every lane-joined sum against comb_term's 64-term
sum (k_ed_comb's) and, where the scalar is known, against a plain double-and-add product.  The GPU
kernel is checked by tests/test_gpu_comb_pass.py."""
import ctypes
import os
import random

import numpy as np
import pytest

import oracle_ffi as of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PE_PATH = os.path.join(ROOT, "tests", "_build", "libcombpassemu.so")
L_ORDER = 2**252 + 27742317777372353535851937790883648493
P_FIELD = 2**255 - 19
LANES = [4, 16]


@pytest.fixture(scope="module")
def pe():
    if not os.path.exists(PE_PATH):
        import subprocess
        subprocess.run(["make", "-C", ROOT, "tests/_build/libcombpassemu.so"], check=True)
    lib = ctypes.CDLL(PE_PATH)
    vp = ctypes.c_void_p
    lib.he_comb_pass_verify.argtypes = [ctypes.c_int, ctypes.c_uint32, vp, vp, vp, vp, vp, vp]
    lib.he_comb_pass_forced_k.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                          ctypes.c_int, vp]
    lib.he_comb_pass_digits.argtypes = [ctypes.c_int, ctypes.c_char_p, vp, vp, ctypes.c_char_p, vp]
    assert lib.he_comb_pass_group() == 16
    return lib


def pass_verify(pe, L, items):
    n = len(items)
    pk = np.frombuffer(b"".join(p for p, _, _ in items) + b"\0" * 16, dtype=np.uint8)
    sg = np.frombuffer(b"".join(s for _, s, _ in items) + b"\0" * 16, dtype=np.uint8)
    msgs = [m for _, _, m in items]
    lens = np.array([len(m) for m in msgs], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    arena = np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8)
    out = np.full(n, 7, dtype=np.uint8)
    rc = pe.he_comb_pass_verify(L, n, pk.ctypes.data, sg.ctypes.data, arena.ctypes.data, offs.ctypes.data,
                                lens.ctypes.data, out.ctypes.data)
    assert rc == 0  # (-1: a digit past a table; -2: a lane-joined sum that is not the 64-term sum)
    assert set(out.tolist()) <= {0, 1}
    return [bool(v) for v in out]


def _vectors():
    vecs = [(bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"]))
            for v in of.load_golden("ed25519_vectors.json")["vectors"]]
    vecs += [(bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"]))
             for v in of.load_golden("zip215_small_order.json")["vectors"]]
    return vecs


def _undecodable(rnd):
    """a 32-byte string that is no point encoding: y with (y^2 - 1) / (d y^2 + 1) a non-square"""
    d = -121665 * pow(121666, -1, P_FIELD) % P_FIELD
    while True:
        y = rnd.randrange(P_FIELD)
        x2 = (y * y - 1) * pow(d * y * y + 1, -1, P_FIELD) % P_FIELD
        if x2 and pow(x2, (P_FIELD - 1) // 2, P_FIELD) != 1:
            return y.to_bytes(32, "little")


@pytest.mark.parametrize("L", LANES)
def test_every_vector_matches_oracle(pe, L):
    """every golden vector (every Appendix-B category) and the 196-case small-order table as ONE
    pass, so the rows of a decompression wave hold unrelated, partly undecodable R's; undecodable
    keys (the identity's table) and s >= l included"""
    vecs = _vectors()
    want = [of.verify(*v) for v in vecs]
    assert set(want) == {True, False} and len(vecs) > 300
    got = pass_verify(pe, L, vecs)
    bad = [(p.hex(), s.hex()) for (p, s, _), g, w in zip(vecs, got, want) if g != w]
    assert not bad, bad[:3]


@pytest.mark.parametrize("L", LANES)
def test_undecodable_points_and_s_at_the_order(pe, L):
    rnd = random.Random(11)
    seed = rnd.randbytes(32)
    pk, m = of.pubkey(seed), b"edge"
    sig = of.sign(seed, m)
    junk = _undecodable(rnd)
    s = int.from_bytes(sig[32:], "little")
    items = [(pk, sig, m),
             (pk, junk + sig[32:], m),                                   # R does not decode
             (junk, sig, m),                                             # A does not decode
             (junk, junk + sig[32:], m),
             (pk, sig[:32] + L_ORDER.to_bytes(32, "little"), m),         # s = l
             (pk, sig[:32] + (L_ORDER - 1).to_bytes(32, "little"), m),   # s = l - 1: canonical, wrong
             (pk, sig[:32] + (s + L_ORDER).to_bytes(32, "little"), m)]   # s + l: right residue, not canonical
    want = [of.verify(*it) for it in items]
    assert want == [True] + [False] * 6
    assert pass_verify(pe, L, items) == want


@pytest.mark.parametrize("L", LANES)
def test_one_bit_flips(pe, L):
    """random valid signatures with one bit flipped in R, s, A and the message; 24 signatures: one
    full workgroup and half of the next"""
    rnd = random.Random(13)
    items = []
    for j in range(12):
        seed = rnd.randbytes(32)
        m = rnd.randbytes(rnd.choice([1, 32, 47, 48, 111, 112, 200]))
        pk, sig = of.pubkey(seed), of.sign(seed, m)
        items.append((pk, sig, m))
        bit = rnd.randrange(256)
        flip = lambda b, i: b[:i // 8] + bytes([b[i // 8] ^ (1 << (i % 8))]) + b[i // 8 + 1:]
        kind = j % 4
        if kind == 0:
            items.append((pk, flip(sig, bit), m))
        elif kind == 1:
            items.append((pk, flip(sig, 256 + bit % 252), m))
        elif kind == 2:
            items.append((flip(pk, bit), sig, m))
        else:
            items.append((pk, sig, flip(m, bit % (8 * len(m)))))
    want = [of.verify(*it) for it in items]
    assert want[::2] == [True] * 12 and not any(want[1::2])
    assert pass_verify(pe, L, items) == want


def _digits(x):
    """msm.h comb_digits restated: signed radix-16 digits of x < 2^253"""
    d, carry = [], 0
    for j in range(64):
        v = ((x >> (4 * j)) & 15) + carry
        carry = 0
        if j + 1 < 64 and v >= 8:
            v -= 16
            carry = 1
        d.append(v)
    assert sum(v << (4 * j) for j, v in enumerate(d)) == x
    return d


@pytest.mark.parametrize("L", LANES)
def test_forced_challenge_scalars(pe, L):
    """k fed straight to the recoding and the lane sums, with s = r + k a so the equation holds for
    it, and s + 1 so it misses: the kernel form's verdict, its sum against comb_term's and against
    double-and-add.  k = 0 leaves every lane of A's comb on the neutral record."""
    rnd = random.Random(17)
    ks = [0, 1, 2, L_ORDER - 1, L_ORDER // 2, 2**252]
    ks += [rnd.randrange(L_ORDER) for _ in range(1000)]
    out = np.zeros(4, dtype=np.int32)
    for j, k in enumerate(ks):
        a, r = rnd.randrange(1, L_ORDER), rnd.randrange(1, L_ORDER)
        spoil = 1 if (j >= 6 and j % 8 == 0) else 0
        for sp in ([0, 1] if j < 6 else [spoil]):
            rc = pe.he_comb_pass_forced_k(L, k.to_bytes(32, "little"), a.to_bytes(32, "little"),
                                          r.to_bytes(32, "little"), sp, out.ctypes.data)
            assert rc == 0 and out[3] == 0, (k, rc)
            assert out[1] == 1, hex(k)
            assert out[0] == 1 - sp, (hex(k), sp, out.tolist())


def _run_digits(pe, L, a, ds, dk):
    """digits fed straight to the lane sums -> idle lanes; asserts the sum is comb_term's, is
    [sum (ds_j - dk_j a) 16^j]B, and that the check accepts exactly that R"""
    e = sum((s - k * a) << (4 * j) for j, (s, k) in enumerate(zip(ds, dk))) % L_ORDER
    out = np.zeros(5, dtype=np.int32)
    dsa, dka = np.array(ds, dtype=np.int32), np.array(dk, dtype=np.int32)
    rc = pe.he_comb_pass_digits(L, a.to_bytes(32, "little"), dsa.ctypes.data, dka.ctypes.data,
                                e.to_bytes(32, "little"), out.ctypes.data)
    assert rc == 0
    assert out[:4].tolist() == [1, 1, 1, 1], (ds, dk, out.tolist())
    return int(out[4])


@pytest.mark.parametrize("L", LANES)
def test_lane_sequential_edges(pe, L):
    """the cases the lane-sequential form adds"""
    rnd = random.Random(19)
    a = rnd.randrange(1, L_ORDER)
    P = 64 // L
    zero = [0] * 64
    # every lane of the signature at zero: the sum is the identity, [8] R must be the identity
    assert _run_digits(pe, L, a, zero, zero) == L
    # one lane whose every digit is zero (each lane in turn for L = 4, a spread for L = 16)
    for t in range(0, L, max(1, L // 4)):
        ds = [rnd.randrange(-8, 8) or 1 for _ in range(64)]
        dk = [rnd.randrange(-8, 8) or 1 for _ in range(64)]
        ds[63] = dk[63] = 1
        for p in range(P):
            ds[P * t + p] = dk[P * t + p] = 0
        assert _run_digits(pe, L, a, ds, dk) == 1
    # a lane whose first non-zero digit is its last position (B's comb, A's comb, both)
    for t in (0, L // 2, L - 1):
        for which in (1, 2, 3):
            ds = [rnd.randrange(-8, 8) for _ in range(64)]
            dk = [rnd.randrange(-8, 8) for _ in range(64)]
            ds[63] = dk[63] = 0
            for p in range(P):
                ds[P * t + p] = dk[P * t + p] = 0
            if which & 1:
                ds[P * t + P - 1] = -3
            if which & 2:
                dk[P * t + P - 1] = 5
            _run_digits(pe, L, a, ds, dk)
    # only the first position of a lane (the seeded record alone), only one lane live
    ds, dk = list(zero), list(zero)
    ds[P * (L - 1)] = 7
    assert _run_digits(pe, L, a, ds, dk) == L - 1
    ds, dk = list(zero), list(zero)
    dk[P * 1] = -8
    assert _run_digits(pe, L, a, ds, dk) == L - 1
    # digits all +8 and all -8 (entry 8 of every table, both signs, both combs)
    for v in (8, -8):
        _run_digits(pe, L, a, [v] * 64, [v] * 64)
        _run_digits(pe, L, a, [v] * 64, [-v] * 64)
        _run_digits(pe, L, a, [v] * 64, zero)
        _run_digits(pe, L, a, zero, [v] * 64)


@pytest.mark.parametrize("L", LANES)
def test_recoding_carries_out_of_every_position(pe, L):
    """s and k whose recoding carries out of every position below the top: nibbles of 8..15 all the
    way up (0x0888...8, 0x0fff...f, and a random mix of 8..15), through the forced-k entry"""
    rnd = random.Random(23)
    out = np.zeros(4, dtype=np.int32)
    carried = [int("0" + "8" * 63, 16), int("0" + "f" * 63, 16),
               int("0" + "".join(rnd.choice("89abcdef") for _ in range(63)), 16)]
    for x in carried:
        assert x < L_ORDER
        d = _digits(x)
        # position j carried iff digits 0..j stand for the low nibbles minus 16^(j + 1)
        for j in range(63):
            assert sum(v << (4 * i) for i, v in enumerate(d[:j + 1])) == (x & (16**(j + 1) - 1)) - 16**(j + 1)
    a = rnd.randrange(1, L_ORDER)
    for k in carried:
        for s in carried:
            # s = r + k a  ->  r = s - k a: both recodings carry at every position
            r = (s - k * a) % L_ORDER
            for sp in (0, 1):
                if sp and (s + 1) % L_ORDER != s + 1:
                    continue
                rc = pe.he_comb_pass_forced_k(L, k.to_bytes(32, "little"), a.to_bytes(32, "little"),
                                              r.to_bytes(32, "little"), sp, out.ctypes.data)
                assert rc == 0 and out[3] == 0
                assert out[1] == 1 and out[0] == 1 - sp, (hex(k), hex(s), sp, out.tolist())


@pytest.mark.parametrize("L", LANES)
def test_random_batch_with_forgeries_off_the_workgroup_multiple(pe, L):
    """70 signatures by a 10-key committee (four full workgroups and six signatures: the last
    workgroup's second decompression wave holds two), forgeries of each kind"""
    rnd = random.Random(70)
    seeds = [rnd.randbytes(32) for _ in range(10)]
    keys = [of.pubkey(s) for s in seeds]
    n = 70
    items = []
    for i in range(n):
        k = rnd.randrange(10)
        m = rnd.randbytes(rnd.choice([0, 1, 32, 47, 48, 111, 112, 200, 512]))
        items.append((keys[k], of.sign(seeds[k], m), m))
    bad = sorted(set([0, 15, 16, 63, 64, n - 1] + rnd.sample(range(n), 8)))
    for j, i in enumerate(bad):
        sg, m = bytearray(items[i][1]), items[i][2]
        kind = j % 4
        if kind == 0:
            sg[3] ^= 0x10
        elif kind == 1:
            sg[40] ^= 0x01
        elif kind == 2:
            m = bytes([m[0] ^ 0x80]) + m[1:] if m else b"\x01"
        else:
            sg[32:] = (int.from_bytes(bytes(sg[32:]), "little") + L_ORDER).to_bytes(32, "little")
        items[i] = (items[i][0], bytes(sg), m)
    want = [of.verify(*it) for it in items]
    assert [i for i, w in enumerate(want) if not w] == bad
    assert pass_verify(pe, L, items) == want
