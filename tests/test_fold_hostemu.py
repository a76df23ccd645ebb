"""k_msm_prep's second trimming on the host (tests/hostemu/fold_hostemu.cpp, built with
NWV_BOUNDS_CHECK), against Python integers:

* sc_reduce512_fold / sc_reduce384_fold: the canonical residue mod l, word for word sc_reduce512's;
* the hash workgroup's unreduced sum of z_i s_i (13 words) and the one reduction of a batch's
  partials (msm_zs_partial, msm_zs_total);
* msm_recode_rows: the digits of msm_recode, for every layout the window plan can choose;
* ge_decompress_stash: the verdict and the point of ge_decompress.
The device's code paths are checked by tests/test_gpu_fold.py."""
import ctypes
import json
import os

import numpy as np
import pytest

import fe_vectors as fv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "_build", "libfoldemu.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")
L = 2**252 + 27742317777372353535851937790883648493
MAXW = 48  # MSM_MAX_WINDOWS


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        import subprocess
        subprocess.run(["make", "-C", ROOT, "tests/_build/libfoldemu.so"], check=True)
    so = ctypes.CDLL(LIB_PATH)
    vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    so.he_fold_reduce512.argtypes = [u32, vp, vp, vp]
    so.he_fold_reduce384.argtypes = [u32, vp, vp, vp]
    so.he_fold_zmul.argtypes = [u32, vp, vp, vp, vp, vp]
    so.he_fold_partial.argtypes = [u32, vp, vp, vp]
    so.he_fold_total.argtypes = [u32, vp, vp]
    so.he_fold_layout.argtypes = [i32, i32, i32, i32, vp, vp, vp]
    so.he_fold_layout.restype = i32
    so.he_fold_recode.argtypes = [i32, i32, i32, i32, i32, u32, vp, vp, vp]
    so.he_fold_recode.restype = i32
    so.he_fold_decompress.argtypes = [u32, vp, vp, vp, vp, vp]
    so.he_fold_decompress.restype = i32
    return so


def words(values, nwords):
    return np.frombuffer(b"".join(int(v).to_bytes(4 * nwords, "little") for v in values), dtype=np.uint32).copy()


def ints(arr, nwords):
    b = arr.tobytes()
    return [int.from_bytes(b[4 * nwords * i:4 * nwords * (i + 1)], "little") for i in range(len(arr) // nwords)]


def reduction_inputs(bits, top, seed):
    """the edges of a `bits`-bit reduction (values up to `top`) and 10^4 seeded random values"""
    v = [0, 1, L - 1, L, L + 1, 2 * L - 1, 2**252 - 1, 2**252, top]
    for k in (top // L, top // L - 1, 2**(bits - 253) + 12345, 2**(bits - 300) + 1, 2**128 - 1, 3):
        v += [k * L - 1, k * L, k * L + 1]
    rnd = np.random.default_rng(seed)
    v += [int.from_bytes(rnd.bytes(bits // 8), "little") for _ in range(10000)]
    # random values of every length, so every word count of the quotient occurs
    v += [int.from_bytes(rnd.bytes(bits // 8), "little") >> int(rnd.integers(0, bits)) for _ in range(2000)]
    assert all(0 <= x <= top for x in v)
    return v


def test_fold_reduction_of_512_bit_values(lib):
    v = reduction_inputs(512, 2**512 - 1, 512)
    x = words(v, 16)
    fold, barrett = np.zeros(8 * len(v), np.uint32), np.zeros(8 * len(v), np.uint32)
    lib.he_fold_reduce512(len(v), x.ctypes.data, fold.ctypes.data, barrett.ctypes.data)
    assert ints(fold, 8) == [a % L for a in v]
    assert np.array_equal(fold, barrett)


def test_fold_reduction_of_384_bit_values(lib):
    """up to 2^384 - 1, which covers the largest product (2^128 - 1)(l - 1) of a coefficient and a
    reduced scalar (an edge of its own)"""
    v = reduction_inputs(384, 2**384 - 1, 384) + [(2**128 - 1) * (L - 1), (2**128 - 1) * (L - 1) - 1]
    x = words(v, 12)
    fold, barrett = np.zeros(8 * len(v), np.uint32), np.zeros(8 * len(v), np.uint32)
    lib.he_fold_reduce384(len(v), x.ctypes.data, fold.ctypes.data, barrett.ctypes.data)
    assert ints(fold, 8) == [a % L for a in v]
    assert np.array_equal(fold, barrett)


def test_coefficient_times_scalar(lib):
    """the 4 x 8 product is the exact integer, and folded it is sc_mul's canonical z k mod l"""
    rnd = np.random.default_rng(48)
    zs = [1, 2**128 - 1, 2**127 + 1, 2**128 - 1, 1] + [int.from_bytes(rnd.bytes(16), "little") | 1 for _ in range(2000)]
    bs = [L - 1, L - 1, 2**256 - 1, 0, 2**252] + [int.from_bytes(rnd.bytes(32), "little") % L for _ in range(2000)]
    z, b = words(zs, 4), words(bs, 8)
    prod = np.zeros(12 * len(zs), np.uint32)
    a, ref = np.zeros(8 * len(zs), np.uint32), np.zeros(8 * len(zs), np.uint32)
    lib.he_fold_zmul(len(zs), z.ctypes.data, b.ctypes.data, prod.ctypes.data, a.ctypes.data, ref.ctypes.data)
    assert ints(prod, 12) == [p * q for p, q in zip(zs, bs)]
    assert ints(a, 8) == [p * q % L for p, q in zip(zs, bs)]
    assert np.array_equal(a, ref)
    assert all(r < 2**253 for r in ints(a, 8))  # what the window layout assumes


def partial_of(lib, zs, ss):
    out = np.zeros(13, np.uint32)
    z, s = words(zs, 4), words(ss, 8)
    lib.he_fold_partial(len(zs), z.ctypes.data, s.ctypes.data, out.ctypes.data)
    return ints(out, 13)[0]


def total_of(lib, partials):
    p = words(partials, 13)
    r = np.zeros(8, np.uint32)
    lib.he_fold_total(len(partials), p.ctypes.data, r.ctypes.data)
    return ints(r, 8)[0]


def test_wide_partial_of_a_full_workgroup(lib):
    """256 lanes, all with z = 2^128 - 1 and s = l - 1: the exact 13-word integer; and the largest
    the lanes can hold at all (s = 2^256 - 1, a non-canonical s the fail flag reports)"""
    assert partial_of(lib, [2**128 - 1] * 256, [L - 1] * 256) == 256 * (2**128 - 1) * (L - 1)
    assert partial_of(lib, [2**128 - 1] * 256, [2**256 - 1] * 256) == 256 * (2**128 - 1) * (2**256 - 1)
    rnd = np.random.default_rng(13)
    for nt in (1, 64, 255, 256):
        zs = [int.from_bytes(rnd.bytes(16), "little") | 1 for _ in range(nt)]
        ss = [int.from_bytes(rnd.bytes(32), "little") % L for _ in range(nt)]
        assert partial_of(lib, zs, ss) == sum(a * b for a, b in zip(zs, ss))


def test_partials_combined_by_the_consumer(lib):
    """many partials, the largest ones included, reduced once by msm_zs_total: the Python value
    mod l (8,192 workgroups of 256 = 2,097,152 signatures)"""
    big = 256 * (2**128 - 1) * (L - 1)
    assert total_of(lib, [big]) == big % L
    assert total_of(lib, [big] * 8192) == 8192 * big % L
    assert total_of(lib, [256 * (2**128 - 1) * (2**256 - 1)] * 65535) == 65535 * 256 * (2**128 - 1) * (2**256 - 1) % L
    assert total_of(lib, [0] * 5) == 0
    rnd = np.random.default_rng(14)
    ps = [int.from_bytes(rnd.bytes(49), "little") for _ in range(1000)]  # < 2^392
    assert total_of(lib, ps) == sum(ps) % L
    # end to end: lanes -> partials -> total
    zs = [int.from_bytes(rnd.bytes(16), "little") | 1 for _ in range(600)]
    ss = [int.from_bytes(rnd.bytes(32), "little") % L for _ in range(600)]
    parts = [partial_of(lib, zs[o:o + 256], ss[o:o + 256]) for o in range(0, 600, 256)]
    assert total_of(lib, parts) == sum(a * b for a, b in zip(zs, ss)) % L


def layout(lib, c_lo, c_hi, narrow, zonly):
    nwz = ctypes.c_int(0)
    width, pos = np.zeros(MAXW, np.uint8), np.zeros(MAXW, np.uint16)
    nw = lib.he_fold_layout(c_lo, c_hi, narrow, zonly, ctypes.byref(nwz), width.ctypes.data, pos.ctypes.data)
    return nw, nwz.value, width[:nw].tolist(), pos[:nw].tolist()


def carry_everywhere(width, pos, nbits):
    """scalars whose recoding carries out of every window: every window's top bit set, every
    window all ones, and every window exactly half (the carry threshold itself)"""
    top = sum(1 << (p + c - 1) for c, p in zip(width, pos) if p + c - 1 < nbits)
    ones = (1 << nbits) - 1
    return [top, ones, top - 1 if top else 0]


# every layout msm_plan can choose: widths 6..15 for the z range and 3..15 above it, evenly spread
# or narrow-top (large batches), and the z-only layout of the split (key cache) form; (13, 13)
# narrow-top is the headline's, (8, 6) evenly spread a small batch's
LAYOUTS = [(lo, hi, nt, 0) for lo in range(6, 16) for hi in range(3, 16) for nt in (0, 1)] + \
          [(lo, 3, 0, 1) for lo in range(6, 16)]


def test_layouts_include_the_named_ones(lib):
    assert (13, 13, 1, 0) in LAYOUTS and (13, 13, 0, 0) in LAYOUTS and (8, 6, 0, 0) in LAYOUTS and (12, 3, 0, 1) in LAYOUTS
    nw, nwz, width, pos = layout(lib, 13, 13, 1, 0)
    assert (nw, nwz) == (20, 10) and sum(width) == 254 and sum(width[:nwz]) == 129


def test_recoding_matches_the_old_function_for_every_layout(lib):
    rnd = np.random.default_rng(253)
    rand_full = [int.from_bytes(rnd.bytes(32), "little") % L for _ in range(24)]
    rand_z = [int.from_bytes(rnd.bytes(16), "little") | 1 for _ in range(24)]
    checked = 0
    for c_lo, c_hi, narrow, zonly in LAYOUTS:
        nw, nwz, width, pos = layout(lib, c_lo, c_hi, narrow, zonly)
        if nw == 0:
            continue
        for zrange in (0, 1):
            if zrange:  # the z_i (and a key's 128-bit halves): windows [0, nw_z)
                n_w, nbits = nwz, 128
                vals = [0, 1, 2**128 - 1, 2**127, 2**127 + 1] + carry_everywhere(width[:nwz], pos[:nwz], 128) + rand_z
            elif zonly:
                continue
            else:  # scalars mod l: every window
                n_w, nbits = nw, 253
                vals = [0, 1, L - 1, 2**128 - 1, 2**253 - 1, 2**252] + carry_everywhere(width, pos, 253) + rand_full
            s = words(vals, 8)
            fresh = np.full(len(vals) * MAXW, 0x7fff, np.int16)
            old = np.full(len(vals) * MAXW, 0x7fff, np.int16)
            ok = lib.he_fold_recode(c_lo, c_hi, narrow, zonly, zrange, len(vals), s.ctypes.data,
                                    fresh.ctypes.data, old.ctypes.data)
            assert ok == 1, (c_lo, c_hi, narrow, zonly, zrange)
            assert np.array_equal(fresh, old), (c_lo, c_hi, narrow, zonly, zrange)
            # and both are the scalar: sum of d_w 2^pos_w, every digit in its window's range
            d = fresh.reshape(len(vals), MAXW)[:, :n_w].astype(object)
            for row, v in zip(d, vals):
                assert sum(int(x) << p for x, p in zip(row, pos)) == v
                for w, x in enumerate(row):
                    half = 1 << (width[w] - 1)
                    assert (0 <= x <= half) if w == n_w - 1 else (-half <= x < half)
            checked += 1
    assert checked >= 2 * 200


def test_stash_decompression_matches_ge_decompress(lib):
    """every key and R of the golden vectors, every ZIP-215 small-order encoding, the x = 0 points
    with either sign bit, y >= p, and seeded random encodings (about half are non-squares)"""
    with open(os.path.join(GOLDEN, "ed25519_vectors.json")) as f:
        g = json.load(f)
    with open(os.path.join(GOLDEN, "zip215_small_order.json")) as f:
        z = json.load(f)
    enc = []
    for v in g["vectors"]:
        enc += [bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"])[:32]]
    enc += [bytes.fromhex(e) for e in z["encodings"]]
    one, minus_one = (1).to_bytes(32, "little"), (fv.P - 1).to_bytes(32, "little")
    for e in (one, minus_one):
        enc += [e, e[:31] + bytes([e[31] | 0x80])]
    enc += [(fv.P + k).to_bytes(32, "little") for k in (0, 1, 3, 18)]  # y >= p
    enc += [(2**255 - 1).to_bytes(32, "little"), (2**256 - 1).to_bytes(32, "little")]
    rnd = np.random.default_rng(58)
    enc += [rnd.bytes(32) for _ in range(300)]
    enc = list(dict.fromkeys(enc))
    n = len(enc)
    buf = np.frombuffer(b"".join(enc), dtype=np.uint8)
    ok, ok_ref = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    rec, rec_ref = np.zeros(32 * n, np.uint32), np.zeros(32 * n, np.uint32)
    clean = lib.he_fold_decompress(n, buf.ctypes.data, ok.ctypes.data, rec.ctypes.data, ok_ref.ctypes.data,
                                   rec_ref.ctypes.data)
    assert clean == 1
    assert np.array_equal(ok, ok_ref)
    assert 0 < int(ok.sum()) < n  # both outcomes occur
    for i in range(n):
        if not ok[i]:
            continue
        for k in range(3):  # y + x, y - x, 2 d x y as field elements
            a = fv.value(rec[32 * i + 10 * k:32 * i + 10 * k + 10]) % fv.P
            b = fv.value(rec_ref[32 * i + 10 * k:32 * i + 10 * k + 10]) % fv.P
            assert a == b, (enc[i].hex(), k)
