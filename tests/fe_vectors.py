"""Inputs and the integer reference for the field-multiply tests (tests/test_fe_seeded_hostemu.py,
tests/test_gpu_fe_seeded.py): ten-limb radix 2^25.5 elements of GF(2^255 - 19) as fe25519.h holds
them, and Python integers mod p as the reference."""
import numpy as np

P = 2**255 - 19
POS = (0, 26, 51, 77, 102, 128, 153, 179, 204, 230)
BITS = (26, 25) * 5
# fe_mul / fe_sq admit limbs up to 3.36 x 2^26 (even limbs) or 2^25 (odd limbs)
MAXLIMB = tuple(int(3.36 * (1 << b)) for b in BITS)
# a carried result: every limb within 1.01 of its width (fe25519.h "L")
OUTLIMB = tuple(int(1.01 * (1 << b)) for b in BITS)
NSQ = 250


def limbs_of(x):
    """the carried ten-limb form of an integer below 2^255"""
    return [(x >> POS[i]) & ((1 << BITS[i]) - 1) for i in range(10)]


def value(limbs):
    return sum(int(v) << POS[i] for i, v in enumerate(limbs))


def edge_elements():
    """0, 1, p - 1, 2^255 - 20, every limb at its admitted maximum and one below it, and every
    single-limb pattern at 1, the limb's width and the admitted maximum"""
    out = [limbs_of(0), limbs_of(1), limbs_of(P - 1), limbs_of(2**255 - 20), list(MAXLIMB),
           [m - 1 for m in MAXLIMB]]
    for i in range(10):
        for v in (1, (1 << BITS[i]) - 1, MAXLIMB[i]):
            e = [0] * 10
            e[i] = v
            out.append(e)
    return out


def random_elements(n, seed):
    """half carried (uniform below 2^255), half uncarried (every limb uniform up to its admitted
    maximum)"""
    rnd = np.random.default_rng(seed)
    out = []
    for k in range(n):
        if k % 2 == 0:
            out.append(limbs_of(int.from_bytes(rnd.bytes(32), "little") >> 1))
        else:
            out.append([int(rnd.integers(0, MAXLIMB[i] + 1)) for i in range(10)])
    return out


def operand_pairs(n_random, seed):
    """(a, b) limb arrays: every edge element against itself, the all-maximum element and a random
    one, then the random elements pairwise"""
    edges = edge_elements()
    rnd = random_elements(n_random, seed)
    a, b = [], []
    for i, e in enumerate(edges):
        for o in (e, list(MAXLIMB), rnd[i % len(rnd)]):
            a.append(e)
            b.append(o)
    for i, e in enumerate(rnd):
        a.append(e)
        b.append(rnd[(i * 7 + 3) % len(rnd)])
    return np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32)


def reference(a, b):
    """[(a b, a^2, a^(2^NSQ)) mod p] per row"""
    out = []
    for ra, rb in zip(a, b):
        x, y = value(ra), value(rb)
        out.append((x * y % P, x * x % P, pow(x, 1 << NSQ, P)))
    return out


def check(a, b, mul, sq, sqn, ref=None):
    """every result equals the reference mod p and is carried (limbs within 1.01 of their width)"""
    ref = ref or reference(a, b)
    for k, (wm, ws, wq) in enumerate(ref):
        for name, got, want in (("mul", mul[k], wm), ("sq", sq[k], ws), ("sqn", sqn[k], wq)):
            assert value(got) % P == want, (name, k, list(a[k]), list(b[k]))
            assert all(int(v) <= OUTLIMB[i] for i, v in enumerate(got)), (name, k, list(got))
