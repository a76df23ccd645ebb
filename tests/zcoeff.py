"""The batch MSM's coefficients restated outside the engine, and the forgery set that pins them.

z_i is the documented PRF (DESIGN.md section 3.1 "Coefficients", narwhal_amd/csrc/msm.h msm_z):
the first 16 bytes of ChaCha20(key = seed, counter = low word of i, nonce = high word of i ||
"nwv-" || "z128") with the low bit forced to 1.

cancelling() shifts s_i by e_i for every i in a position set P so that sum z_i e_i = 0 mod l.
R, A and M are untouched (every k_i is unchanged) and every touched signature is individually
invalid, yet the batch equation's error term -(sum z_i e_i) B vanishes exactly when the verifier's
z_i, for every i in P, is the documented one: the MSM must accept under the construction's seed
and reject under any other.  A truncated or colliding coefficient, a dropped index or a stale
seed breaks the cancellation.  (ed25519-consensus accepts the same batch given the same
coefficients; production callers pass no seed, so nobody can build one.)

Helper module: no test functions.  Used by test_zcoeff_host.py (host emulation) and
zcoeff_gpu_check.py (the device)."""
import numpy as np

L = 2**252 + 27742317777372353535851937790883648493
_SIGMA = (0x61707865, 0x3320646e, 0x79622d32, 0x6b206574)
NONCE_NWV, NONCE_Z128 = 0x2d76776e, 0x3832317a  # "nwv-", "z128" as little-endian words


def _rotl(v, n):
    return (v << np.uint32(n)) | (v >> np.uint32(32 - n))


def _qr(x, a, b, c, d):
    x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha20_blocks(key32, counter, n0, n1, n2):
    """RFC 8439 section 2.3 block function over arrays: counter, n0, n1, n2 are uint32 arrays (or
    scalars) broadcast to one block each -> uint32 [N, 16]"""
    cols = np.broadcast_arrays(*[np.atleast_1d(np.asarray(v, dtype=np.uint32)) for v in (counter, n0, n1, n2)])
    n = cols[0].shape[0]
    s = np.empty((16, n), dtype=np.uint32)
    for k in range(4):
        s[k] = _SIGMA[k]
    s[4:12] = np.frombuffer(bytes(key32), dtype="<u4").astype(np.uint32)[:, None]
    for k in range(4):
        s[12 + k] = cols[k]
    x = s.copy()
    for _ in range(10):
        _qr(x, 0, 4, 8, 12); _qr(x, 1, 5, 9, 13); _qr(x, 2, 6, 10, 14); _qr(x, 3, 7, 11, 15)
        _qr(x, 0, 5, 10, 15); _qr(x, 1, 6, 11, 12); _qr(x, 2, 7, 8, 13); _qr(x, 3, 4, 9, 14)
    return (x + s).T.copy()


def z_many(seed32, idx):
    """the documented z_i for every i of idx (any integer sequence; taken as uint64) -> list of int"""
    seed32 = bytes(seed32)
    if len(seed32) != 32:
        raise ValueError("seed must be 32 bytes")
    i = np.asarray(idx, dtype=np.uint64).reshape(-1)
    if i.size == 0:
        return []
    lo = (i & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (i >> np.uint64(32)).astype(np.uint32)
    blk = chacha20_blocks(seed32, lo, hi, NONCE_NWV, NONCE_Z128)
    w = blk[:, :4].copy()
    w[:, 0] |= np.uint32(1)
    raw = w.astype("<u4").tobytes()
    return [int.from_bytes(raw[16 * k:16 * k + 16], "little") for k in range(i.size)]


def cancelling(sigs, P, seed32, rng, zs=None):
    """sigs: list of 64-byte signatures; P: at least two distinct positions; rng: random.Random.
    -> a new list with s_i + e_i mod l at every i in P, where sum_{i in P} z_i e_i = 0 mod l and no
    e_i is zero.  zs (optional, indexable by position: a dict or a full-length list) gives the
    coefficients instead of z_many(seed32, P)."""
    P = [int(i) for i in P]
    if len(P) < 2 or len(set(P)) != len(P):
        raise ValueError("P needs at least two distinct positions")
    z = [int(zs[i]) for i in P] if zs is not None else z_many(seed32, P)
    while True:
        e = [rng.randrange(1, L) for _ in P[:-1]]
        acc = sum(zi * ei for zi, ei in zip(z, e)) % L
        last = (-acc * pow(z[-1] % L, -1, L)) % L
        if last:
            break
    e.append(last)
    out = list(sigs)
    for i, ei in zip(P, e):
        sg = bytes(out[i])
        s = (int.from_bytes(sg[32:], "little") + ei) % L
        out[i] = sg[:32] + s.to_bytes(32, "little")
    return out


def shard_seed(seed32, lo):
    """the coefficient seed of the shard that starts at signature lo (nwv_ed25519_verify_batch and
    _keyed in nwv_host.hip): bytes 24..31 XOR the little-endian bytes of lo; the shard's
    coefficient indices are local to its range"""
    s = bytearray(seed32)
    for k, b in enumerate(int(lo).to_bytes(8, "little")):
        s[24 + k] ^= b
    return bytes(s)
