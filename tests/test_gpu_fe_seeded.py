"""The device path of fe25519.h's column sums is inline assembly (carry-seeded v_mad_u64_u32
chains) that the host emulation cannot run.  tools/fe_vectors runs fe_mul, fe_sq and
fe_sqn(., 250) on the GPU, one element per lane, on the edge set of tests/fe_vectors.py plus 4,096
random elements; the results must equal Python integers mod 2^255 - 19 and be carried.

End to end, batches of 65 and 1,025 signatures under NWV_FLAG_NO_ROW_PREP (lane-local
decompression), with and without the key cache, hold every golden and ZIP-215 small-order vector
and one forged signature in first, middle and last position: verdict and exact bad set equal the
oracle's."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import fe_vectors as fv
import oracle_ffi as of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "fe_vectors")


def test_device_mul_sq_sqn_match_integers():
    if not os.path.exists(TOOL):
        subprocess.run(["make", "-C", ROOT, "tools/fe_vectors"], check=True)
    a, b = fv.operand_pairs(4096, seed=950)
    n = len(a)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([n, fv.NSQ], dtype="<u4").tobytes())
            f.write(a.astype("<u4").tobytes())
            f.write(b.astype("<u4").tobytes())
        r = subprocess.run(["timeout", "-k", "10", "60", TOOL, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = np.fromfile(fout, dtype="<u4").reshape(n, 3, 10)
    fv.check(a, b, out[:, 0], out[:, 1], out[:, 2])


def _v(v):
    return bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"])


@pytest.fixture(scope="module", params=["keycache", "nokeycache"])
def eng(request):
    import narwhal_amd
    from narwhal_amd import _lib
    flags = _lib.NWV_FLAG_MSM_ALWAYS | _lib.NWV_FLAG_NO_ROW_PREP
    if request.param == "nokeycache":
        flags |= _lib.NWV_FLAG_NO_KEYCACHE
    e = narwhal_amd.Engine(device=0, flags=flags)
    yield e
    e.close()


@pytest.fixture(scope="module")
def vectors():
    vecs = [_v(v) for name in ("ed25519_vectors.json", "zip215_small_order.json")
            for v in of.load_golden(name)["vectors"]]
    return vecs, [of.verify(*v) for v in vecs]


def _keyed(items):
    keys, idx, pos = [], [], {}
    for pk, _, _ in items:
        if pk not in pos:
            pos[pk] = len(keys)
            keys.append(pk)
        idx.append(pos[pk])
    return keys, idx


@pytest.mark.parametrize("n", [65, 1025])
def test_lane_local_batches_match_oracle(eng, vectors, n):
    vecs, vwant = vectors
    rnd = np.random.default_rng(n)
    seeds = [rnd.bytes(32) for _ in range(n)]
    msgs = [rnd.bytes(32) for _ in range(n)]
    pk, sg = eng.sign_many(seeds, msgs)
    honest = [(pk[32 * i:32 * i + 32].tobytes(), sg[64 * i:64 * i + 64].tobytes(), msgs[i]) for i in range(n)]
    ok, bits = eng.verify_batch(honest, seed=bytes([n % 251]) * 32)
    assert ok and all(bits)
    # first, middle and last stay honest signatures (the forged ones); the vectors fill the other
    # places, in as many batches as it takes to hold them all
    forge_at = (0, n // 2, n - 1)
    places = [i for i in range(n) if i not in forge_at]
    for lo in range(0, len(vecs), len(places)):
        base, want_base = list(honest), [True] * n
        for p, k in zip(places, range(lo, min(lo + len(places), len(vecs)))):
            base[p], want_base[p] = vecs[k], vwant[k]
        for bad in (None,) + forge_at:
            items, want = list(base), list(want_base)
            if bad is not None:
                p, s, m = items[bad]
                items[bad] = (p, s[:7] + bytes([s[7] ^ 0x20]) + s[8:], m)
                want[bad] = of.verify(*items[bad])
                assert not want[bad]
            ok, bits = eng.verify_batch(items, seed=bytes([lo % 256]) * 32)
            assert ok == all(want)
            assert bits == want
            keys, kidx = _keyed(items)
            ok, bits = eng.verify_batch_keyed(keys, kidx, [s for _, s, _ in items], [m for _, _, m in items])
            assert ok == all(want)
            assert bits == want
