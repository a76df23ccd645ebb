"""The wave interpreter's lane arithmetic, program by program, at its limb edges -- on the CPU.

tests/hostemu/bls_wave_vectors_hostemu.cpp builds bls_wave.h for the host with BLS_BOUNDS_CHECK:
comb_sums also forms every limb's positive and negative sum on its own in 64 bits (each below 2^32,
the difference non-negative below the top limb: the packed pairs' precondition), carry_par checks
its output limbs (<= 2^28 + 16, top limb non-negative after the fallback), fp_mul / fp_sqr their
column sums in 128 bits, quick_reduce its input's top limb and its result (< 2p).  Every compiled
program runs on the images of tests/bls_wave_vectors.py (inputs from an edge set around 0, p, 2p,
2^380 and a multiple of 2^364, mixed, uniform, and one-hot at 2p - 1), with lane_value<8> (the
one-item kernels' form, the P << k table below slot 0) and, where the program stays inside a
packed bank, with lane_value<4> (the packed kernel's form: four reads in flight then the rest, the
table elsewhere).  Each whole image must equal the one the generator's exact-integer simulation
gives; no bound may fire; and the set must reach carry_par's fallback to the sequential pass and a
negative top limb sum, which random canonical inputs never do (0 of 1,880 runs)."""
import collections
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bls_wave_vectors as wv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(ROOT, "tests", "_build", "libblswvemu.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-C", ROOT, "tests/_build/libblswvemu.so"], check=True)
    L = ctypes.CDLL(path)
    u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
    for fn in (L.bwv_run8, L.bwv_run4):
        fn.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int, u32p]
    L.bwv_stats.argtypes = [np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")]
    L.bwv_first_fired.restype = ctypes.c_char_p
    L.bwv_f_is_one.argtypes = [u32p]
    return L


def _stats(emu):
    s = np.zeros(3, dtype=np.uint64)
    emu.bwv_stats(s)
    return [int(x) for x in s]


def test_layout_matches_header(emu):
    ints, _ = wv.header()
    assert (emu.bwv_nslots(), emu.bwv_nslots_pc(), emu.bwv_reg_f()) == (ints["NSLOTS"], ints["NSLOTS_PC"], ints["REG_F"])


def test_every_program_image_exact_and_in_bounds(emu):
    cases = wv.run_cases()
    ints, _ = wv.header()
    npc = ints["NSLOTS_PC"]
    assert len({c.prog for c in cases}) == 47
    _stats(emu)
    bad, fired = [], []
    fallback, negtop = collections.Counter(), collections.Counter()
    npc_runs = 0
    for c in cases:
        got = c.image.copy()
        assert emu.bwv_run8(c.off, c.n, c.nl0, c.reps, got) == 0, c.prog
        bad.append(wv.mismatch(c, got))
        if c.pc:
            npc_runs += 1
            bank = c.image[:npc].copy()
            assert emu.bwv_run4(c.off, c.n, c.nl0, c.reps, bank) == 0, c.prog
            m = wv.mismatch(c, bank, c.want[:npc])
            bad.append(m and "lane_value<4>: " + m)
        f, pf, nt = _stats(emu)
        if f:
            fired.append(f"{c.prog} case {c.label} reps {c.reps}: {f} bounds")
        fallback[c.prog] += pf
        negtop[c.prog] += nt
    bad = [m for m in bad if m]
    assert not bad, f"{len(bad)} images differ, first: {bad[:5]}"
    assert not fired, f"first bound: {emu.bwv_first_fired().decode()}; {fired[:10]}"
    assert npc_runs > 0
    reach = {p: n for p, n in fallback.items() if n}
    print(f"{len(cases)} runs ({npc_runs} also as a packed bank): carry_par fell back {sum(fallback.values())} times "
          f"in {len(reach)} programs, negative top limb sums {sum(negtop.values())}")
    assert sum(fallback.values()) > 0 and sum(negtop.values()) > 0, \
        f"the vectors no longer reach carry_par's fallback: per program {dict(fallback)}, negative tops {dict(negtop)}"


def test_out_of_table_program_is_refused(emu):
    ints, progs = wv.header()
    img = np.zeros((ints["NSLOTS"], 14), dtype=np.uint32)
    off, n, nl0 = progs["cyc_sqr_f"]
    assert emu.bwv_run8(off, n, nl0, 1, img) == 0
    assert emu.bwv_run8(off + 8, n, nl0, 1, img) == -1      # not a record boundary
    assert emu.bwv_run8(off, n, nl0 + 1, 1, img) == -1      # not the stage's lanes
    assert emu.bwv_run8(1 << 30, n, nl0, 1, img) == -1
    off, n, nl0 = progs["iso2_add"]                          # slots beyond a packed bank
    assert emu.bwv_run4(off, n, nl0, 1, np.zeros((ints["NSLOTS_PC"], 14), dtype=np.uint32)) == -1


def test_f_is_one_on_redundant_values(emu):
    for f, want in wv.isone_values():
        words = np.array([wv.limbs(v) for v in f], dtype=np.uint32)
        assert emu.bwv_f_is_one(words) == int(want), [hex(v) for v in f]


def test_device_tool_refuses_malformed_files_before_any_gpu_call(tmp_path):
    """tools/bls_wave_vectors validates its input's framing (magic, caps on cases, reps, k, slots,
    and the exact file length) before its first HIP call: exit status 1 with or without a GPU (a
    failed HIP call would be 2), and no output file"""
    tool = os.path.join(ROOT, "tools", "bls_wave_vectors")
    if not os.path.exists(tool):
        subprocess.run(["make", "-C", ROOT, "tools/bls_wave_vectors"], check=True)
    ints, progs = wv.header()
    off, n, nl0 = progs["cyc_sqr_f"]
    npc, nslots = ints["NSLOTS_PC"], ints["NSLOTS"]
    z = lambda words: np.zeros(words, dtype=np.uint32)
    good, _ = wv.pack([(wv.ISONE, 0, 0, 0, 0, 1, 0, z(12 * 14), 64)])
    words = np.frombuffer(good, dtype="<u4")

    def patched(i, v):
        w = words.copy()
        w[i] = v
        return w.tobytes()
    bad = {
        "empty": b"",
        "magic": patched(0, 0),
        "no cases": patched(1, 0),
        "too many cases": patched(1, 1 << 20),
        "payload count": patched(2, 12 * 14 + 1),
        "output count": patched(3, 65),
        "mode": patched(4, 4),
        "truncated": good[:-4],
        "trailing bytes": good + b"\0",
        "k = 0": wv.pack([(wv.ISONE, 0, 0, 0, 0, 0, 0, z(1), 64)])[0],
        "k = 5": wv.pack([(wv.ISONE, 0, 0, 0, 0, 5, 0, z(5 * 12 * 14), 64)])[0],
        "RUNK k = 5": wv.pack([(wv.RUNK, off, n, nl0, 1, 5, npc, z(5 * npc * 14), 5 * npc * 14)])[0],
        "RUNK slots": wv.pack([(wv.RUNK, off, n, nl0, 1, 1, nslots, z(nslots * 14), nslots * 14)])[0],
        "RUN1 slots": wv.pack([(wv.RUN1, off, n, nl0, 1, 1, nslots + 1, z((nslots + 1) * 14), (nslots + 1) * 14)])[0],
        "reps = 0": wv.pack([(wv.RUN1, off, n, nl0, 0, 1, nslots, z(nslots * 14), nslots * 14)])[0],
        "reps = 9": wv.pack([(wv.RUN1, off, n, nl0, 9, 1, nslots, z(nslots * 14), nslots * 14)])[0],
        "65 lanes": wv.pack([(wv.RUN1, off, n, 65, 1, 1, nslots, z(nslots * 14), nslots * 14)])[0],
        "65 stages": wv.pack([(wv.RUN1, off, 65, nl0, 1, 1, nslots, z(nslots * 14), nslots * 14)])[0],
    }
    fout = tmp_path / "out.bin"
    for name, data in bad.items():
        fin = tmp_path / "in.bin"
        fin.write_bytes(data)
        r = subprocess.run(["timeout", "-k", "10", "60", tool, str(fin), str(fout)], capture_output=True, text=True)
        assert r.returncode == 1, (name, r.returncode, r.stderr)
        assert not fout.exists(), name
