"""The wave interpreter on the device, program by program, at its limb edges.

tools/bls_wave_vectors runs, in one launch with one 64-lane workgroup per case:
  RUN1   every image of tests/bls_wave_vectors.py (all 47 programs; inputs at the edge set, mixed,
         uniform and one-hot at 2p - 1; the repeated programs 1, 2 and 3 times over) through
         wave::Wave::run, the real wave_run: its lane-to-record mapping, its record prefetch and its
         wrap to the first stage when reps > 1;
  RUNK   the images of the programs that stay inside a packed bank, 1 to 4 banks behind one
         shared P << k table as pair_flat lays them out, a different case in every bank, every lane of a
         stage calling lane_value<NWV_BLS_PAIR_TERMS>: the four-reads-then-the-rest grouping, the
         table at its own address and the banks' isolation as the compiler emits them for gfx950.
         This does NOT re-test pair_flat's own lane-to-item loop (lane l: item l / nl of a pass,
         record l % nl), which is inline in the kernel and stays covered end to end by
         tests/test_gpu_bls.py::test_verify_many_packed_waves;
  INV    fp_inv_wave on test_fp_inv_variable_time's values and 0, each also as x + p: all 64
         lanes' results equal, below 2p with normalised limbs, and the inverse's Montgomery form;
  ISONE  Wave::f_is_one and WaveK::f_is_one_mask for 1 to 4 banks on redundant forms of one and of
         values that are not one, in each bank in turn, the other banks holding one.
Every word of every slot after a program is determined by the generator's exact-integer
simulation, so images are compared for equality: no tolerance, no case left out."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import bls_wave_vectors as wv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "bls_wave_vectors")


def _entries():
    """(entries for wv.pack, what each is: (kind, ...))"""
    ints, _ = wv.header()
    nslots, npc, reg_f = ints["NSLOTS"], ints["NSLOTS_PC"], ints["REG_F"]
    g, _ = wv.generator()
    cases = wv.run_cases()
    ent, what = [], []
    for c in cases:
        ns = npc if c.pc else nslots
        ent.append((wv.RUN1, c.off, c.n, c.nl0, c.reps, 1, ns, c.image[:ns], 14 * ns))
        what.append(("run1", c, ns))
    groups = {}
    for c in cases:
        if c.pc:
            groups.setdefault((c.prog, c.reps), []).append(c)
    k = 0
    for grp in groups.values():
        at = 0
        while at < len(grp):
            k = k % 4 + 1
            banks = grp[at:at + k]
            at += len(banks)
            c = banks[0]
            ent.append((wv.RUNK, c.off, c.n, c.nl0, c.reps, len(banks), npc,
                        np.stack([b.image[:npc] for b in banks]), 14 * npc * len(banks)))
            what.append(("runk", banks, npc))
    for x in wv.inv_values():
        ent.append((wv.INV, 0, 0, 0, 0, 0, 0, np.array(wv.limbs(x), dtype=np.uint32), 64 * 14))
        what.append(("inv", x))
    one = [g.mont(1)] + [0] * 11
    for k in range(1, 5):
        for j in range(k):
            for f, is_one in wv.isone_values():
                fs = [f if b == j else one for b in range(k)]
                ent.append((wv.ISONE, 0, 0, 0, 0, k, 0,
                            np.array([[wv.limbs(v) for v in fb] for fb in fs], dtype=np.uint32), 64))
                what.append(("isone", k, j, is_one))
    return ent, what


def _run_tool(tool):
    """the tool's output for every case, from one run"""
    ent, what = _entries()
    data, outs = wv.pack(ent)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(data)
        r = subprocess.run(["timeout", "-k", "10", "120", tool, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = np.fromfile(fout, dtype="<u4")
    assert len(out) == sum(w for _, w in outs)
    return [(w, out[o:o + n]) for w, (o, n) in zip(what, outs)]


@pytest.fixture(scope="module")
def device():
    if not os.path.exists(TOOL):
        subprocess.run(["make", "-C", ROOT, "tools/bls_wave_vectors"], check=True)
    return _run_tool(TOOL)


def _of(device, kind):
    got = [(w, o) for w, o in device if w[0] == kind]
    assert got
    return got


def test_wave_run_images_exact(device):
    bad = []
    progs = set()
    for (_, c, ns), o in _of(device, "run1"):
        progs.add(c.prog)
        bad.append(wv.mismatch(c, o.reshape(ns, 14), c.want[:ns]))
    assert len(progs) == 47
    bad = [m for m in bad if m]
    assert not bad, f"{len(bad)} images differ, first: {bad[:5]}"


def test_packed_bank_images_exact(device):
    bad = []
    sizes = set()
    for (_, banks, npc), o in _of(device, "runk"):
        sizes.add(len(banks))
        o = o.reshape(len(banks), npc, 14)
        for j, c in enumerate(banks):
            m = wv.mismatch(c, o[j], c.want[:npc])
            bad.append(m and f"bank {j} of {len(banks)}: " + m)
    assert sizes == {1, 2, 3, 4}
    bad = [m for m in bad if m]
    assert not bad, f"{len(bad)} banks differ, first: {bad[:5]}"


def test_fp_inv_wave(device):
    g, _ = wv.generator()
    for (_, x), o in _of(device, "inv"):
        o = o.reshape(64, 14)
        assert (o == o[0]).all(), hex(x)
        assert all(int(w) < (1 << 28) for w in o[0]), hex(x)
        v = wv.value(o[0])
        assert v < 2 * g.P and v % g.P == wv.inv_want(x), hex(x)


def test_f_is_one_verdicts(device):
    for (_, k, j, is_one), o in _of(device, "isone"):
        want = ((1 << k) - 1) & ~(0 if is_one else 1 << j)
        assert (o == (want | want << 8)).all(), (k, j, is_one, [hex(int(w)) for w in o[:4]])


def test_tool_refuses_programs_outside_the_tables(tmp_path):
    """a program offset, stage count or lane count that is not a compiled program's, or a program
    that addresses slots the case does not have, ends the tool with status 1 before any launch"""
    if not os.path.exists(TOOL):
        subprocess.run(["make", "-C", ROOT, "tools/bls_wave_vectors"], check=True)
    ints, progs = wv.header()
    nslots, npc = ints["NSLOTS"], ints["NSLOTS_PC"]
    off, n, nl0 = progs["cyc_sqr_f"]
    ioff, in_, inl0 = progs["iso2_add"]
    last = max(progs.values())
    img = np.zeros(nslots * 14, dtype=np.uint32)

    def run1(off, n, nl0, slots=nslots):
        return (wv.RUN1, off, n, nl0, 1, 1, slots, img[:slots * 14], slots * 14)
    bad = {
        "not a record boundary": run1(off + 8, n, nl0),
        "misaligned": run1(off + 1, n, nl0),
        "not the stage's lanes": run1(off, n, nl0 + 1),
        "past the last program": run1(last[0], last[1] + 1, last[2]),
        "far outside": run1(1 << 30, n, nl0),
        "slots beyond the image": run1(ioff, in_, inl0, npc),
        "slots beyond a bank": (wv.RUNK, ioff, in_, inl0, 1, 1, npc, img[:npc * 14], npc * 14),
    }
    fout = tmp_path / "out.bin"
    for name, entry in bad.items():
        # a good case first: the whole file is refused, not only the bad case
        data, _ = wv.pack([run1(off, n, nl0), entry])
        fin = tmp_path / "in.bin"
        fin.write_bytes(data)
        r = subprocess.run(["timeout", "-k", "10", "60", TOOL, str(fin), str(fout)], capture_output=True, text=True)
        assert r.returncode == 1, (name, r.returncode, r.stderr)
        assert not fout.exists(), name
