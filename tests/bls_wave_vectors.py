"""Slot images for the wave interpreter's tests (tests/test_bls_wave_vectors_hostemu.py,
tests/test_gpu_bls_wave_vectors.py): every compiled program of tools/gen_bls_wave.py on inputs at
the limb arithmetic's edges, and the image the generator's exact-integer `simulate` says must
come out.

A stage's result is an exact integer (a product is (a b + m p) / R with m chosen limb by limb from
the integer a b, whatever the operands' limbs were) and every slot is written normalised, so after
a program every word of every slot is determined: the tests compare whole images for equality,
temporaries included, and the slots a program never writes must still hold what was put there
(here: seeded junk below 2p, so a read of a slot the program should not read shows too)."""
import functools
import importlib.util
import os
import random
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 381
# the programs the engine runs several times in one interpreter call (exp_chain's squarings and
# doublings: cyc_sqr_F, g1_dbl_U) and the two other repeated steps; they also run 2 and 3 times over
REPEATED = ("cyc_sqr_F", "sqr_F", "g1_dbl_U", "mlp_dbl_fixed")


@functools.lru_cache(maxsize=None)
def generator():
    """(module, compiled programs): tools/gen_bls_wave.py as its __main__ block builds them"""
    spec = importlib.util.spec_from_file_location("gen_bls_wave", os.path.join(ROOT, "tools", "gen_bls_wave.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    state = random.getstate()
    random.seed(1)
    compiled = g.build_all()
    random.setstate(state)
    return g, compiled


@functools.lru_cache(maxsize=None)
def header():
    """the constants and the program table of the committed bls_wave_prog.h"""
    src = open(os.path.join(ROOT, "narwhal_amd", "csrc", "bls_wave_prog.h")).read()
    ints = {k: int(v) for k, v in re.findall(r"constexpr int (\w+) = (\d+);", src)}
    progs = {name.lower(): (int(off), int(n), int(nl0))
             for name, off, n, nl0 in re.findall(r"constexpr Prog P_(\w+) = \{(\d+)u, (\d+), (\d+)\};", src)}
    return ints, progs


def limbs(v):
    g, _ = generator()
    assert 0 <= v < (1 << 392)
    return g._limbs(v)


def value(words):
    return sum(int(w) << (28 * j) for j, w in enumerate(words))


def edge_set():
    g, _ = generator()
    p, T = g.P, 1 << 364
    top = (2 * p - 1) // T * T
    return [0, 1, p - 1, p, p + 1, 2 * p - 2, 2 * p - 1, 1 << 380, (1 << 381) - 1, top, top - 1]


def input_sets(nin, rnd):
    """(class, values) per case for a program of nin inputs"""
    g, _ = generator()
    p2 = 2 * g.P
    edges = edge_set()
    assert all(0 <= e < p2 for e in edges)
    out = [(f"a{i}", [e] * nin) for i, e in enumerate(edges)]
    out += [(f"b{i}", [rnd.choice(edges) for _ in range(nin)]) for i in range(8)]
    out += [(f"c{i}", [rnd.randrange(p2) for _ in range(nin)]) for i in range(4)]
    if nin <= 12:
        for i in range(nin):
            out.append((f"d{i}", [p2 - 1 if j == i else 0 for j in range(nin)]))
            out.append((f"d{i}r", [0 if j == i else p2 - 1 for j in range(nin)]))
    return out


class Case:
    __slots__ = ("prog", "label", "reps", "off", "n", "nl0", "pc", "image", "want")


@functools.lru_cache(maxsize=None)
def run_cases():
    """every program x every input class (x reps for REPEATED): Case.image is the whole NSLOTS
    image put in, Case.want the one simulate gives; Case.pc tells whether the program stays inside a
    packed bank (slots below NSLOTS_PC), where image[:NSLOTS_PC] is the bank's image"""
    g, compiled = generator()
    ints, progs = header()
    assert sorted(progs) == sorted(n.lower() for n in compiled), "bls_wave_prog.h and the generator disagree"
    assert len(compiled) == 47
    nslots, nslots_pc = ints["NSLOTS"], ints["NSLOTS_PC"]
    assert nslots == max(cp.max_slot for cp in compiled.values()) and nslots_pc == g.LAYOUT["nslots_pc"]
    rnd = random.Random(SEED)
    p2 = 2 * g.P
    junk = [rnd.randrange(p2) for _ in range(nslots)]
    junk_limbs = np.array([limbs(v) for v in junk], dtype=np.uint32)
    consts = {a.slot: m for m, a in g.CTX.consts.items()}
    cases = []
    for name, cp in compiled.items():
        ins = sorted(cp.prog.inputs.values(), key=lambda a: a.slot)
        in_slots = [a.slot for a in ins]
        assert len(set(in_slots)) == len(in_slots) and not set(in_slots) & (set(consts) | {0})
        assert all(g.REGS.bound(reg) == p2 for reg, _ in cp.prog.inputs)
        touched = {r["dst"] for st in cp.stages for r in st} | \
            {sl for st in cp.stages for r in st for part in (r["a"], r["b"]) if part for side in part for sl, _ in side}
        pc = max(touched) < nslots_pc
        assert pc == (g._prog_regs(cp.prog) <= set(g.PC_REGS)), name
        base = junk_limbs.copy()
        base[0] = 0
        for s, m in consts.items():
            base[s] = limbs(m)
        for label, vals in input_sets(len(ins), rnd):
            for reps in ((1, 2, 3) if name in REPEATED else (1,)):
                # simulate sees only what a program may read: slot 0, the constants, its inputs
                # (a read of anything else is a KeyError here)
                wm = {0: 0, **consts, **dict(zip(in_slots, vals))}
                for _ in range(reps):
                    g.simulate(cp, wm)
                c = Case()
                c.prog, c.label, c.reps, c.pc = name, label, reps, pc
                c.off, c.n, c.nl0 = progs[name.lower()]
                c.image = base.copy()
                for s, v in zip(in_slots, vals):
                    c.image[s] = limbs(v)
                c.want = c.image.copy()
                for s, v in wm.items():
                    if s not in consts and s != 0:
                        c.want[s] = limbs(v)
                cases.append(c)
    return cases


def mismatch(case, got, want=None):
    """'' when got equals the case's expected image, else program, case, slot and limb of the first
    difference"""
    want = case.want if want is None else want
    if np.array_equal(got, want):
        return ""
    s, j = np.argwhere(got != want)[0]
    return (f"{case.prog} case {case.label} reps {case.reps}: slot {s} limb {j}: "
            f"got {int(got[s, j]):#x} want {int(want[s, j]):#x}")


# ---- fp_inv_wave and the F == 1 verdicts ---------------------------------------------------------
def inv_values():
    """test_fp_inv_variable_time's values and 0, each also as x + p (slot integers below 2p)"""
    g, _ = generator()
    p = g.P
    rnd = random.Random(56)
    vals = [1, 2, 3, p - 1, p - 2, (p + 1) // 2, 1 << 62, (1 << 62) - 1, 1 << 380, (1 << 381) % p, 0]
    vals += [rnd.randrange(1, p) for _ in range(300)] + [rnd.randrange(1, 1 << rnd.randrange(1, 380)) for _ in range(100)]
    return vals + [v + p for v in vals]


def inv_want(x):
    """the Montgomery form of the inverse of the field element whose Montgomery form is x"""
    g, _ = generator()
    return g.mont(pow(g.unmont(x % g.P), g.P - 2, g.P))


def isone_values():
    """(F as 12 slot integers, is the Fp12 one) for the verdict's cases"""
    g, _ = generator()
    p, one = g.P, g.mont(1)
    z = [0] * 11
    out = [([one] + z, True)]
    f = [one + p] + z
    f[5] = p
    out.append((f, True))        # non-canonical one and zero
    f = [one] + z
    f[11] = 1
    out.append((f, False))
    out.append(([0] + z, False))  # coefficient 0 = 0 is all zero ...
    f = [0] + z
    f[3] = p
    out.append((f, False))       # ... also with a non-canonical zero elsewhere
    for c in (0, 7):
        f = [one] + z
        f[c] = 2 * p - 1
        out.append((f, False))
    return out


# ---- the device tool's file (tools/bls_wave_vectors.hip) -----------------------------------------
MAGIC = 0x31565742
RUN1, RUNK, INV, ISONE = 0, 1, 2, 3


def pack(entries):
    """entries: (mode, off, n, nl0, reps, k, slots, payload words, words out) per case -> the input
    file's bytes and every case's (offset, words) in the output file"""
    tab, parts, outs = [], [], []
    nout = 0
    for mode, off, n, nl0, reps, k, slots, payload, wout in entries:
        tab.append([mode, off, n, nl0, reps, k, slots, 0])
        parts.append(np.ascontiguousarray(payload, dtype="<u4").reshape(-1))
        outs.append((nout, wout))
        nout += wout
    payload = np.concatenate(parts)
    hdr = np.array([MAGIC, len(entries), len(payload), nout], dtype="<u4")
    return hdr.tobytes() + np.array(tab, dtype="<u4").tobytes() + payload.tobytes(), outs
