"""The packed-f32 form of the chain kernels compiled at run time (csrc/chain_codegen.cpp: every {+, -, *} step is
v_pk_add_f32 / v_pk_mul_f32, a subtraction a packed add with the negate modifier, and "c - (acc op x)" reads c for both
halves from one scalar register) against the step interpreter and the CPU oracle, bit for bit with NaN == NaN.

Every step code {ADD, SUB_L, SUB_R, MUL, ADD_INV, SUBL_INV, SUBR_INV, MUL_INV} meets every operand kind a graph can give it:
an input plane, a constant, and the value of a second chain joined into the program (the "saved" value).  EVERY record has a
constant of its own (and in RGBA every channel its own: blockIdx.y selects the record table), so a constant read from the
wrong dword, the wrong half or the wrong record changes the result; -0.0 and a subnormal are among them, and +-inf and NaN
take each record's constant in turn in programs of their own (they would hide every later step of a long one).  The planes
carry util.EDGE_VALUES at their head and util.SALT_VALUES on their edge rows and columns.  Flat (dense rows: one row of
float4 units) and pitched launches, Gray and RGBA.

A "c - (acc op x)" record exists for a plane or saved operand; with a constant operand the host keeps the two steps two
records (a record holds one constant), which is what the constant cases of the *_INV codes run.

The up-sampling chain form (kc_upchain_*) is unchanged and keeps its own tests (test_gpu_upsample.py)."""
import numpy as np
import pytest

from test_gpu_chain_variants import Inputs
from util import assert_planes

pytestmark = pytest.mark.gpu

CODES = {  # code -> (Mix type, running value on the right, "c - ..." after it)
    "ADD": ("Add", False, False), "SUB_L": ("Subtract", False, False), "SUB_R": ("Subtract", True, False),
    "MUL": ("Multiply", False, False), "ADD_INV": ("Add", False, True), "SUBL_INV": ("Subtract", False, True),
    "SUBR_INV": ("Subtract", True, True), "MUL_INV": ("Multiply", False, True),
}
KINDS = ["plane", "constant", "saved"]
LAYOUTS = {  # (rgba, (w, h)): 512 columns are dense rows (a flat launch), 130 are pitched
    "gray_flat": (False, (512, 24)), "gray_pitched": (False, (130, 37)), "rgba_flat": (True, (512, 16)), "rgba_pitched": (True, (130, 21)),
}
SUBNORMAL = float(np.float32(1e-40))
# one triple (R, G, B) per record, all different; moderate sizes, so that the running value of a long program stays finite
# wherever the planes are
FINITE = [(0.375, -1.25, 2.0), (1.5, -0.0, 0.75), (-3.0, SUBNORMAL, 0.5), (2.0, -0.5, 1.0), (0.625, 1.75, -0.0), (-0.875, 0.25, 3.0),
          (1.0, -2.0, SUBNORMAL), (0.1, 1.1, -1.1), (2.5, 0.3, -0.7), (-1.5, 0.9, 1.3), (0.2, -0.4, 0.6), (1.25, 2.25, -2.75),
          (0.05, 0.95, 1.05), (-0.35, 0.45, -0.55), (3.5, -3.25, 0.15), (0.85, -0.65, 1.45)]
SPECIAL = {"neg_zero": -0.0, "subnormal": SUBNORMAL, "inf": float("inf"), "neg_inf": float("-inf"), "nan": float("nan")}


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    spec, chain1 = kc.get_specialize(), kc.get_option("chain1")
    yield kc
    kc.set_specialize(spec)
    kc.set_option("chain1", chain1)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


def build(kc, orc, inp, records):
    """records: (code, kind, constant triple).  Returns (lazy image, expected planes).  Plane operands alternate between
    inputs 1 and 2; a saved operand is a second chain (input 2 * the record's constant, rotated) that has not run."""
    nch = 3 if inp.rgba else 1
    mix, mt = kc.mix_process, kc.MixType.parse
    acc, want = inp.imgs[0], [inp.planes[0][c] for c in range(nch)]
    for i, (code, kind, cs) in enumerate(records):
        op, right, inv = CODES[code]
        if kind == "plane":
            k = 1 + i % 2
            x, xw = inp.imgs[k], [inp.planes[k][c] for c in range(nch)]
        elif kind == "constant":
            x, xw = inp.const(cs), [inp.value(("c", cs), c) for c in range(nch)]
        else:
            rot = cs[1:] + cs[:1]
            x = mix(inp.imgs[2], inp.const(rot), mt("Multiply"))
            xw = [orc.mix_plane("Multiply", inp.planes[2][c], inp.value(("c", rot), c)) for c in range(nch)]
        acc = mix(x, acc, mt(op)) if right else mix(acc, x, mt(op))
        want = [orc.mix_plane(op, xw[c], want[c]) if right else orc.mix_plane(op, want[c], xw[c]) for c in range(nch)]
        if inv:
            ic = cs[2:] + cs[:2] if kind == "constant" else cs  # a constant operand has taken cs itself
            acc = mix(inp.const(ic), acc, mt("Subtract"))
            want = [orc.mix_plane("Subtract", inp.value(("c", ic), c), want[c]) for c in range(nch)]
    return acc, want


def three_ways(kc, orc, inp, records, what):
    """interpreter == compiled kernel == oracle; the compiled run must have launched a compiled kernel."""
    kc.set_option("chain1", 0)  # a one-record program goes to its compiled kernel, not to chain1.hip
    kc.set_specialize(0)
    img, want = build(kc, orc, inp, records)
    interp = img.planes()
    kc.set_specialize(2)
    s0 = kc.specialize_stats()
    img, _ = build(kc, orc, inp, records)
    spec = img.planes()
    s1 = kc.specialize_stats()
    assert s1["compiles_failed"] == s0["compiles_failed"], what
    assert s1["specialized_launches"] > s0["specialized_launches"], what
    nch = 3 if inp.rgba else 1
    assert_planes(spec[:nch], interp[:nch], what=what + ": compiled kernel vs interpreter")
    assert_planes(spec[:nch], want, what=what + ": compiled kernel vs oracle")
    assert_planes(interp[:nch], want, what=what + ": interpreter vs oracle")


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("kind", KINDS)
def test_every_code_in_one_program(kc, orc, kind, layout):
    rgba, (w, h) = LAYOUTS[layout]
    inp = Inputs(kc, 3, h, w, rgba, "pool")
    records = [(code, kind, FINITE[i]) for i, code in enumerate(CODES)] + [(code, kind, FINITE[8 + i]) for i, code in enumerate(reversed(CODES))]
    three_ways(kc, orc, inp, records, "%s %s" % (kind, layout))


@pytest.mark.parametrize("layout", ["gray_flat", "rgba_pitched"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("code", sorted(CODES))
def test_each_code_alone_and_in_either_slot(kc, orc, code, kind, layout):
    """One record of the code alone, then as the second of a pair and the first of the next pair (records travel two to a
    16-byte pair: .a and .b), the neighbours with constants of their own."""
    rgba, (w, h) = LAYOUTS[layout]
    inp = Inputs(kc, 3, h, w, rgba, "pool")
    three_ways(kc, orc, inp, [(code, kind, FINITE[3])], "%s %s %s alone" % (code, kind, layout))
    records = [("ADD_INV", "plane", FINITE[0]), (code, kind, FINITE[5]), (code, kind, FINITE[9]), ("MUL_INV", "plane", FINITE[12])]
    three_ways(kc, orc, inp, records, "%s %s %s between neighbours" % (code, kind, layout))


@pytest.mark.parametrize("special", sorted(SPECIAL))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("code", sorted(CODES))
def test_special_constants(kc, orc, code, kind, special):
    """-0.0, a subnormal, +-inf and NaN as the constant of each record in turn (R, G and B take it in different records in
    RGBA), the other records keeping finite constants of their own."""
    v = SPECIAL[special]
    for layout, slots in (("gray_flat", [(v, v, v)]), ("rgba_pitched", [(v, 0.5, -1.5), (0.75, v, 2.0)])):
        rgba, (w, h) = LAYOUTS[layout]
        inp = Inputs(kc, 3, h, w, rgba, "pool")
        for where in (0, 1):
            for cs in slots:
                records = [(code, kind, FINITE[2]), (code, kind, FINITE[6])]
                records[where] = (code, kind, cs)
                three_ways(kc, orc, inp, records, "%s %s constant %s in record %d, %s" % (code, kind, special, where, layout))
