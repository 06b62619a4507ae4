"""The compiled chain kernels with more than one float4 per lane (csrc/chain_codegen.cpp, chain_quads_for / emit_quads) on the
device: bit for bit against the CPU oracle and against the same evaluation with chain_quads = 1 (one float4 per lane, the
form every other launch keeps), NaN == NaN.

The warm cache-policy mask is forced at these small sizes with the option nt_force (0x101: input 0 and the result
nontemporal, the other inputs plain; 0x102 the same with input 1).  The unit counts (float4 per plane) straddle every guard
of two and of four quads per lane with 256-lane workgroups: 1, 255 / 256 / 257, 511 / 512 / 513, 1023 / 1025, a flat launch
of many rows (64 x 33: dense rows, 528 units) and a pitched one (1028 x 7: rows padded to the pool's pitch), which keeps one
float4 per lane.  The form each launch took is read back from kc_stats_counter ("specialized_nt_<mask>[_q<quads>]")."""
import numpy as np
import pytest

from util import SEED_A, assert_planes, splitmix_plane, with_edge_cases

pytestmark = pytest.mark.gpu

QUADS = 2  # kQuadsWarm (csrc/chain_codegen.cpp): what the rule picks
SHAPES = [(4, 1), (1020, 1), (1024, 1), (1028, 1), (2044, 1), (2048, 1), (2052, 1), (4092, 1), (4100, 1), (64, 33), (1028, 7)]
TAIL = [np.nan, np.inf, -np.inf, -0.0, 1e-40, 3e38, 1.25]  # written from the last sample backwards: the guarded end
CONSTS = [0.375, -1.25, 2.0, 1.5, -0.0, 0.75, -3.0, 0.5, 0.625, 1.75, -0.875, 0.25, 1.0, -2.0, 0.1, 1.1]


def inv(op, k, c):
    """One record "c - (acc op input k)" as two Mix nodes."""
    return [(op, False, ("p", k)), ("Subtract", True, ("c", c))]


# name: (input planes, start, steps or "join", nt_force, more than one quad per lane where the launch is flat); a program of
# more than 16 records and one with a divide keep one float4 per lane
PROGRAMS = {
    "headline": (2, ("p", 0), sum((inv("Add" if i % 2 == 0 else "Multiply", 1, CONSTS[i]) for i in range(16)), []), 0x101, True),
    "one_record": (2, ("p", 0), inv("Multiply", 1, 0.625), 0x101, True),
    "start_constant": (2, ("c", 1.5), inv("Add", 0, 0.375) + [("Subtract", True, ("p", 1)), ("Multiply", False, ("p", 0))], 0x102, True),
    "three_inputs": (3, ("p", 0), inv("Add", 1, 2.0) + inv("Multiply", 2, -1.25) + [("Subtract", False, ("p", 1))], 0x101, True),
    "joined": (3, ("p", 0), "join", 0x101, True),
    "seventeen_records": (2, ("p", 0), sum((inv("Add" if i % 2 == 0 else "Multiply", 1, CONSTS[i % 16]) for i in range(17)), []), 0x101, False),
    "divide": (2, ("p", 0), inv("Add", 1, 0.75) + [("Divide", False, ("p", 1))] + inv("Multiply", 1, 0.5), 0x101, False),
}


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    saved = {n: kc.get_option(n) for n in ("nt_force", "chain1")}
    spec = kc.get_specialize()
    kc.set_option("chain1", 0)  # a one-record program goes to its compiled kernel, not to chain1.hip
    kc.set_specialize(2)        # compile at first sight and wait
    yield kc
    kc.set_chain_quads(0)
    for n, v in saved.items():
        kc.set_option(n, v)
    kc.set_specialize(spec)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


_planes = {}


def planes_of(w, h):
    """Three planes of values in [-1, 3) with the IEEE edge cases at the head and at the very end; made once per shape."""
    if (w, h) not in _planes:
        out = []
        for k in range(3):
            p = with_edge_cases(splitmix_plane(SEED_A + 17 * k, 0, h, w) * np.float32(4.0) - np.float32(1.0), shift=k + 1).reshape(-1)
            n = min(len(TAIL), len(p) // 2)
            p[len(p) - n:] = np.roll(np.array(TAIL, np.float32), k)[:n][::-1]
            out.append(p.reshape(h, w))
        _planes[(w, h)] = out
    return _planes[(w, h)]


_expected = {}


def expected(orc, name, w, h):
    """The oracle's result of a program on a shape; computed once, never written to."""
    if (name, w, h) not in _expected:
        n_in, start, steps, _, _ = PROGRAMS[name]
        p = planes_of(w, h)
        full = lambda v: np.full((h, w), v, np.float32)
        want = p[start[1]] if start[0] == "p" else full(start[1])
        if steps == "join":
            second = orc.mix_plane("Subtract", full(0.75), orc.mix_plane("Multiply", p[2], p[1]))
            want = orc.mix_plane("Subtract", full(2.0), orc.mix_plane("Add", want, p[1]))
            want = orc.mix_plane("Multiply", want, second)
            want = orc.mix_plane("Subtract", full(-1.25), orc.mix_plane("Add", want, p[2]))
        else:
            for op, right, (kind, v) in steps:
                x = p[v] if kind == "p" else full(v)
                want = orc.mix_plane(op, x, want) if right else orc.mix_plane(op, want, x)
        want.setflags(write=False)
        _expected[(name, w, h)] = want
    return _expected[(name, w, h)]


def evaluate(kc, name, w, h):
    n_in, start, steps, _, _ = PROGRAMS[name]
    mix, mt = kc.mix_process, kc.MixType.parse
    imgs = [kc.SlotImage.from_planes([p]) for p in planes_of(w, h)[:n_in]]
    const = lambda v: kc.SlotImage.from_value((w, h), v, False)
    acc = imgs[start[1]] if start[0] == "p" else const(start[1])
    if steps == "join":
        # a second chain that has not run joins the first: its value is put aside and read back (CH_SAVE_LOAD)
        second = mix(const(0.75), mix(imgs[2], imgs[1], mt("Multiply")), mt("Subtract"))
        acc = mix(const(2.0), mix(acc, imgs[1], mt("Add")), mt("Subtract"))
        acc = mix(acc, second, mt("Multiply"))
        acc = mix(const(-1.25), mix(acc, imgs[2], mt("Add")), mt("Subtract"))
    else:
        for op, right, (kind, v) in steps:
            x = imgs[v] if kind == "p" else const(v)
            acc = mix(x, acc, mt(op)) if right else mix(acc, x, mt(op))
    return acc.planes()[0]


def launched_forms(kc, mask, run):
    """(result of run(), {counter suffix: launches}) over the three forms a compiled kernel of this mask can have."""
    names = {s: "specialized_nt_%03x%s" % (mask, s) for s in ("", "_q2", "_q4")}
    before = {s: kc.stats_counter(n) for s, n in names.items()}
    got = run()
    return got, {s: kc.stats_counter(n) - before[s] for s, n in names.items() if kc.stats_counter(n) != before[s]}


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_program_on_shape(kc, orc, name, shape):
    w, h = shape
    n_in, _, _, force, eligible = PROGRAMS[name]
    mask = force & (((1 << n_in) - 1) | 0x100)
    flat = h == 1 or (w * 4) % 256 == 0  # one row, or dense rows at the pool's pitch
    kc.set_option("nt_force", force)
    settings = [(0, QUADS), (1, 1), (2, 2), (4, 4)]  # (four is not the rule's choice, but the setting exists)
    results = {}
    for setting, per_lane in settings:
        kc.set_chain_quads(setting)
        got, forms = launched_forms(kc, mask, lambda: evaluate(kc, name, w, h))
        suffix = "_q%d" % per_lane if eligible and flat and per_lane > 1 else ""
        assert forms == {suffix: 1}, "%s %dx%d chain_quads=%d: launched %s" % (name, w, h, setting, forms)
        results[setting] = got
    want = expected(orc, name, w, h)
    for setting, got in results.items():
        assert_planes([got], [want], what="%s %dx%d chain_quads=%d vs oracle" % (name, w, h, setting))
        assert_planes([got], [results[1]], what="%s %dx%d chain_quads=%d vs one quad per lane" % (name, w, h, setting))
