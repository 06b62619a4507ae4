"""GPU parity of every form the Mix chain family launches: the one-step kernels (chain1_kernel<CODE, NTA, NTB, NTS>), the
step interpreter (chain_kernel<K, U, MODE, NT>, chain_kernel_k0<MODE>) and kernels compiled for a program at run time with
their cache-policy bits.  Every case is ONE launch, exactly one counter of the family (kc_stats_counter) rises, by one, and
the result equals the CPU oracle evaluated node by node: bit for bit, and under the Pow contract (util.pow_mismatch) where the
program ends in Pow.

The inputs carry IEEE edge cases (util.with_edge_cases at the head, util.salt on the first, middle and last rows and columns):
NaN, +-inf, +-0, subnormals and values whose products overflow meet every op.  Programs are deterministic: a Pow step only
ever comes last (a one-ulp Pow difference would otherwise be amplified by the steps after it; Pow inside longer programs is
held by test_gpu_pow.py, interpreter against compiled kernel, bit for bit).

The nontemporal forms are reached through the real cache policy (runtime.cpp chain_cache_policy), never forced: 1 MiB planes
(512 x 512 f32, one channel), cache_budget_mb 0, 1 or 2, and the inputs the test still holds.  The policy keeps the inputs
with at least two references cacheable while they fit, most referenced first, and streams the result unless it fits beside
them.  An input of a chain built from Mix nodes has at least two references at launch whether or not the caller still holds
it: the link of the Mix that took it and the flattened chain each hold one (runtime.cpp plane_mix, chain_flatten); a held
one has three.  So holding an input decides which input is kept at a budget for one, never whether an input is streamed
while the result is not.  With a start plane S and an operand plane X (chain1's nontemporal bits: 1 S, 2 X, 4 the result):
  budget >= 3: 0;  budget 2: 4;  budget 1: hold X 5, hold S (or neither: the first input wins the tie) 6;  budget 0: 7.
Forms no graph reaches:
  chain1_nt1, chain1_nt2, chain1_nt3 (and the compiled kernels' masks 0x001 - 0x003 of a two-input program): streamed inputs
  with a cacheable result need an input with a single reference (above).
  chain_k0_m0 / chain_k0_m1: the host folds a Mix of two constants except Pow (runtime.cpp plane_mix), so a program without
  an input plane always starts with Pow: MODE 2.
  the nontemporal interpreter at a tuning unroll (U != 4 in MODE 0) does not exist (chain.hip launch_chain_k), nor a
  nontemporal chain_kernel_k0.
A one-record program with a step code that puts the running value on the right (x - acc, x / acc, x ^ acc, c - (x - acc))
comes from a Mix whose right input is a chain that has not run, and that chain then running on its own first: the case
materialises it before the launch that is measured."""
import ctypes as C

import numpy as np
import pytest

from util import SEED_A, assert_planes, pow_mismatch, salt, splitmix_plane, with_edge_cases

pytestmark = pytest.mark.gpu

UNROLLS = (1, 2, 4, 6, 8)
INTERP = ["chain_interp_k%d_u%d_m0" % (k, u) for k in range(1, 5) for u in UNROLLS]
INTERP += ["chain_interp_k%d_u4_m0_nt" % k for k in range(1, 5)]
INTERP += ["chain_interp_k%d_u4_m1%s" % (k, nt) for k in range(1, 5) for nt in ("", "_nt")]
INTERP += ["chain_interp_k%d_u1_m2%s" % (k, nt) for k in range(1, 5) for nt in ("", "_nt")]
CHAIN1 = ["chain1_nt%d" % b for b in range(8)]
SPEC = ["specialized_nt_%03x" % (m | r) for m in range(16) for r in (0, 0x100)]
# the instantiations a graph can reach (see the module docstring for the others)
INSTANTIATIONS = ["chain1_nt%d" % b for b in (0, 4, 5, 6, 7)] + INTERP + ["chain_k0_m2"]
UNREACHABLE = ["chain1_nt1", "chain1_nt2", "chain1_nt3", "chain_k0_m0", "chain_k0_m1"] + ["chain_interp_k%d_u%d_m0_nt" % (k, u) for k in range(1, 5) for u in (1, 2, 6, 8)]
# every counter of the family: a case asserts the delta of each (0 unless the case names it)
COUNTERS = INSTANTIATIONS + UNREACHABLE + SPEC + ["chain1_launches"]

CODE_OF = {  # chain1 step code -> (Mix type, running value on the right, "c - ..." after it)
    "ADD": ("Add", False, False), "SUB_L": ("Subtract", False, False), "SUB_R": ("Subtract", True, False),
    "MUL": ("Multiply", False, False), "DIV_L": ("Divide", False, False), "DIV_R": ("Divide", True, False),
    "POW_L": ("Pow", False, False), "POW_R": ("Pow", True, False), "ADD_INV": ("Add", False, True),
    "SUBL_INV": ("Subtract", False, True), "SUBR_INV": ("Subtract", True, True), "MUL_INV": ("Multiply", False, True),
}
CONSTS = [(0.375, -1.25, 2.0), (1.5, 0.0, -0.0), (-3.0, 1e-20, 0.5), (2.0, -0.5, 1e30)]  # per channel R, G, B


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    saved = {n: kc.get_option(n) for n in ("cache_budget_mb", "chain1", "chain_unroll", "max_blocks")}
    spec = kc.get_specialize()
    yield kc
    for n, v in saved.items():
        kc.set_option(n, v)
    kc.set_specialize(spec)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


@pytest.fixture
def options(kc):
    saved = {n: kc.get_option(n) for n in ("cache_budget_mb", "chain1", "chain_unroll", "max_blocks")}
    spec = kc.get_specialize()
    yield
    for n, v in saved.items():
        kc.set_option(n, v)
    kc.set_specialize(spec)


def edge_plane(seed, k, h, w):
    """Values in [-1, 3) with the IEEE edge cases at the head (with_edge_cases) and on the edge rows and columns (salt)."""
    p = splitmix_plane(seed, k, h, w) * np.float32(4.0) - np.float32(1.0)
    p = with_edge_cases(p, shift=k + 1)
    return salt(p, [0, 1, h // 2, h - 2, h - 1], [0, 1, 2, w // 2, w - 2, w - 1], shift=3 * k)


class Inputs:
    """K input planes per channel as images of one layout: "pool" (kc_image_from_f32: planes of the pool, 256-byte pitch)
    or "wrapped" (caller-owned torch memory, kc_plane_wrap, rows padded by 48 bytes: input pitches differ from the output's)."""

    def __init__(self, kc, k, h, w, rgba, storage, seed=SEED_A):
        self.kc, self.h, self.w, self.rgba = kc, h, w, rgba
        nch = 3 if rgba else 1
        self.planes = [[edge_plane(seed + 17 * i, c, h, w) for c in range(nch)] for i in range(k)]
        self.keep = []  # torch tensors behind wrapped planes
        self.imgs = [self._image(p, storage) for p in self.planes]

    def _image(self, planes, storage):
        kc = self.kc
        if storage == "pool":
            return kc.SlotImage.from_planes(planes + ([np.ones((self.h, self.w), np.float32)] if self.rgba else []))
        import torch
        from kanter_core_amd import _lib
        L = _lib.load()
        pitch = (self.w + 3) // 4 * 4 + 12
        handles = []
        for p in planes:
            t = torch.full((self.h, pitch), float("nan"), device="cuda")
            t[:, :self.w] = torch.from_numpy(p).cuda()
            self.keep.append(t)
            h = C.c_void_p()
            assert L.kc_plane_wrap(t.data_ptr(), self.w, self.h, pitch * 4, C.byref(h)) == 0
            handles.append(h)
        torch.cuda.synchronize()
        img = C.c_void_p()
        if self.rgba:
            a = C.c_void_p()
            assert L.kc_plane_const(self.w, self.h, 1.0, C.byref(a)) == 0
            assert L.kc_image_rgba((C.c_void_p * 4)(*(handles + [a])), C.byref(img)) == 0
            handles.append(a)
        else:
            assert L.kc_image_gray(handles[0], C.byref(img)) == 0
        for h in handles:
            L.kc_plane_release(h)
        return kc.SlotImage(img.value)

    def const(self, vals):
        """A constant image: one value per channel (RGBA: three different ones)."""
        if not self.rgba:
            return self.kc.SlotImage.from_value((self.w, self.h), vals[0], False)
        from kanter_core_amd import _lib
        L = _lib.load()
        hs = [C.c_void_p() for _ in range(4)]
        for h, v in zip(hs, list(vals[:3]) + [1.0]):
            assert L.kc_plane_const(self.w, self.h, float(v), C.byref(h)) == 0
        img = C.c_void_p()
        assert L.kc_image_rgba((C.c_void_p * 4)(*hs), C.byref(img)) == 0
        for h in hs:
            L.kc_plane_release(h)
        return self.kc.SlotImage(img.value)

    def value(self, operand, c):
        kind, v = operand
        return self.planes[v][c] if kind == "p" else np.full((self.h, self.w), v[c], np.float32)


def run_program(kc, orc, inp, start, steps, hold=None, pre=False):
    """Builds the program lazily, drops the inputs not in `hold` (indices; None: keep all), returns (result image, expected
    planes).  start / operands: ("p", k) input plane k, ("c", (r, g, b)) a constant; steps: (Mix type, right, operand) --
    right: the running value is the Mix's right input.  pre: the start is a chain (x 1) that runs on its own before the
    measured launch (see the module docstring)."""
    nch = 3 if inp.rgba else 1
    imgs = list(inp.imgs)
    acc = imgs[start[1]] if start[0] == "p" else inp.const(start[1])
    t = None
    if pre:
        t = acc = kc.mix_process(acc, inp.const((1.0, 1.0, 1.0)), kc.MixType.Multiply)
        imgs[start[1]] = None  # the start is t's result from here on
    want = [inp.value(start, c) for c in range(nch)]
    for op, right, opnd in steps:
        x = imgs[opnd[1]] if opnd[0] == "p" else inp.const(opnd[1])
        acc = kc.mix_process(x, acc, kc.MixType.parse(op)) if right else kc.mix_process(acc, x, kc.MixType.parse(op))
        want = [orc.mix_plane(op, inp.value(opnd, c), want[c]) if right else orc.mix_plane(op, want[c], inp.value(opnd, c))
                for c in range(nch)]
    if t is not None:
        t.materialize()
        imgs[start[1]] = t
    if hold is not None:
        for k in range(len(imgs)):
            if k not in hold:
                imgs[k] = None
    inp.imgs = imgs  # what the test still holds
    return acc, want


def snapshot(kc):
    return {n: kc.stats_counter(n) for n in COUNTERS}, kc.stats()["kernel_launches"]


def measure(kc, img):
    """Runs the program (kc_image_to_f32: one batched launch for R, G, B; the constant alpha is not filled on the device)."""
    before = snapshot(kc)
    planes = img.planes()
    now = snapshot(kc)
    return {n: now[0][n] - before[0][n] for n in COUNTERS if now[0][n] != before[0][n]}, now[1] - before[1], planes


def check(got, want, rgba, pow_last, what):
    if rgba:
        assert_planes(got[3:], [np.ones_like(want[0])], what=what + " alpha")
        got = got[:3]
    if pow_last:
        for c, (g, w) in enumerate(zip(got, want)):
            bad = pow_mismatch(g, w)
            assert not bad.any(), "%s plane %d: %d Pow mismatches" % (what, c, int(bad.sum()))
    else:
        assert_planes(got, want, what=what)


SEEN = set()


def expect_one(kc, img, counter, extra=()):
    seen, launches, planes = measure(kc, img)
    want = {n: 1 for n in (counter,) + tuple(extra)}
    assert launches == 1 and seen == want, "%d launches, counters %s, expected %s" % (launches, seen, want)
    SEEN.add(counter)
    return planes


# ------------------------------------------------------------------------------------------------ chain1
def chain1_steps(code, operand):
    op, right, inv = CODE_OF[code]
    steps = [(op, right, operand)]
    if inv:
        steps.append(("Subtract", True, ("c", CONSTS[2])))
    return steps, right


# (id, code, start, operand, rgba, storage, (w, h), cache_budget_mb or None, held inputs or None, nt bits)
CHAIN1_CASES = []
for code in CODE_OF:
    CHAIN1_CASES.append(("%s_nt0_rgba_pitched" % code, code, ("p", 0), ("p", 1), True, "pool", (130, 37), None, None, 0))
    CHAIN1_CASES.append(("%s_nt7" % code, code, ("p", 0), ("p", 1), False, "pool", (512, 512), 0, None, 7))
# every combination the policy reaches (module docstring)
for code in ("ADD", "POW_R", "SUBR_INV"):
    for nt, mb, hold in ((4, 2, [0, 1]), (4, 2, []), (5, 1, [1]), (6, 1, [0]), (6, 1, [])):
        CHAIN1_CASES.append(("%s_nt%d_hold%s" % (code, nt, "".join(map(str, hold)) or "none"), code, ("p", 0), ("p", 1), False, "pool", (512, 512), mb, hold, nt))
CHAIN1_CASES += [
    # a constant on either side: one input plane (its bit, the result's)
    ("POW_L_const_start", "POW_L", ("c", CONSTS[0]), ("p", 0), True, "pool", (64, 40), None, None, 0),
    ("POW_L_const_operand", "POW_L", ("p", 0), ("c", CONSTS[3]), True, "wrapped", (37, 19), None, None, 0),
    ("MUL_const_start_nt6", "MUL", ("c", CONSTS[1]), ("p", 0), False, "pool", (512, 512), 0, None, 6),
    ("DIV_R_const_operand_nt5", "DIV_R", ("p", 0), ("c", CONSTS[2]), False, "pool", (512, 512), 0, None, 5),
    ("SUB_L_const_operand_nt4", "SUB_L", ("p", 0), ("c", CONSTS[1]), False, "pool", (512, 512), 1, [0], 4),
    ("SUB_L_wrapped_gray", "SUB_L", ("p", 0), ("p", 1), False, "wrapped", (130, 33), None, None, 0),
    ("ADD_INV_wrapped_rgba", "ADD_INV", ("p", 0), ("p", 1), True, "wrapped", (64, 21), None, None, 0),
    ("POW_R_1024x1040", "POW_R", ("p", 0), ("p", 1), True, "pool", (1024, 1040), None, None, 0),
]


@pytest.mark.parametrize("case", CHAIN1_CASES, ids=[c[0] for c in CHAIN1_CASES])
def test_chain1_form(kc, orc, options, case):
    name, code, start, operand, rgba, storage, (w, h), mb, hold, nt = case
    kc.set_option("chain1", 1)
    k = max([v[1] for v in (start, operand) if v[0] == "p"]) + 1
    inp = Inputs(kc, k, h, w, rgba, storage)
    steps, right = chain1_steps(code, operand)
    img, want = run_program(kc, orc, inp, start, steps, hold=hold, pre=right)
    if mb is not None:
        kc.set_option("cache_budget_mb", mb)
    got = expect_one(kc, img, "chain1_nt%d" % nt, ("chain1_launches",))
    check(got, want, rgba, code.startswith("POW"), name)


# ------------------------------------------------------------------------------------------------ the interpreter
OPS = {0: ["Add", "Subtract", "Multiply"], 1: ["Add", "Subtract", "Multiply", "Divide"], 2: ["Add", "Subtract", "Multiply", "Divide"]}


def make_program(k, n, mode, const_start, seed):
    """n steps over k input planes (each used at least once) and per-channel constants; MODE 1 holds a divide, MODE 2 ends
    in Pow.  A constant start takes a plane operand first (a Mix of two constants is folded on the host)."""
    rng = np.random.default_rng(seed)
    start = ("c", CONSTS[seed % len(CONSTS)]) if const_start else ("p", 0)
    need = list(range(k)) if const_start else list(range(1, k))
    steps = []
    for i in range(n):
        if need and (i >= n - len(need) - 1 or rng.random() < 0.6):
            opnd = ("p", need.pop(0))
        elif rng.random() < 0.7 or (i == 0 and const_start):
            opnd = ("p", int(rng.integers(k)))
        else:
            opnd = ("c", CONSTS[int(rng.integers(len(CONSTS)))])
        op = OPS[mode][int(rng.integers(len(OPS[mode])))]
        if mode == 1 and i == n // 2:
            op = "Divide"
        if mode == 2 and i == n - 1:
            op = "Pow"
        right = bool(rng.integers(2)) and not (i == 0 and const_start)
        steps.append((op, right, opnd))
    assert not need
    return start, steps


# (id, K, mode, unroll, steps, constant start, rgba, storage, (w, h), budget, max_blocks, counter)
INTERP_CASES = []
LAYOUTS = [(False, "pool", (256, 24)), (True, "pool", (130, 37)), (False, "wrapped", (37, 29)), (True, "wrapped", (64, 17)),
           (False, "pool", (130, 9))]
STEP_COUNTS = [2, 3, 64, 7, 10, 5, 17, 4, 33, 6]
for i, (k, u) in enumerate([(k, u) for k in range(1, 5) for u in UNROLLS]):
    rgba, storage, size = LAYOUTS[i % len(LAYOUTS)]
    INTERP_CASES.append(("m0_k%d_u%d" % (k, u), k, 0, u, max(k + 1, STEP_COUNTS[i % len(STEP_COUNTS)]), i % 3 == 1, rgba, storage, size, None,
                         None, "chain_interp_k%d_u%d_m0" % (k, u)))
for mode, u in ((0, 4), (1, 4), (2, 1)):
    for k in range(1, 5):
        rgba, storage, size = LAYOUTS[(k + mode) % len(LAYOUTS)]
        n = max(k + 1, STEP_COUNTS[(3 * k + mode) % len(STEP_COUNTS)])
        if mode:
            INTERP_CASES.append(("m%d_k%d" % (mode, k), k, mode, 0, n, k % 2 == 0, rgba, storage, size, None, None,
                                 "chain_interp_k%d_u%d_m%d" % (k, u, mode)))
        INTERP_CASES.append(("m%d_k%d_nt" % (mode, k), k, mode, 0, n + 1, k == 3, False, "pool", (512, 512), 0, None,
                             "chain_interp_k%d_u%d_m%d_nt" % (k, u, mode)))
INTERP_CASES += [
    # grid stride: the workgroups loop over the plane, the last trip partial (4096 floats a trip per workgroup at U = 4,
    # 1024 at U = 1)
    ("stride_m0_u4_blocks1", 2, 0, 4, 9, False, True, "pool", (130, 37), None, 1, "chain_interp_k2_u4_m0"),
    ("stride_m0_u8_blocks3", 3, 0, 8, 12, True, False, "pool", (512, 100), None, 3, "chain_interp_k3_u8_m0"),
    ("stride_m0_u4_blocks3_nt", 2, 0, 4, 8, False, False, "pool", (512, 512), 0, 3, "chain_interp_k2_u4_m0_nt"),
    ("stride_m1_blocks3", 2, 1, 0, 6, False, False, "wrapped", (200, 100), None, 3, "chain_interp_k2_u4_m1"),
    ("stride_m2_blocks1", 1, 2, 0, 4, False, True, "pool", (37, 41), None, 1, "chain_interp_k1_u1_m2"),
    ("stride_m2_blocks3_nt", 4, 2, 0, 5, False, False, "pool", (512, 512), 0, 3, "chain_interp_k4_u1_m2_nt"),
    # many workgroups
    ("m0_1024x1040", 3, 0, 0, 20, False, True, "pool", (1024, 1040), None, None, "chain_interp_k3_u4_m0"),
    ("m2_1024x1040", 2, 2, 0, 3, False, True, "pool", (1024, 1040), None, None, "chain_interp_k2_u1_m2"),
]


@pytest.mark.parametrize("case", INTERP_CASES, ids=[c[0] for c in INTERP_CASES])
def test_interpreter_form(kc, orc, options, case):
    name, k, mode, unroll, n, const_start, rgba, storage, (w, h), mb, blocks, counter = case
    kc.set_option("chain1", 0)
    kc.set_specialize(0)
    kc.set_option("chain_unroll", unroll)
    if blocks is not None:
        kc.set_option("max_blocks", blocks)
    inp = Inputs(kc, k, h, w, rgba, storage)
    start, steps = make_program(k, n, mode, const_start, seed=len(name) * 31 + n)
    img, want = run_program(kc, orc, inp, start, steps, hold=[] if mb is not None else None)
    if mb is not None:
        kc.set_option("cache_budget_mb", mb)
    got = expect_one(kc, img, counter)
    check(got, want, rgba, mode == 2, name)


# chain_kernel_k0<2>: constants only (Value ^ Value, or constant planes of a size); further constant steps ride along.  The
# Pow of a longer program is exact (2^3, 0.25^-0.5 ...): nothing for the steps after it to amplify.
K0_CASES = [
    # (id, (w, h), rgba, (base, exponent) per channel, further steps, max_blocks)
    ("value_pow_value", (1, 1), False, [(0.33, 0.66)], [], None),
    ("rgba_channels_differ", (130, 37), True, [(2.0, 3.0), (0.25, -0.5), (-8.0, 2.0)],
     [("Add", False, ("c", CONSTS[0])), ("Multiply", True, ("c", CONSTS[2]))], None),
    ("gray_edges", (64, 64), False, [(0.0, -1.0)], [], None),
    ("stride_blocks3", (512, 40), True, [(1.5, 2.0), (4.0, 0.5), (-2.0, -1.0)], [("Subtract", True, ("c", CONSTS[1]))], 3),
    ("rgba_1024x1040", (1024, 1040), True, [(3.0, 0.5), (7.0, 1.25), (1e-30, 0.25)], [], None),
]


@pytest.mark.parametrize("case", K0_CASES, ids=[c[0] for c in K0_CASES])
def test_k0_form(kc, orc, options, case):
    name, (w, h), rgba, pairs, steps, blocks = case
    kc.set_option("chain1", 0)
    kc.set_specialize(0)
    if blocks is not None:
        kc.set_option("max_blocks", blocks)
    inp = Inputs(kc, 0, h, w, rgba, "pool")
    bases = tuple(p[0] for p in pairs) * 3
    exps = tuple(p[1] for p in pairs) * 3
    if (w, h) == (1, 1):
        img = kc.mix_process(kc.value_process(bases[0]), kc.value_process(exps[0]), kc.MixType.Pow)
    else:
        img = kc.mix_process(inp.const(bases), inp.const(exps), kc.MixType.Pow)
    nch = 3 if rgba else 1
    want = [orc.mix_plane("Pow", np.full((h, w), bases[c], np.float32), np.full((h, w), exps[c], np.float32)) for c in range(nch)]
    for op, right, opnd in steps:
        x = inp.const(opnd[1])
        img = kc.mix_process(x, img, kc.MixType.parse(op)) if right else kc.mix_process(img, x, kc.MixType.parse(op))
        want = [orc.mix_plane(op, inp.value(opnd, c), want[c]) if right else orc.mix_plane(op, want[c], inp.value(opnd, c))
                for c in range(nch)]
    got = expect_one(kc, img, "chain_k0_m2")
    check(got, want, rgba, not steps, name)


# ------------------------------------------------------------------------------------------------ compiled kernels
# a two-input program (start A, operand B): its cache-policy bits through the policy (A is input 0, B input 1)
SPEC_CASES = [
    # (id, steps, rgba, (w, h), budget, held inputs, mask)
    ("none", 4, True, (130, 37), None, None, 0x000),
    ("stream_result", 4, False, (512, 512), 2, [], 0x100),
    ("stream_a_and_result", 4, False, (512, 512), 1, [1], 0x101),
    ("stream_b_and_result", 4, False, (512, 512), 1, [0], 0x102),
    ("stream_all", 4, False, (512, 512), 0, [0, 1], 0x103),
    ("none_1024x1040", 2, True, (1024, 1040), None, None, 0x000),
]


@pytest.mark.parametrize("case", SPEC_CASES, ids=[c[0] for c in SPEC_CASES])
def test_compiled_form(kc, orc, options, case):
    name, n, rgba, (w, h), mb, hold, mask = case
    kc.set_specialize(2)
    inp = Inputs(kc, 2, h, w, rgba, "pool")
    steps = [("Add", False, ("p", 1)), ("Multiply", True, ("c", CONSTS[0])), ("Subtract", True, ("p", 0)),
             ("Divide", False, ("p", 1))][:n]
    img, want = run_program(kc, orc, inp, ("p", 0), steps, hold=hold)
    if mb is not None:
        kc.set_option("cache_budget_mb", mb)
    got = expect_one(kc, img, "specialized_nt_%03x" % mask)
    check(got, want, rgba, False, name)


def test_every_instantiation_ran(kc):
    """Every form a graph can reach is some case's expected form, and ran in this process."""
    declared = {"chain1_nt%d" % c[-1] for c in CHAIN1_CASES} | {c[-1] for c in INTERP_CASES} | {"chain_k0_m2"}
    assert not set(UNREACHABLE) & declared
    assert set(INSTANTIATIONS) <= declared, sorted(set(INSTANTIATIONS) - declared)
    missing = [n for n in INSTANTIATIONS if kc.stats_counter(n) < 1]
    assert not missing, missing
    assert set(INSTANTIATIONS) <= SEEN, sorted(set(INSTANTIATIONS) - SEEN)
    assert all(kc.stats_counter(n) == 0 for n in UNREACHABLE)
