"""Mix(Pow) on every route that launches it, against a high-precision reference (tests/pow_ref.py): away from an f32 rounding
boundary the result is the correctly rounded power, within pow_positive's derived error band of one either neighbour
(pow_ref.pow_band).  Routes: the one-step kernels (acc ^ x and x ^ acc; plane ^ plane, plane ^ constant, constant ^ plane),
the step interpreter (MODE 2) with and without its nontemporal form, chain_kernel_k0 (Value ^ Value), and a kernel compiled for
the program at run time; on the same inputs they agree bit for bit.  Special values (zeros of both signs, subnormals, +-1,
infinities, NaN, negative bases with integer and non-integer exponents) are bit-exact against the oracle's powf and against
pow in f64 rounded to f32.  Random multi-step programs holding Pow give the same bits in the interpreter and compiled."""
import numpy as np
import pytest

import pow_ref as P
from util import SEED_A, bit_equal, splitmix_plane, with_edge_cases

pytestmark = pytest.mark.gpu

N = 512  # a region is N x N pairs (2^18)
K0_PAIRS = 256


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    return kc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


@pytest.fixture
def options(kc):
    saved = {n: kc.get_option(n) for n in ("cache_budget_mb", "chain1")}
    spec = kc.get_specialize()
    yield
    for n, v in saved.items():
        kc.set_option(n, v)
    kc.set_specialize(spec)


def counted(kc, name, fn):
    before = kc.stats_counter(name)
    out = fn()
    assert kc.stats_counter(name) == before + 1, name
    return out


def gray(kc, p):
    return kc.SlotImage.from_planes([np.ascontiguousarray(p, np.float32)])


def pow_routes(kc, a, b):
    """{route: result plane} for a ^ b (planes of one shape)."""
    h, w = a.shape
    budget = kc.get_option("cache_budget_mb")
    A, B = gray(kc, a), gray(kc, b)
    one = kc.SlotImage.from_value((w, h), 1.0, False)
    out = {}
    kc.set_option("chain1", 1)
    out["chain1_pow_l"] = counted(kc, "chain1_nt0", lambda: kc.mix_process(A, B, kc.MixType.Pow).planes()[0])
    # x ^ acc: the running value is B (a chain B x 1 that has run on its own), the operand A
    t = kc.mix_process(B, one, kc.MixType.Multiply)
    r = kc.mix_process(A, t, kc.MixType.Pow)
    t.materialize()
    out["chain1_pow_r"] = counted(kc, "chain1_nt0", lambda: r.planes()[0])
    kc.set_option("chain1", 0)
    kc.set_specialize(0)
    out["interp"] = counted(kc, "chain_interp_k2_u1_m2", lambda: kc.mix_process(A, B, kc.MixType.Pow).planes()[0])
    kc.set_option("cache_budget_mb", 0)
    out["interp_nt"] = counted(kc, "chain_interp_k2_u1_m2_nt", lambda: kc.mix_process(A, B, kc.MixType.Pow).planes()[0])
    kc.set_option("cache_budget_mb", budget)
    kc.set_specialize(2)
    out["compiled"] = counted(kc, "specialized_nt_000", lambda: kc.mix_process(A, B, kc.MixType.Pow).planes()[0])
    kc.set_specialize(1)
    kc.set_option("chain1", 1)
    return out


def k0_route(kc, a, b):
    kc.set_specialize(0)
    got = np.empty(len(a), np.float32)
    for i, (x, y) in enumerate(zip(a, b)):
        img = kc.mix_process(kc.value_process(float(x)), kc.value_process(float(y)), kc.MixType.Pow)
        got[i] = img.planes()[0][0, 0]
    kc.set_specialize(1)
    return got


def assert_contract(got, a, b, what):
    bad, frac = P.contract_failures(got.reshape(-1), a.reshape(-1), b.reshape(-1))
    assert frac < 2.0 ** -8, "%s: the band covers %.3g of the samples" % (what, frac)
    if len(bad):
        a, b, g = a.reshape(-1), b.reshape(-1), got.reshape(-1)
        cr, _, _ = P.correctly_rounded(a[bad], b[bad])
        raise AssertionError("%s: %d of %d off the contract, e.g. %s" % (
            what, len(bad), g.size, [(float(a[i]), float(b[i]), float(g[i]), float(c)) for i, c in zip(bad[:4], cr[:4])]))


@pytest.mark.parametrize("name", P.REGIONS)
def test_pow_regions_on_every_route(kc, options, name):
    a, b = P.region(name, N * N)
    a2, b2 = a.reshape(N, N), b.reshape(N, N)
    routes = pow_routes(kc, a2, b2)
    assert_contract(routes["chain1_pow_l"], a, b, name + " chain1_pow_l")
    for r, got in routes.items():
        assert bit_equal(got, routes["chain1_pow_l"]), "%s: %s differs from chain1_pow_l" % (name, r)
    # a constant on either side: plane ^ b[0] and a[0] ^ plane
    kc.set_option("chain1", 1)
    bc = np.full_like(a2, b2[0, 0])
    ac = np.full_like(b2, a2[0, 0])
    pc = counted(kc, "chain1_nt0", lambda: kc.mix_process(gray(kc, a2), kc.SlotImage.from_value((N, N), float(b2[0, 0]), False),
                                                          kc.MixType.Pow).planes()[0])
    cp = counted(kc, "chain1_nt0", lambda: kc.mix_process(kc.SlotImage.from_value((N, N), float(a2[0, 0]), False), gray(kc, b2),
                                                          kc.MixType.Pow).planes()[0])
    assert_contract(pc, a2, bc, name + " plane ^ constant")
    assert_contract(cp, ac, b2, name + " constant ^ plane")
    # Value ^ Value (chain_kernel_k0): a few hundred of the pairs, each its own 1 x 1 launch
    i = np.linspace(0, N * N - 1, K0_PAIRS).astype(int)
    k0 = k0_route(kc, a[i], b[i])
    assert bit_equal(k0, routes["chain1_pow_l"].reshape(-1)[i]), name + " k0"


def test_pow_special_values_bit_exact(kc, orc, options):
    a, b = P.special_pairs()
    want = P.f64_rounded(a, b)
    assert bit_equal(orc.mix_plane("Pow", a, b), want)
    n = a.shape[0]
    # padded to a plane of whole quads: every pair sits at its own lane
    ap, bp = np.ones((n, 28), np.float32), np.ones((n, 28), np.float32)
    ap[:, :n], bp[:, :n] = a, b
    routes = pow_routes(kc, ap, bp)
    for r, got in routes.items():
        g = got[:, :n]
        bad = ~((g.view(np.uint32) == want.view(np.uint32)) | (np.isnan(g) & np.isnan(want)))
        assert not bad.any(), "%s: %s" % (r, [(float(x), float(y), float(gg), float(ww)) for x, y, gg, ww in
                                              zip(a[bad][:6], b[bad][:6], g[bad][:6], want[bad][:6])])
    k0 = k0_route(kc, a.reshape(-1), b.reshape(-1))
    assert bit_equal(k0, want.reshape(-1)), "k0"


def test_random_programs_with_pow_interpreter_equals_compiled(kc, options):
    """Multi-step programs with Pow anywhere (a one-ulp Pow difference would be amplified by the steps after it, so the
    two device paths must agree exactly); the inputs carry the IEEE edge cases."""
    rng = np.random.default_rng(23)
    h, w = 48, 72
    planes = [with_edge_cases(splitmix_plane(SEED_A + i, 0, h, w) * np.float32(3.0), i + 1) for i in range(3)]
    kc.set_option("chain1", 0)
    ops = ["Add", "Subtract", "Multiply", "Divide", "Pow", "Pow"]
    for trial in range(10):
        n = int(rng.integers(2, 9))
        prog = [(ops[int(rng.integers(len(ops)))], bool(rng.integers(2)), int(rng.integers(4))) for _ in range(n)]
        if all(op != "Pow" for op, _, _ in prog):
            prog[int(rng.integers(n))] = ("Pow",) + prog[0][1:]
        results = []
        for mode in (0, 2):
            kc.set_specialize(mode)
            imgs = [gray(kc, p) for p in planes]
            acc = imgs[0]
            for op, right, k in prog:
                x = imgs[k] if k < 3 else kc.SlotImage.from_value((w, h), 0.75, False)
                acc = kc.mix_process(x, acc, kc.MixType.parse(op)) if right else kc.mix_process(acc, x, kc.MixType.parse(op))
            results.append(acc.planes()[0])
        assert bit_equal(results[0], results[1]), "trial %d: %s" % (trial, prog)
