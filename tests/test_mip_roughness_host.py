"""The host half of roughness chains (kc_image_build_roughness_mips, include/kanter_core_amd.h), on a machine without a GPU:
kc_mip_unit_normal and kc_mip_roughness_texel equal tests/mip_roughness_ref.py bit for bit, the reference itself has the
properties the rule is there for (a flat map leaves the plain chain untouched, also after 8-bit quantisation; cancelling normals
give exactly 1; more spread never gives less roughness; results stay in [0, 1]), and the entry points refuse what the contract
says, in its order, as far as that is reachable without a device."""
import ctypes as C
import itertools

import numpy as np
import pytest

import mip_ref
import mip_roughness_ref as ref
from util import SEED_A, bit_equal, synthetic_rgba

KC_ERR_NO_DEVICE, KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 101, 102, 104
MIP_PER_LEVEL = 2
F = np.float32
FLT_MAX = np.finfo(F).max
POWERS = [2.0 ** -10, 1.0, 65536.0]
R_SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, 1e-39, -0.25, -3e38, 1.25, 3e38, 1.0, 0.5], F)
E_SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, 3e38, -3e38, FLT_MAX, 0.5, 0.5 + 2.0 ** -24, 0.5 - 2.0 ** -24, 1.0], F)


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    return kc


@pytest.fixture(scope="module")
def L():
    from kanter_core_amd import _lib
    return _lib.load()


def check_units(kc, triples, what):
    t = np.ascontiguousarray(triples, F)
    want = np.stack(ref.unit(t[:, 0], t[:, 1], t[:, 2]), axis=1)
    got = np.stack([kc.mip_unit_normal(e) for e in t])
    assert got.dtype == F and np.isfinite(got).all(), what
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert bad.size == 0, "%s: %d of %d differ, e.g. %s got %s want %s" % (what, bad.size, len(t), t[bad[0]], got[bad[0]], want[bad[0]])


def check_texels(kc, m, r, what):
    """Every row of m (n, 3) with every value of r (n,), at every power of POWERS."""
    m, r = np.ascontiguousarray(m, F), np.ascontiguousarray(r, F)
    assert len(m) == len(r)
    for power in POWERS:
        want = ref.texel(m[:, 0], m[:, 1], m[:, 2], r, power)
        got = np.array([kc.mip_roughness_texel(m[i], r[i], power) for i in range(len(m))], F)
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        bad = np.flatnonzero(~same)
        assert bad.size == 0, "%s power %g: %d of %d differ, e.g. m %s r %s got %s want %s" % (
            what, power, bad.size, len(m), m[bad[0]], r[bad[0]], got[bad[0]], want[bad[0]])


def unit_vectors(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def box(a, b, c, d):
    return ((a + b) + (c + d)) * F(0.25)


# ------------------------------------------------------------------ the two functions against the reference
def test_unit_normal_equals_the_reference(kc):
    axis = np.concatenate([np.linspace(0.0, 1.0, 9, dtype=F), np.array([0.3, 0.8535534, 1.25, -0.25], F)])
    check_units(kc, list(itertools.product(axis, repeat=3)), "grid")
    rng = np.random.default_rng(SEED_A)
    check_units(kc, rng.random((2048, 3), dtype=F), "random")
    n = unit_vectors(rng, 2048)
    check_units(kc, (n * 0.5 + 0.5).astype(F), "unit")
    check_units(kc, np.round((n * 0.5 + 0.5) * 255.0).astype(F) / F(255.0), "8-bit")
    check_units(kc, list(itertools.product(E_SPECIALS, repeat=3)), "specials")
    flat = np.array([0.0, 0.0, 1.0], F)
    for e in ([0.5, 0.5, 0.5], [np.nan, 0.5, 1.0], [0.5, np.inf, 1.0], [0.5, 0.5, -np.inf], [FLT_MAX, 0.5, 0.5], [0.5, 0.5, 1.0]):
        assert bit_equal(kc.mip_unit_normal(e), flat), e


def test_texel_equals_the_reference_on_a_grid(kc):
    axis = np.array([-1.0, -0.7071068, -0.5, -0.1, 0.0, 1e-3, 0.25, 0.5774, 0.9, 1.0], F)
    m = np.array(list(itertools.product(axis, repeat=3)), F)
    for r in (0.0, 0.05, 0.3, 0.5, 0.9, 1.0):
        check_texels(kc, m, np.full(len(m), r, F), "grid r=%g" % r)


def test_texel_equals_the_reference_on_random_vectors(kc):
    rng = np.random.default_rng(SEED_A + 1)
    m = unit_vectors(rng, 4096) * rng.random((4096, 1)) ** 0.25  # |m| <= 1, most of them long
    check_texels(kc, m.astype(F), rng.random(4096, dtype=F), "random")
    short = unit_vectors(rng, 512) * 10.0 ** rng.uniform(-24, 0, (512, 1))  # down to sums of squares that underflow
    check_texels(kc, short.astype(F), rng.random(512, dtype=F), "short")


def test_texel_equals_the_reference_on_boxes_of_perturbed_unit_vectors(kc):
    rng = np.random.default_rng(SEED_A + 2)
    n = 4096
    base = unit_vectors(rng, n)
    for spread in (0.0, 1e-4, 1e-2, 0.3, 3.0):
        four = []
        for _ in range(4):
            v = base + spread * rng.standard_normal((n, 3))
            enc = (v / np.linalg.norm(v, axis=1, keepdims=True) * 0.5 + 0.5).astype(F)
            four.append(np.stack(ref.unit(enc[:, 0], enc[:, 1], enc[:, 2]), axis=1))
        m = box(*four)
        assert m.dtype == F
        check_texels(kc, m, rng.random(n, dtype=F), "spread %g" % spread)


def test_texel_at_length_zero_one_and_beside_one(kc):
    one = F(1.0)
    beside = [np.nextafter(one, F(0.0)), one, np.nextafter(one, F(2.0)), F(1.0 - 2.0 ** -15), F(1.0 - 2.0 ** -14), F(1.0 - 2.0 ** -13),
              F(1.0 / (1.0 + 2.0 ** -14)), np.nextafter(F(1.0 / (1.0 + 2.0 ** -14)), F(0.0)), np.nextafter(F(1.0 / (1.0 + 2.0 ** -14)), F(2.0))]
    rows = [[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [1e-30, 0.0, 0.0], [1e-23, 1e-23, 0.0], [1e-19, 0.0, 0.0]]  # l == 0: exact, or q underflows
    for l in beside:
        rows += [[l, 0.0, 0.0], [0.0, -l, 0.0], [0.0, 0.0, l]]
    m = np.array(rows, F)
    for r in (0.0, 0.3, 1.0, 1.5, -0.5):
        check_texels(kc, m, np.full(len(m), r, F), "lengths r=%g" % r)
    for power in POWERS:
        assert kc.mip_roughness_texel([0.0, 0.0, 0.0], 0.25, power) == F(1.0)
        assert kc.mip_roughness_texel([1e-30, 0.0, 0.0], 0.25, power) == F(1.0)
        for r in (0.25, 1.5, -0.5, -0.0, 1e-45):  # a flat footprint keeps the plain box, unclamped
            for l in (one, np.nextafter(one, F(0.0)), np.nextafter(one, F(2.0))):
                assert bit_equal(kc.mip_roughness_texel([0.0, l, 0.0], r, power), F(r)), (r, l, power)


def test_texel_on_special_roughness_values(kc):
    ms = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.0, 0.1, 0.0], [0.6, 0.0, 0.7], [1e-20, 0.0, 0.0]], F)
    m = np.repeat(ms, len(R_SPECIALS), axis=0)
    r = np.tile(R_SPECIALS, len(ms))
    check_texels(kc, m, r, "special r")
    for row in ms:
        assert np.isnan(kc.mip_roughness_texel(row, np.nan, 1.0))  # NaN stays NaN, also where the normals cancel


def test_null_arguments_shapes_and_power_are_refused(kc, L):
    a, out, d = np.array([0.5, 0.5, 1.0], F), np.full(3, 7.0, F), C.c_float(7.0)
    assert L.kc_mip_unit_normal(None, out.ctypes.data) == KC_ERR_INVALID_ARG
    assert L.kc_mip_unit_normal(a.ctypes.data, None) == KC_ERR_INVALID_ARG
    assert (out == 7.0).all()
    assert L.kc_mip_unit_normal(a.ctypes.data, out.ctypes.data) == 0 and bit_equal(out, np.array([0.0, 0.0, 1.0], F))
    assert L.kc_mip_roughness_texel(None, 0.5, 1.0, C.byref(d)) == KC_ERR_INVALID_ARG
    assert L.kc_mip_roughness_texel(a.ctypes.data, 0.5, 1.0, None) == KC_ERR_INVALID_ARG
    for power in (0.0, -1.0, float("nan"), float("inf"), 65537.0):
        assert L.kc_mip_roughness_texel(a.ctypes.data, 0.5, power, C.byref(d)) == KC_ERR_INVALID_ARG, power
    assert d.value == 7.0
    with pytest.raises(ValueError):
        kc.mip_unit_normal([0.5, 0.5])
    with pytest.raises(ValueError):
        kc.mip_roughness_texel([0.5, 0.5], 0.5)


def test_refusals_and_their_order_without_a_device(L):
    """Flags first, then the arguments and the power, then KC_ERR_NO_DEVICE: no image exists before kc_init, so an opaque non-NULL
    handle is never looked at before it."""
    no_device = not L.kc_is_initialized()  # with a device the calls that pass the argument checks would read the handles
    fake = C.c_void_p(0x1000)
    arr, count = (C.c_void_p * 16)(), C.c_uint32(77)
    build = L.kc_image_build_roughness_mips
    ok = (fake, 0, fake, C.c_float(1.0), 0, arr, 16, C.byref(count))

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return a
    for flags in (1, 4, 32, 64, 0x80000000, MIP_PER_LEVEL | 32):
        assert build(*with_(4, flags)) == KC_ERR_UNSUPPORTED, flags
        assert build(None, 0, None, C.c_float(-1.0), flags, None, 0, None) == KC_ERR_UNSUPPORTED, flags  # before the arguments
    for i in (0, 2, 5, 7):
        assert build(*with_(i, None)) == KC_ERR_INVALID_ARG, i
    for power in (0.0, -1.0, float("nan"), float("inf"), 65536.5):
        assert build(*with_(3, C.c_float(power))) == KC_ERR_INVALID_ARG, power
    if no_device:
        for flags in (0, MIP_PER_LEVEL):
            assert build(*with_(4, flags)) == KC_ERR_NO_DEVICE
        assert build(*with_(3, C.c_float(65536.0))) == KC_ERR_NO_DEVICE and build(*with_(3, C.c_float(2.0 ** -10))) == KC_ERR_NO_DEVICE
    assert count.value == 77
    # the level exporters: the flags under kc_image_to_bc's rule, the arguments and the format, then the device
    host = (C.c_uint8 * 64)()
    levels = (C.c_void_p * 1)(0x1000)
    to_bc, dds = L.kc_image_levels_to_bc_mips, L.kc_image_levels_write_dds
    for fmt, flags in ((4, 1), (5, 1), (95, 1), (1, 2), (98, 32), (1, 64)):  # sRGB with BC4 / BC5 / BC6H; the chain builders' flags
        assert to_bc(levels, 1, fmt, flags, host, 64) == KC_ERR_UNSUPPORTED, (fmt, flags)
        assert dds(levels, 1, b"/nonexistent/x.dds", fmt, flags) == KC_ERR_UNSUPPORTED, (fmt, flags)
    assert to_bc(None, 0, 4, 2, None, 0) == KC_ERR_UNSUPPORTED
    assert to_bc(None, 1, 4, 0, host, 64) == KC_ERR_INVALID_ARG
    assert to_bc(levels, 1, 4, 0, None, 64) == KC_ERR_INVALID_ARG
    assert to_bc(levels, 0, 4, 0, host, 64) == KC_ERR_INVALID_ARG
    assert to_bc(levels, 1, 99, 0, host, 64) == KC_ERR_INVALID_ARG
    assert dds(None, 1, b"/nonexistent/x.dds", 4, 0) == KC_ERR_INVALID_ARG
    assert dds(levels, 1, None, 4, 0) == KC_ERR_INVALID_ARG
    assert dds(levels, 1, b"/nonexistent/x.dds", 99, 0) == KC_ERR_INVALID_ARG
    if no_device:
        assert to_bc(levels, 1, 4, 0, host, 64) == KC_ERR_NO_DEVICE
        assert to_bc(levels, 1, 1, 1, host, 64) == KC_ERR_NO_DEVICE
        assert dds(levels, 1, b"/nonexistent/x.dds", 4, 0) == KC_ERR_NO_DEVICE
    assert not any(host)


# ------------------------------------------------------------------ the reference itself
def flat_normals(w, h, n=(0.3, -0.2, 0.9327379)):
    return [np.full((h, w), c * 0.5 + 0.5, F) for c in n]


@pytest.mark.parametrize("power", POWERS)
@pytest.mark.parametrize("quantised", [False, True])
def test_a_flat_map_gives_the_plain_chain(power, quantised):
    """Also where every texel has another direction's rounding: smooth normals through 8 bits.  Unclamped: rho leaves [0, 1]."""
    w, h = 130, 70
    rho = synthetic_rgba(SEED_A, h, w)[0] * F(1.5) - F(0.25)
    for X, Y, Z in (flat_normals(w, h), flat_normals(w, h, (0.0, 0.0, 1.0))):
        if quantised:
            X, Y, Z = [np.round(p * F(255.0)).astype(F) / F(255.0) for p in (X, Y, Z)]
        got, plain = ref.chain(rho, X, Y, Z, power), mip_ref.chain(rho)
        assert len(got) == mip_ref.level_count(w, h)
        for k, (g, p) in enumerate(zip(got, plain)):
            assert bit_equal(g, p), k


def test_the_floor_swallows_the_rounding_of_unit_vectors():
    """t of a single unit vector, exact or through 8 bits, stays far below 2^-14."""
    rng = np.random.default_rng(SEED_A + 3)
    n = unit_vectors(rng, 1 << 16)
    for enc in ((n * 0.5 + 0.5).astype(F), np.round((n * 0.5 + 0.5) * 255.0).astype(F) / F(255.0)):
        u = ref.unit(enc[:, 0], enc[:, 1], enc[:, 2])
        l = np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
        t = (F(1.0) - l) / l
        assert t.dtype == F and float(np.abs(t).max()) <= 2.0 ** -20


def test_cancelling_halves_give_exactly_one():
    w, h = 64, 32
    X = np.tile(np.array([1.0, 0.0], F), (h, w // 2))  # +x and -x side by side
    Y, Z = np.full((h, w), 0.5, F), np.full((h, w), 0.5, F)
    rho = synthetic_rgba(SEED_A, h, w)[1]
    for power in POWERS:
        got = ref.chain(rho, X, Y, Z, power)
        for k in range(1, len(got)):
            assert bit_equal(got[k], np.ones(got[k].shape, F)), (power, k)


def test_more_spread_never_gives_less_roughness():
    """For one r and power, d does not fall as the averaged vector gets shorter -- up to the ulp or two by which d may lie below
    clamp01(r) near 1 (four roundings of relative 2^-24 each, halved twice by the roots: under 4 ulps)."""
    l = np.concatenate([np.linspace(1.0, 0.0, 4097), 1.0 - np.logspace(-7, -1, 512)]).astype(F)
    l = np.sort(np.unique(l))[::-1]  # from flat to cancelling
    zero = np.zeros(len(l), F)
    for power in POWERS:
        for r in (0.0, 0.01, 0.2, 0.5, 0.8, 0.999, 1.0):
            d = ref.texel(zero, zero, l, np.full(len(l), r, F), power).astype(np.float64)
            assert d[0] == F(r) and d[-1] == 1.0
            assert (np.diff(d) >= -4 * 2.0 ** -24).all(), (power, r, float(np.diff(d).min()))
            assert (d >= float(F(r)) - 4 * 2.0 ** -24).all(), (power, r)


@pytest.mark.parametrize("power", POWERS)
def test_results_lie_in_the_unit_interval(power):
    rng = np.random.default_rng(SEED_A + 4)
    n = 1 << 16
    m = (unit_vectors(rng, n) * rng.random((n, 1))).astype(F)
    r = rng.random(n, dtype=F)
    r[:8] = [0.0, 1.0, 1e-45, 1e-20, 0.5, 0.999999, 1e-3, 0.25]
    d = ref.texel(m[:, 0], m[:, 1], m[:, 2], r, power)
    assert np.isfinite(d).all() and (d >= 0.0).all() and (d <= 1.0).all()
    chain = ref.chain(synthetic_rgba(SEED_A, 70, 130)[0], *synthetic_rgba(SEED_A + 9, 70, 130)[:3], power)
    for k, lv in enumerate(chain):
        assert lv.shape == mip_ref.level_size(130, 70, k)[::-1]
        assert np.isfinite(lv).all() and (lv >= 0.0).all() and (lv <= 1.0).all(), k
    assert float(chain[3].mean()) > float(mip_ref.chain(chain[0])[3].mean()) + 0.05 * min(1.0, power)  # random normals: rougher
