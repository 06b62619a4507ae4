"""The host half of alpha-weighted mip chains (KC_MIP_ALPHA_WEIGHT, include/kanter_core_amd.h), on a machine without a GPU: the
reference tests/mip_alpha_ref.py has the properties the rule is there for (a constant alpha of 1 is the plain chain bit for bit; a
cutout's colour stays the cutout's colour at every texel of every level where the plain chain darkens; the top-down form of the
push equals the per-texel ancestor form on odd sizes; no positive alpha gives zeros), kc_mip_alpha_weight and kc_mip_alpha_texel
equal it bit for bit, and the entry points accept or refuse the flag as the contract says, in its order, as far as that is
reachable without a device."""
import ctypes as C
import itertools

import numpy as np
import pytest

import mip_alpha_ref as ref
import mip_ref
from test_gpu_mip_roughness import SPECIALS
from util import SEED_A, bit_equal, synthetic_rgba

KC_ERR_NO_DEVICE, KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 101, 102, 104
MIP_PER_LEVEL, MIP_NORMALS, MIP_COVERAGE, MIP_ALPHA_WEIGHT, BC_SRGB = 2, 32, 64, 128, 1
F = np.float32
ODD_SIZES = [(5, 3), (7, 7), (130, 70), (1, 5), (33, 17), (63, 65), (100, 3)]  # (w, h)


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    return kc


@pytest.fixture(scope="module")
def L():
    from kanter_core_amd import _lib
    return _lib.load()


def dot_mask(w, h):
    """Dots of radius 3 on a grid of 10: 32 of every 100 texels, the first dot around (2.5, 2.5)."""
    y, x = np.mgrid[0:h, 0:w]
    dx, dy = (x + 2) % 10 - 4.5, (y + 2) % 10 - 4.5
    return dx * dx + dy * dy < 9.0


def same_levels(got, want):
    return len(got) == len(want) and all(bit_equal(g, w) for g, w in zip(got, want))


# ------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("w,h", [(64, 64), (130, 70), (5, 3), (1, 5), (33, 17)])
def test_a_constant_alpha_of_one_gives_the_plain_chain(w, h):
    p = synthetic_rgba(SEED_A, h, w)
    p = [c * F(1.5) - F(0.25) for c in p[:3]]  # unclamped colours
    for alpha in (np.ones((h, w), F), np.full((h, w), 1.5, F), np.full((h, w), np.inf, F)):
        got = ref.chain(p[0], p[1], p[2], alpha)
        for c in range(3):
            assert same_levels(got[c], mip_ref.chain(p[c])), (c, float(alpha[0, 0]))


@pytest.mark.parametrize("w,h", [(64, 64), (130, 70), (5, 3), (320, 192)])
def test_a_dot_mask_keeps_its_colour_where_the_plain_chain_darkens(w, h):
    """Colour 0.8 on black under a dot mask of about 30 %.  Every texel of every level, the filled ones included, stays within
    2^-21 of 0.8: P and W of a texel are the same box of 0.8 a and of a, so q is 0.8 up to the rounding of 0.8 * a, of the
    boxes (exact here: sums of few equal values) and of the divide -- a few ulps of 0.8 = 2^-24 each, far inside 2^-21.  The
    reference measured 1.2e-7 at the most at these sizes."""
    mask = dot_mask(w, h)
    assert mask[:2, :4].any() and not mask.all() and (w < 64 or 0.28 < mask.mean() < 0.36)
    colour, alpha = np.where(mask, F(0.8), F(0.0)).astype(F), mask.astype(F)
    got = ref.chain(colour, colour, colour, alpha)
    worst = max(float(np.abs(lv.astype(np.float64) - 0.8).max()) for ch in got for lv in ch)
    print("worst distance from 0.8 at %dx%d: %.3g" % (w, h, worst))
    assert worst <= 2.0 ** -21
    if w >= 64:
        plain = mip_ref.chain(colour)
        assert float(plain[2].mean()) < 0.3 and float(got[0][2].mean()) > 0.79


@pytest.mark.parametrize("w,h", ODD_SIZES)
def test_the_top_down_form_equals_the_ancestor_form(w, h):
    rng = np.random.default_rng([SEED_A, w, h])
    p = synthetic_rgba(SEED_A + 1, h, w)
    lone = np.zeros((h, w), F)
    lone[h - 1, w - 1] = 1.0  # in a dropped column or row where the extent is odd
    alphas = [np.where(rng.random((h, w)) < 0.3, F(1.0), F(0.0)).astype(F),
              np.where(rng.random((h, w)) < 0.5, rng.random((h, w), dtype=F), F(0.0)).astype(F),
              np.where(rng.random((h, w)) < 0.02, F(0.25), F(0.0)).astype(F), lone, np.zeros((h, w), F)]
    for i, a in enumerate(alphas):
        top, anc = ref.chain(p[0], p[1], p[2], a), ref.chain_by_ancestors(p[0], p[1], p[2], a)
        for c in range(3):
            assert len(top[c]) == mip_ref.level_count(w, h)
            assert same_levels(top[c], anc[c]), (i, c)


def test_an_opaque_texel_in_a_dropped_column_and_row_has_no_known_ancestor():
    w, h = 130 + 1, 70 + 1
    p = synthetic_rgba(SEED_A + 2, h, w)
    a = np.zeros((h, w), F)
    a[h - 1, w - 1] = 1.0
    got = ref.chain(p[0], p[1], p[2], a)
    for c in range(3):
        assert got[c][0][h - 1, w - 1] == p[c][h - 1, w - 1]
        got[c][0][h - 1, w - 1] = 0.0
        assert not any(lv.any() for lv in got[c])


@pytest.mark.parametrize("w,h", [(64, 64), (130, 70), (1, 5), (1, 1)])
def test_no_positive_alpha_gives_zeros(w, h):
    p = synthetic_rgba(SEED_A + 3, h, w)
    p[0][0, 0], p[1][h - 1, 0] = np.nan, np.inf  # never enter
    for a in (np.zeros((h, w), F), np.full((h, w), -1.0, F), np.full((h, w), np.nan, F), np.full((h, w), -0.0, F)):
        for ch in ref.chain(p[0], p[1], p[2], a):
            assert all(bit_equal(lv, np.zeros(lv.shape, F)) for lv in ch)


def test_known_texels_lie_in_the_hull_of_the_known_colours_under_them():
    w, h = 130, 70
    rng = np.random.default_rng(SEED_A + 4)
    p = synthetic_rgba(SEED_A + 5, h, w)
    a = np.where(rng.random((h, w)) < 0.4, rng.random((h, w), dtype=F), F(0.0)).astype(F)
    q, known = ref.pull(p[0], p[1], p[2], a)
    lo, hi = float(p[0][known[0]].min()), float(p[0][known[0]].max())
    for k in range(1, len(known)):
        v = q[0][k][known[k]].astype(np.float64)
        assert (v >= lo - 2.0 ** -20).all() and (v <= hi + 2.0 ** -20).all(), k


# ------------------------------------------------------------------ the two functions against the reference
def test_the_weight_equals_the_reference(kc, L):
    values = np.concatenate([SPECIALS, np.array([1e-39, 0.25, 0.99999994, 1.0000001, 2.0, -1e-45], F),
                             np.random.default_rng(SEED_A).random(256, dtype=F) * F(1.5) - F(0.25)])
    got = np.array([kc.mip_alpha_weight(a) for a in values], F)
    assert bit_equal(got, ref.weight(values)) and not np.isnan(got).any()
    for a in (np.nan, -0.0, -1.0, -np.inf, 0.0):
        assert kc.mip_alpha_weight(a).view(np.uint32) == 0, a  # +0.0
    assert kc.mip_alpha_weight(np.inf) == 1.0 and kc.mip_alpha_weight(1e-45) == F(1e-45)
    w = C.c_float(7.0)
    assert L.kc_mip_alpha_weight(0.5, None) == KC_ERR_INVALID_ARG
    assert L.kc_mip_alpha_weight(0.5, C.byref(w)) == 0 and w.value == 0.5


def test_the_texel_equals_the_reference(kc, L):
    rows = list(itertools.product(SPECIALS, repeat=2))  # every special value as p and as w
    rng = np.random.default_rng(SEED_A + 6)
    rows += list(zip(rng.random(2048, dtype=F), rng.random(2048, dtype=F)))
    rows += list(zip(rng.random(256, dtype=F) * F(1e-38), rng.random(256, dtype=F) * F(1e-38)))  # denormal quotients
    for p, w in rows:
        p3 = np.array([p, F(0.5) * p, -p], F)
        want, known = ref.texel(p3, np.full(3, w, F))
        got, got_known = kc.mip_alpha_texel(p3, w)
        assert got.dtype == F and got_known == bool(known[0]) == bool(w > 0), (p, w)
        assert bit_equal(got, want), (p, w, got, want)
        if not got_known:
            assert not got.view(np.uint32).any(), (p, w)  # +0.0 in all three
    p3, q, known = np.array([0.1, 0.2, 0.3], F), np.full(3, 7.0, F), C.c_int(7)
    for args in ((None, 0.5, q.ctypes.data, C.byref(known)), (p3.ctypes.data, 0.5, None, C.byref(known)), (p3.ctypes.data, 0.5, q.ctypes.data, None)):
        assert L.kc_mip_alpha_texel(*args) == KC_ERR_INVALID_ARG
    assert (q == 7.0).all() and known.value == 7
    assert L.kc_mip_alpha_texel(p3.ctypes.data, 1.0, q.ctypes.data, C.byref(known)) == 0 and known.value == 1 and bit_equal(q, p3)
    with pytest.raises(ValueError):
        kc.mip_alpha_texel([0.5, 0.5], 1.0)


# ------------------------------------------------------------------ the flag, without a device
def test_the_flag_is_bit_128_and_the_python_keyword_sets_it(kc):
    from kanter_core_amd import api
    assert kc.MIP_ALPHA_WEIGHT == MIP_ALPHA_WEIGHT
    assert api._mip_flags(False, False, False) == 0 and api._mip_flags(True, True, False, 128) == BC_SRGB | MIP_PER_LEVEL | MIP_COVERAGE | 128 << 24
    assert api._mip_flags(False, False, False, alpha_weighted=True) == MIP_ALPHA_WEIGHT
    assert api._mip_flags(True, True, False, 1, True) == BC_SRGB | MIP_PER_LEVEL | MIP_COVERAGE | 1 << 24 | MIP_ALPHA_WEIGHT


def test_refusals_and_their_order_without_a_device(L):
    """With KC_MIP_NORMALS the flag is KC_ERR_UNSUPPORTED before any argument is looked at; alone, or with its legal companions,
    a call gets past the flag check: KC_ERR_INVALID_ARG for a NULL argument, KC_ERR_NO_DEVICE before kc_init."""
    no_device = not L.kc_is_initialized()  # with a device the calls that pass the argument checks would read the handles
    fake = C.c_void_p(0x1000)
    arr, count = (C.c_void_p * 16)(), C.c_uint32(77)
    host = (C.c_uint8 * 64)()
    A = MIP_ALPHA_WEIGHT
    legal = (A, A | MIP_PER_LEVEL, A | MIP_COVERAGE | 128 << 24)
    for flags in (A | MIP_NORMALS, A | MIP_NORMALS | MIP_PER_LEVEL, A | 4, A | 8, A | 1 << 24):
        assert L.kc_image_build_mips(fake, flags, arr, 16, C.byref(count)) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_build_mips(None, flags, None, 0, None) == KC_ERR_UNSUPPORTED, flags  # before the arguments
    for flags in legal:
        assert L.kc_image_build_mips(None, flags, arr, 16, C.byref(count)) == KC_ERR_INVALID_ARG, flags
        assert L.kc_image_build_mips(fake, flags, None, 16, C.byref(count)) == KC_ERR_INVALID_ARG, flags
        if no_device:
            assert L.kc_image_build_mips(fake, flags, arr, 16, C.byref(count)) == KC_ERR_NO_DEVICE, flags
    assert count.value == 77
    # the chain exporters: BC3 with sRGB is legal beside the flag
    for fmt, flags, want in ((3, A | MIP_NORMALS, KC_ERR_UNSUPPORTED), (98, A | MIP_NORMALS | MIP_PER_LEVEL, KC_ERR_UNSUPPORTED),
                             (3, A | 4, KC_ERR_UNSUPPORTED),
                             (3, A, KC_ERR_INVALID_ARG), (3, A | BC_SRGB, KC_ERR_INVALID_ARG), (98, A | MIP_COVERAGE | 9 << 24, KC_ERR_INVALID_ARG)):
        assert L.kc_image_to_bc_mips(None, fmt, flags, None, 0) == want, (fmt, flags)
        assert L.kc_image_to_bc_mips_device(None, fmt, flags, None, 0, None) == want, (fmt, flags)
        assert L.kc_image_write_dds(None, None, fmt, flags, 1) == want, (fmt, flags)
        assert L.kc_image_write_dds(None, None, fmt, flags, 0) == want, (fmt, flags)
        assert L.kc_live_graph_buffer_bc_mips(None, 0, 0, fmt, flags, None, 0, None) == want, (fmt, flags)
    assert L.kc_image_to_bc_mips(None, 4, A | BC_SRGB, None, 0) == KC_ERR_UNSUPPORTED  # sRGB is not for BC4, with the flag or without
    if no_device:
        assert L.kc_image_to_bc_mips(fake, 3, A, host, 64) == KC_ERR_NO_DEVICE
        assert L.kc_image_to_bc_mips_device(fake, 3, A, C.c_void_p(0x1000), 64, None) == KC_ERR_NO_DEVICE
        assert L.kc_image_write_dds(fake, b"/nonexistent/x.dds", 3, A, 1) == KC_ERR_NO_DEVICE
    assert not any(host)
    # those that keep refusing it
    out = (C.c_uint8 * 148)()
    assert L.kc_dds_header(64, 64, 3, A, 1, out, None) == KC_ERR_UNSUPPORTED and not any(out)
    assert L.kc_dds_header(64, 64, 3, 0, 1, out, None) == 0
    for flags in (A, A | MIP_PER_LEVEL):
        assert L.kc_image_build_roughness_mips(fake, 0, fake, C.c_float(1.0), flags, arr, 16, C.byref(count)) == KC_ERR_UNSUPPORTED
    assert L.kc_image_mip_coverage_info(fake, A | MIP_COVERAGE | 128 << 24, None, 0, None) == KC_ERR_UNSUPPORTED
    for flags in (A, A | 1):
        assert L.kc_image_previews(None, 0, flags, None, 0) == KC_ERR_UNSUPPORTED
        assert L.kc_image_previews_device(None, 0, flags, None, 0, None) == KC_ERR_UNSUPPORTED
        assert L.kc_live_graph_buffer_previews(None, None, None, None, 0, flags, None, 0) == KC_ERR_UNSUPPORTED
    assert count.value == 77
