"""Signed distance fields on the device (kc_image_distance_field, csrc/sdf.hip): the f32 words of distance_field() equal
tests/sdf_ref.py bit for bit -- the all-pairs definition at every shape but the largest, the windowed search there.

Shapes (w, h): single rows and columns, 3 x 3, one band and one segment exactly (64 x 64), one texel either side of the kernels'
units -- the columns kernel works in bands of 64 rows and segments of 256 columns, the rows kernel in segments of 256 columns and
groups of 4 rows: (257, 65) and (255, 63) -- odd sizes of several bands, and 1024 x 512 (32 and 512 workgroups: every XCD).
Spreads: 1, 2, 7, 64 (the band height: a halo as high as a band), one larger than the image (the halo wraps more than once), and
254 on (300, 40).  Masks: 30 % noise, blobs, a lone inside texel at each corner, a lone outside texel, empty, full, one-texel
stripes on the band, row-group and segment seams, fractional alpha one ulp either side of kc_alpha_ref_threshold(B), NaN and the
infinities.  B: 1, 128, 255.  Every mask and size with and without KC_SDF_WRAP.

Then the property the 0.5 test rests on, channel selection, the plane states (constant, aliased, a pending chain, a caller-owned
plane of loose pitch), the launch counters, the cache-policy instantiations, the refusals and the shipping recipe end to end.
A squared distance does not depend on the spread, so one all-pairs table per (shape, mask, wrap) serves every spread."""
import ctypes as C

import numpy as np
import pytest

import sdf_ref as R
from test_gpu_streaming_variants import counted, scrub_planes
from util import bit_equal, wrapped_image

pytestmark = pytest.mark.gpu

KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 102, 104
F = np.float32
BAND, SEG, ROWS = 64, 256, 4  # csrc/kc_internal.hpp: KC_SDF_BAND, KC_SDF_SEG, KC_SDF_ROWS
SMALL = [(1, 1), (1, 5), (5, 1), (3, 3), (64, 64), (65, 63), (130, 70), (SEG + 1, BAND + 1), (SEG - 1, BAND - 1)]  # (w, h)
BIG = (1024, 512)
BINARY = ["noise", "blobs", "corners", "hole", "empty", "full", "seams"]
COUNTERS = ["sdf_columns", "sdf_rows", "sdf_columns_nt", "sdf_rows_nt"]
TWO = {"sdf_columns": 1, "sdf_rows": 1}


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    return kc


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def L():
    from kanter_core_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ data
def binary_mask(kind, w, h):
    rng = np.random.default_rng([41, w, h, BINARY.index(kind)])
    y, x = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    if kind == "noise":
        m = rng.random((h, w)) < 0.3
    elif kind == "blobs":
        for _ in range(max(2, w * h // 1500)):
            cx, cy, r = rng.random() * w, rng.random() * h, 1.5 + rng.random() * min(w, h, 60) / 3.0
            m |= (x - cx) ** 2 + (y - cy) ** 2 < r * r
    elif kind == "corners":
        m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = True
    elif kind == "hole":
        m[:] = True
        m[h // 3, (2 * w) // 3] = False
    elif kind == "full":
        m[:] = True
    elif kind == "seams":  # the last row / column of a unit and the first of the next, alternately
        for e in range(BAND, h + 1, BAND):
            m[e - 1, 0::2] = True
            if e < h:
                m[e, 1::2] = True
        for e in range(ROWS, h, 9 * ROWS):
            m[e - 1, :] ^= True
        for e in range(SEG, w + 1, SEG):
            m[0::2, e - 1] = True
            if e < w:
                m[1::2, e] = True
    return m


def fractional_plane(w, h, B, kc):
    """Alpha around r_B: the threshold itself, one ulp below and above, and values a little further off, in noise order"""
    r = kc.alpha_ref_threshold(B)
    pool = np.array([r, np.nextafter(r, F(-1)), np.nextafter(r, F(2)), r * F(0.5), min(F(1.0), r * F(1.5)), F(0.0), F(1.0)], F)
    return pool[np.random.default_rng([43, w, h, B]).integers(0, len(pool), size=(h, w))]


def special_plane(w, h):
    pool = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 0.25, 0.75, 1e-45, 2.0, -1.0], F)
    p = pool[np.random.default_rng([47, w, h]).integers(0, len(pool), size=(h, w))]
    p.reshape(-1)[:len(pool)] = pool[:p.size]
    return p


_REF = {}


def cached(key, make):
    if key not in _REF:
        _REF[key] = make()
        _REF[key].setflags(write=False)
    return _REF[key]


def brute(key, mask, wrap):
    return cached(("d2", key, wrap), lambda: R.d2_brute(mask, wrap))


def spreads_for(w, h):
    return [1, 2, 7, BAND, min(max(w, h) + 3, 254)]


def field(kc, plane, B, S, wrap, channel=None):
    return kc.SlotImage.from_planes([plane]).distance_field(ref=B, spread=S, wrap=wrap, channel=channel)


def check(kc, plane, mask, d2, B, S, wrap, what):
    got = field(kc, plane, B, S, wrap)
    assert not got.is_rgba() and tuple(got.size()) == plane.shape[::-1], what
    g, want = got.planes()[0], R.value(d2, mask, S)
    bad = g.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), list(zip(*np.nonzero(bad)))[:4], g[bad][:4], want[bad][:4])
    assert np.array_equal(g >= F(0.5), mask), what  # the alpha test at 0.5 gives back the mask, exactly


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("kind", BINARY)
@pytest.mark.parametrize("w,h", SMALL)
def test_binary_masks_equal_the_definition(kc, w, h, kind):
    mask = binary_mask(kind, w, h)
    plane = mask.astype(F)
    assert np.array_equal(R.inside(plane, 128), mask)
    for wrap in (False, True):
        d2 = brute((w, h, kind), mask, wrap)
        for S in spreads_for(w, h):
            check(kc, plane, mask, d2, 128, S, wrap, (w, h, kind, S, wrap))


@pytest.mark.parametrize("B", [1, 128, 255])
@pytest.mark.parametrize("w,h", SMALL)
def test_fractional_and_special_alpha_classify_as_the_reference(kc, w, h, B):
    for name, plane in (("fractional", fractional_plane(w, h, B, kc)), ("special", special_plane(w, h)), ("noise01", binary_mask("noise", w, h).astype(F))):
        mask = R.inside(plane, B)
        for wrap in (False, True):
            d2 = brute((w, h, name, B), mask, wrap)
            for S in (2, 7):
                check(kc, plane, mask, d2, B, S, wrap, (w, h, name, B, S, wrap))


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("kind", ["noise", "blobs", "seams"])
def test_spread_254(kc, kind, wrap):
    w, h = 300, 40
    mask = binary_mask(kind, w, h)
    check(kc, mask.astype(F), mask, brute((w, h, kind), mask, wrap), 128, 254, wrap, (kind, wrap))


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("kind,S", [("blobs", 7), ("noise", 2), ("seams", 7)])
def test_many_workgroups_equal_the_windowed_search(kc, kind, S, wrap):
    w, h = BIG
    mask = binary_mask(kind, w, h)
    want = cached(("win", kind, S, wrap), lambda: R.distance_field(mask.astype(F), 128, S, wrap))
    (got, seen, launches) = counted(kc, COUNTERS, {}, lambda: field(kc, mask.astype(F), 128, S, wrap).planes()[0])
    assert bit_equal(got, want) and seen == TWO and launches == 2
    assert np.array_equal(got >= F(0.5), mask)


# ------------------------------------------------------------------ launches, policies, the source
@pytest.mark.parametrize("w,h", SMALL + [(300, 40)])
def test_two_launches_at_every_size_and_the_source_is_untouched(kc, w, h):
    plane = binary_mask("noise", w, h).astype(F)
    img = kc.SlotImage.from_planes([plane])
    b0 = kc.stats()["algorithmic_bytes"]
    (out, seen, launches) = counted(kc, COUNTERS, {}, lambda: img.distance_field(spread=3))
    assert seen == TWO and launches == 2
    assert kc.stats()["algorithmic_bytes"] - b0 == 12 * w * h
    assert bit_equal(img.planes()[0], plane)


@pytest.mark.parametrize("wrap", [False, True])
def test_the_nontemporal_instantiations(kc, wrap):
    w, h = 130, 70
    mask = binary_mask("blobs", w, h)
    want = R.value(brute((w, h, "blobs"), mask, wrap), mask, 7)
    scrub_planes(kc, w, h)
    call = lambda: field(kc, mask.astype(F), 128, 7, wrap).planes()[0]
    (got, seen, launches) = counted(kc, COUNTERS, {"cache_budget_mb": 0}, call)
    assert bit_equal(got, want) and seen == dict(TWO, sdf_columns_nt=1, sdf_rows_nt=1) and launches == 2


# ------------------------------------------------------------------ channels and plane states
def test_channel_selection(kc, L):
    w, h = 65, 63
    masks = [binary_mask(k, w, h) for k in ("noise", "blobs", "seams", "hole")]
    rgba = kc.SlotImage.from_planes([m.astype(F) for m in masks])
    for ch, m in enumerate(masks):
        want = R.value(brute((w, h, ("noise", "blobs", "seams", "hole")[ch]), m, False), m, 7)
        assert bit_equal(rgba.distance_field(spread=7, channel=ch).planes()[0], want), ch
        if ch == 3:
            assert bit_equal(rgba.distance_field(spread=7).planes()[0], want)  # the default is alpha
    gray = kc.SlotImage.from_planes([masks[1].astype(F)])
    want = R.value(brute((w, h, "blobs"), masks[1], False), masks[1], 7)
    assert bit_equal(gray.distance_field(spread=7).planes()[0], want) and bit_equal(gray.distance_field(spread=7, channel=0).planes()[0], want)
    # aliased planes: [p, p, p, ones]
    wide = gray.as_type(True)
    for ch in range(3):
        assert bit_equal(wide.distance_field(spread=7, channel=ch).planes()[0], want), ch
    (ones, seen, launches) = counted(kc, COUNTERS, {}, lambda: wide.distance_field(spread=7))
    assert seen == {} and launches == 0 and (ones.planes()[0] == 1.0).all()


@pytest.mark.parametrize("value,B,want", [(1.0, 128, 1.0), (0.0, 128, 0.0), (0.5, 128, 0.0), (0.5, 127, 1.0), (np.nan, 255, 1.0), (-np.inf, 1, 0.0)])
def test_a_constant_plane_launches_nothing(kc, L, value, B, want):
    img = kc.SlotImage.from_value((37, 21), value, False)
    b0 = kc.stats()["bytes_in_use"]
    (out, seen, launches) = counted(kc, COUNTERS, {}, lambda: img.distance_field(ref=B, spread=9, wrap=True))
    assert seen == {} and launches == 0 and kc.stats()["bytes_in_use"] == b0
    p, is_c, v = C.c_void_p(), C.c_int(), C.c_float()
    assert L.kc_image_plane(out._h, 0, C.byref(p)) == 0 and L.kc_plane_is_const(p, C.byref(is_c), C.byref(v)) == 0
    L.kc_plane_release(p)
    assert is_c.value == 1 and F(v.value).view(np.uint32) == F(want).view(np.uint32)
    assert tuple(out.size()) == (37, 21) and not out.is_rgba()


def test_a_pending_chain_runs_first(kc):
    w, h = 130, 70
    rng = np.random.default_rng(53)
    a, b = rng.random((h, w), dtype=F), rng.random((h, w), dtype=F) * F(1.5)
    lazy = kc.mix_process(kc.SlotImage.from_planes([a]), kc.SlotImage.from_planes([b]), kc.MixType.Multiply)
    (got, seen, launches) = counted(kc, COUNTERS, {}, lambda: lazy.distance_field(ref=128, spread=7))
    product = (a * b).astype(F)
    mask = R.inside(product, 128)
    assert seen == TWO and launches >= 3  # the chain's own launch, then the two
    assert bit_equal(got.planes()[0], R.value(R.d2_brute(mask, False), mask, 7))
    assert bit_equal(lazy.planes()[0], product)


@pytest.mark.parametrize("layout", ["pad48", "offset"])
@pytest.mark.parametrize("wrap", [False, True])
def test_a_caller_owned_plane_of_loose_pitch(kc, torch, layout, wrap):
    """The guard is NaN, which counts as inside: a read beside the pixels would change the field."""
    w, h = 130, 70
    mask = binary_mask("blobs", w, h)
    src = wrapped_image(kc, torch, [mask.astype(F)], layout, F(np.nan))
    (got, seen, launches) = counted(kc, COUNTERS, {}, lambda: src.image.distance_field(spread=BAND, wrap=wrap).planes()[0])
    assert seen == TWO and launches == 2
    assert bit_equal(got, R.value(brute((w, h, "blobs"), mask, wrap), mask, BAND))
    src.assert_untouched()


# ------------------------------------------------------------------ refusals
def test_refusals_launch_and_allocate_nothing(kc, L):
    gray = kc.SlotImage.from_planes([binary_mask("noise", 9, 7).astype(F)])
    rgba = gray.as_type(True)
    huge = kc.SlotImage.from_value((65536, 32769), 1.0, False)  # 2^31 + 65536 texels, no memory behind them
    kc.sync()
    before = kc.stats()
    out = C.c_void_p(0x77)
    cases = [((gray._h, 0, 128, 8, 2), KC_ERR_UNSUPPORTED), ((gray._h, 0, 128, 8, 0x80000001), KC_ERR_UNSUPPORTED),
             ((gray._h, 9, 0, 0, 4), KC_ERR_UNSUPPORTED),  # the flags come before the arguments
             ((None, 0, 128, 8, 0), KC_ERR_INVALID_ARG),
             ((gray._h, 0, 0, 8, 0), KC_ERR_INVALID_ARG), ((gray._h, 0, 256, 8, 1), KC_ERR_INVALID_ARG),
             ((gray._h, 0, 128, 0, 0), KC_ERR_INVALID_ARG), ((gray._h, 0, 128, 255, 1), KC_ERR_INVALID_ARG),
             ((gray._h, 1, 128, 8, 0), KC_ERR_INVALID_ARG), ((rgba._h, 4, 128, 8, 0), KC_ERR_INVALID_ARG),
             ((huge._h, 0, 128, 8, 0), KC_ERR_INVALID_ARG)]
    for args, want in cases:
        assert L.kc_image_distance_field(*args, C.byref(out)) == want, args[1:]
        assert out.value == 0x77
    assert L.kc_image_distance_field(gray._h, 0, 128, 8, 0, None) == KC_ERR_INVALID_ARG
    after = kc.stats()
    assert after["kernel_launches"] == before["kernel_launches"] and after["bytes_in_use"] == before["bytes_in_use"]
    with pytest.raises(kc.TexProError) as e:
        gray.distance_field(spread=255)
    assert e.value.kind == "InvalidArgument"
    assert gray.distance_field(spread=254, ref=255).size() == gray.size()  # the ends of both ranges are legal


# ------------------------------------------------------------------ the recipe
def test_field_resize_bc4_dds_round_trip(kc, tmp_path):
    w = h = 64
    mask = binary_mask("blobs", w, h)
    sdf = kc.SlotImage.from_planes([mask.astype(F)]).distance_field(spread=16)
    small = kc.resize_image(sdf, (16, 16), kc.ResizeFilter.Triangle)
    path = tmp_path / "sdf.dds"
    small.write_dds(path, "bc4", mips=False)
    back, info = kc.SlotImage.read_dds(path, gray=True, return_info=True)
    assert tuple(back.size()) == (16, 16) and not back.is_rgba()
    assert (info.width, info.height) == (16, 16)
    # the file holds exactly the blocks to_bc writes for the resized field
    assert bit_equal(back.planes()[0], kc.SlotImage.from_bc(small.to_bc(4), 16, 16, 4, gray=True).planes()[0])
