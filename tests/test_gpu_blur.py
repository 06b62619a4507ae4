"""The blur on the device (kc_image_blur, csrc/blur.hip): the f32 words of SlotImage.blur() equal tests/blur_ref.py -- run with
the library's own weights -- bit for bit (any NaN equals any NaN).

Shapes (w, h): single texels, rows and columns, 3 x 3, one unit of both kernels exactly -- the rows kernel works in segments of
256 columns and groups of 4 rows, the columns kernel in tiles of 64 columns and bands of 64 rows: (256, 64) -- one texel either
side of it on both axes, (2 SEG + 3, 2 BAND + 5), and 1024 x 512 (512 and 128 workgroups: every XCD).  Sigmas: 0.3 (R 1), 1.0
(R 3), 1.5 (R 5, no multiple of four), 21.3 (R 64: halos larger than the small shapes, several wraps) and the pair (4.0, 0.3).
Every shape and sigma clamped and with wrap; values in [-0.25, 1.25), and once per shape and sigma salted on the unit seams
with NaN, the infinities, 3e38 neighbours whose pair add overflows (on both axes), subnormals and -0.0.

Then the properties the rule promises (mirror symmetry, translation under wrap, one axis alone, no axis at all), channel masks
and plane states (aliased, constant, a pending chain, caller-owned planes of loose pitch), the launch counters and algorithmic
bytes, the cache-policy instantiations, the refusals, and one recipe end to end."""
import ctypes as C

import numpy as np
import pytest

import blur_ref as R
from test_gpu_streaming_variants import counted, scrub_planes
from util import bit_equal, edge_lines, resize_source, salt, wrapped_image

pytestmark = pytest.mark.gpu

KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 102, 104
F = np.float32
SEG, ROWS, COLS, BAND = 256, 4, 64, 64  # csrc/kc_internal.hpp: KC_BLUR_SEG, KC_BLUR_ROWS, KC_BLUR_COLS, KC_BLUR_BAND
SMALL = [(1, 1), (1, 5), (5, 1), (3, 3), (SEG, BAND), (SEG + 1, BAND + 1), (SEG - 1, BAND - 1), (2 * SEG + 3, 2 * BAND + 5)]  # (w, h)
BIG = (1024, 512)
SIGMAS = [(0.3, 0.3), (1.0, 1.0), (1.5, 1.5), (21.3, 21.3), (4.0, 0.3)]  # (x, y)
COUNTERS = ["blur_rows", "blur_columns", "blur_rows_nt", "blur_columns_nt"]
TWO = {"blur_rows": 1, "blur_columns": 1}


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


# ------------------------------------------------------------------ data and references
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
        if isinstance(_CACHE[key], np.ndarray):
            _CACHE[key].setflags(write=False)
    return _CACHE[key]


def weights(kc, sigma):
    """the library's weights of a sigma; None for 0"""
    return None if sigma == 0 else cached(("w", sigma), lambda: kc.blur_weights(sigma))


def plain(w, h, channel=0):
    return cached(("plain", w, h, channel), lambda: resize_source(83, channel, h, w))


def salted(w, h):
    def make():
        p = resize_source(89, 0, h, w)
        rows, cols = edge_lines(h, [ROWS, BAND], 2), edge_lines(w, [4, COLS, SEG], 2)
        salt(p, rows, cols)           # 3e38 pairs one above the other
        salt(p.T, cols, rows, 3)      # and side by side
        return p
    return cached(("salted", w, h), make)


def want(kc, key, plane, sx, sy, wrap):
    return cached(("ref", key, plane.shape, sx, sy, wrap), lambda: R.blur(plane, weights(kc, sx), weights(kc, sy), wrap))


def handles(L, img):
    """the plane handles of an image's channels, as integers (no reference is kept)"""
    out = []
    for c in range(4 if img.is_rgba() else 1):
        p = C.c_void_p()
        assert L.kc_image_plane(img._h, c, C.byref(p)) == 0
        L.kc_plane_release(p)
        out.append(p.value)
    return out


def const_of(L, img, c):
    """(is constant, its value) of channel c"""
    p, is_c, v = C.c_void_p(), C.c_int(), C.c_float()
    assert L.kc_image_plane(img._h, c, C.byref(p)) == 0 and L.kc_plane_is_const(p, C.byref(is_c), C.byref(v)) == 0
    L.kc_plane_release(p)
    return is_c.value == 1, F(v.value)


def mismatch(got, ref):
    bad = ~((got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref)))
    return int(bad.sum()), [tuple(int(i) for i in yx) for yx in zip(*np.nonzero(bad))][:4], got[bad][:4], ref[bad][:4]


def check_gray(kc, key, plane, sx, sy, wrap, launches_want=2):
    img = kc.SlotImage.from_planes([plane])
    (got, seen, launches) = counted(kc, COUNTERS, {}, lambda: img.blur(sx, sy, wrap=wrap))
    what = (key, plane.shape[::-1], sx, sy, wrap)
    assert not got.is_rgba() and tuple(got.size()) == plane.shape[::-1], what
    g, ref = got.planes()[0], want(kc, key, plane, sx, sy, wrap)
    assert bit_equal(g, ref), (what,) + mismatch(g, ref)
    assert launches == launches_want and sum(seen.values()) == launches_want, (what, seen, launches)
    return g


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("w,h", SMALL + [BIG])
def test_every_shape_and_sigma_equals_the_reference(kc, w, h):
    scrub_planes(kc, w, h)
    for sx, sy in SIGMAS:
        for wrap in (False, True):
            check_gray(kc, "plain", plain(w, h), sx, sy, wrap)
            if (w, h) != BIG or sx == 1.5:
                check_gray(kc, "salted", salted(w, h), sx, sy, wrap)


@pytest.mark.parametrize("w,h", SMALL)
def test_mirror_symmetry_and_translation_under_wrap(kc, w, h):
    blur = lambda p, sx, sy, wrap: kc.SlotImage.from_planes([np.ascontiguousarray(p)]).blur(sx, sy, wrap=wrap).planes()[0]
    for name, p in (("plain", plain(w, h)), ("salted", salted(w, h))):
        for sx, sy in ((1.5, 1.5), (4.0, 0.3), (21.3, 21.3)):
            for wrap in (False, True):
                base = blur(p, sx, sy, wrap)
                assert bit_equal(blur(p[:, ::-1], sx, sy, wrap), base[:, ::-1]), (name, sx, sy, wrap, "x")
                assert bit_equal(blur(p[::-1, :], sx, sy, wrap), base[::-1, :]), (name, sx, sy, wrap, "y")
            dy, dx = 1 + h // 3, 2 + (2 * w) // 3
            assert bit_equal(blur(np.roll(p, (dy, dx), (0, 1)), sx, sy, True), np.roll(base, (dy, dx), (0, 1))), (name, sx, sy)


@pytest.mark.parametrize("w,h", SMALL)
def test_one_axis_alone_is_one_launch_and_no_axis_is_the_source(kc, L, w, h):
    p = plain(w, h)
    for s in (1.5, 21.3):
        for wrap in (False, True):
            img = kc.SlotImage.from_planes([p])
            b0 = kc.stats()["algorithmic_bytes"]
            (gx, seen, launches) = counted(kc, COUNTERS, {}, lambda: img.blur(s, 0.0, wrap=wrap))
            assert seen == {"blur_rows": 1} and launches == 1 and kc.stats()["algorithmic_bytes"] - b0 == 8 * w * h
            assert bit_equal(gx.planes()[0], R.blur_axis(p, weights(kc, s), 1, wrap)), (s, wrap, "x")
            (gy, seen, launches) = counted(kc, COUNTERS, {}, lambda: img.blur(0.0, s, wrap=wrap))
            assert seen == {"blur_columns": 1} and launches == 1
            assert bit_equal(gy.planes()[0], R.blur_axis(p, weights(kc, s), 0, wrap)), (s, wrap, "y")
    img = kc.SlotImage.from_planes([p, p * F(0.5), p + F(1.0), p])
    (same, seen, launches) = counted(kc, COUNTERS, {}, lambda: img.blur(0.0, channels=[1, 3]))
    assert seen == {} and launches == 0 and handles(L, same) == handles(L, img) and same.is_rgba()


# ------------------------------------------------------------------ channels and plane states
@pytest.mark.parametrize("wrap", [False, True])
def test_channel_masks_return_the_other_planes_themselves(kc, L, wrap):
    w, h = SEG + 1, BAND + 1
    planes = [plain(w, h, c) for c in range(4)]
    img = kc.SlotImage.from_planes(planes)
    src = handles(L, img)
    assert len(set(src)) == 4
    refs = [want(kc, ("plain", c), planes[c], 1.5, 1.5, wrap) for c in range(4)]
    for chans in ([0], [3], [0, 1, 2], None):
        b0 = kc.stats()["algorithmic_bytes"]
        (got, seen, launches) = counted(kc, COUNTERS, {}, lambda: img.blur(1.5, wrap=wrap, channels=chans))
        sel = range(4) if chans is None else chans
        assert seen == TWO and launches == 2, (chans, seen, launches)
        assert kc.stats()["algorithmic_bytes"] - b0 == 16 * w * h * len(sel)
        out, pix = handles(L, got), got.planes()
        for c in range(4):
            if c in sel:
                assert out[c] not in src and bit_equal(pix[c], refs[c]), (chans, c)
            else:
                assert out[c] == src[c], (chans, c)
    assert [bit_equal(a, b) for a, b in zip(img.planes(), planes)] == [True] * 4  # the source is untouched


def test_aliased_planes_are_blurred_once(kc, L):
    w, h = 130, 70
    p = plain(w, h)
    wide = kc.SlotImage.from_planes([p]).as_type(True)  # [p, p, p, ones]
    src = handles(L, wide)
    assert src[0] == src[1] == src[2] != src[3]
    sx, sy = 4.0, 0.3
    b0 = kc.stats()["algorithmic_bytes"]
    (got, seen, launches) = counted(kc, COUNTERS, {}, lambda: wide.blur(sx, sy))
    assert seen == TWO and launches == 2 and kc.stats()["algorithmic_bytes"] - b0 == 16 * w * h  # one distinct resident plane
    out = handles(L, got)
    assert out[0] == out[1] == out[2] and out[0] not in src and out[3] not in src
    assert bit_equal(got.planes()[0], want(kc, "plain", p, sx, sy, False))
    is_c, v = const_of(L, got, 3)
    one = R.blur(np.ones((3, 3), F), weights(kc, sx), weights(kc, sy), False)[1, 1]  # the rule on 1.0: not necessarily 1.0
    assert is_c and v.view(np.uint32) == one.view(np.uint32)
    only = wide.blur(sx, sy, channels=[1])  # one of the three: the other two stay the source's
    assert handles(L, only)[0] == src[0] and handles(L, only)[2] == src[2] and handles(L, only)[3] == src[3]
    assert bit_equal(only.planes()[1], want(kc, "plain", p, sx, sy, False))


@pytest.mark.parametrize("sx,sy", [(1.5, 1.5), (21.3, 0.0), (0.0, 0.3), (4.0, 0.3)])
@pytest.mark.parametrize("value", [0.5, np.nan, -np.inf])
def test_a_constant_plane_launches_and_allocates_nothing(kc, L, value, sx, sy):
    img = kc.SlotImage.from_value((37, 21), value, False)
    b0 = kc.stats()["bytes_in_use"]
    (out, seen, launches) = counted(kc, COUNTERS, {}, lambda: img.blur(sx, sy, wrap=True))
    assert seen == {} and launches == 0 and kc.stats()["bytes_in_use"] == b0
    is_c, v = const_of(L, out, 0)
    ref = R.blur(np.full((3, 3), value, F), weights(kc, sx), weights(kc, sy), True)[1, 1]
    assert is_c and bit_equal(v, ref), (v, ref)
    assert tuple(out.size()) == (37, 21) and not out.is_rgba()


def test_a_pending_chain_runs_first(kc):
    w, h = 130, 70
    a, b = plain(w, h, 1), plain(w, h, 2)
    lazy = kc.mix_process(kc.SlotImage.from_planes([a]), kc.SlotImage.from_planes([b]), kc.MixType.Multiply)
    (got, seen, launches) = counted(kc, COUNTERS, {}, lambda: lazy.blur(1.0, wrap=True))
    product = (a * b).astype(F)
    assert seen == TWO and launches >= 3  # the chain's own launch, then the two
    assert bit_equal(got.planes()[0], R.blur(product, weights(kc, 1.0), weights(kc, 1.0), True))
    assert bit_equal(lazy.planes()[0], product)


@pytest.mark.parametrize("layout", ["pad48", "offset"])
@pytest.mark.parametrize("wrap", [False, True])
def test_caller_owned_planes_of_loose_pitch(kc, torch, layout, wrap):
    """The guard is NaN: a read beside the pixels would turn results NaN.  130 columns end in a quad of two texels."""
    w, h = 130, 70
    planes = [plain(w, h, c) for c in range(4)]
    src = wrapped_image(kc, torch, planes, layout, F(np.nan))
    for sx, sy, n in ((1.5, 1.5, 2), (21.3, 0.0, 1), (0.0, 21.3, 1)):
        (got, seen, launches) = counted(kc, COUNTERS, {}, lambda: src.image.blur(sx, sy, wrap=wrap).planes())
        assert launches == n and sum(seen.values()) == n, (sx, sy, seen)
        for c in range(4):
            assert bit_equal(got[c], want(kc, ("plain", c), planes[c], sx, sy, wrap)), (sx, sy, c)
    src.assert_untouched()


# ------------------------------------------------------------------ launches, bytes, policies
@pytest.mark.parametrize("w,h", SMALL + [BIG])
def test_two_launches_at_every_shape_for_gray_and_rgba(kc, w, h):
    planes = [plain(w, h, c) for c in range(4)]
    for img, n in ((kc.SlotImage.from_planes(planes[:1]), 1), (kc.SlotImage.from_planes(planes), 4)):
        b0 = kc.stats()["algorithmic_bytes"]
        (out, seen, launches) = counted(kc, COUNTERS, {}, lambda: img.blur(1.0))
        assert seen == TWO and launches == 2, (n, seen, launches)
        assert kc.stats()["algorithmic_bytes"] - b0 == 16 * w * h * n
        for c, g in enumerate(out.planes()):
            assert bit_equal(g, want(kc, ("plain", c) if c else "plain", planes[c], 1.0, 1.0, False)), (n, c)
        assert [bit_equal(a, b) for a, b in zip(img.planes(), planes)] == [True] * n


@pytest.mark.parametrize("wrap", [False, True])
def test_the_nontemporal_instantiations(kc, wrap):
    w, h = SEG + 1, BAND + 1
    p = salted(w, h)
    for sx, sy, seen_want in ((1.5, 1.5, dict(TWO, blur_rows_nt=1, blur_columns_nt=1)), (1.5, 0.0, {"blur_rows": 1, "blur_rows_nt": 1}),
                              (0.0, 21.3, {"blur_columns": 1, "blur_columns_nt": 1})):
        scrub_planes(kc, w, h)
        call = lambda: kc.SlotImage.from_planes([p]).blur(sx, sy, wrap=wrap).planes()[0]
        (got, seen, launches) = counted(kc, COUNTERS, {"cache_budget_mb": 0}, call)
        assert seen == seen_want and launches == len(seen_want) // 2, (sx, sy, seen)
        assert bit_equal(got, want(kc, "salted", p, sx, sy, wrap)), (sx, sy)


# ------------------------------------------------------------------ refusals
def test_refusals_launch_and_allocate_nothing(kc, L):
    gray = kc.SlotImage.from_planes([plain(9, 7)])
    rgba = gray.as_type(True)
    huge = kc.SlotImage.from_value((65536, 32769), 1.0, False)  # 2^31 + 65536 texels, no memory behind them
    kc.sync()
    before = kc.stats()
    out = C.c_void_p(0x77)
    f = C.c_float
    cases = [((gray._h, f(1.0), f(1.0), 1, 2), KC_ERR_UNSUPPORTED), ((gray._h, f(1.0), f(1.0), 1, 0x80000001), KC_ERR_UNSUPPORTED),
             ((None, f(np.nan), f(-1.0), 0, 4), KC_ERR_UNSUPPORTED),  # the flags come before the arguments
             ((None, f(1.0), f(1.0), 1, 0), KC_ERR_INVALID_ARG),
             ((gray._h, f(np.nan), f(1.0), 1, 0), KC_ERR_INVALID_ARG), ((gray._h, f(1.0), f(np.nan), 1, 1), KC_ERR_INVALID_ARG),
             ((gray._h, f(-1.0), f(1.0), 1, 0), KC_ERR_INVALID_ARG), ((gray._h, f(1.0), f(-0.5), 1, 0), KC_ERR_INVALID_ARG),
             ((gray._h, f(np.inf), f(1.0), 1, 0), KC_ERR_INVALID_ARG), ((gray._h, f(0.0), f(np.inf), 1, 1), KC_ERR_INVALID_ARG),
             ((gray._h, f(21.4), f(1.0), 1, 0), KC_ERR_INVALID_ARG), ((gray._h, f(0.0), f(1e30), 1, 0), KC_ERR_INVALID_ARG),
             ((gray._h, f(1.0), f(1.0), 0, 0), KC_ERR_INVALID_ARG), ((rgba._h, f(0.0), f(0.0), 0, 1), KC_ERR_INVALID_ARG),
             ((gray._h, f(1.0), f(1.0), 2, 0), KC_ERR_INVALID_ARG), ((gray._h, f(1.0), f(1.0), 3, 0), KC_ERR_INVALID_ARG),
             ((rgba._h, f(1.0), f(1.0), 16, 0), KC_ERR_INVALID_ARG), ((rgba._h, f(1.0), f(1.0), 0x80000001, 0), KC_ERR_INVALID_ARG),
             ((huge._h, f(1.0), f(1.0), 1, 0), KC_ERR_INVALID_ARG), ((huge._h, f(0.0), f(0.0), 1, 1), KC_ERR_INVALID_ARG)]
    for args, status in cases:
        assert L.kc_image_blur(*args, C.byref(out)) == status, [a.value if isinstance(a, f) else a for a in args[1:]]
        assert out.value == 0x77
    assert L.kc_image_blur(gray._h, f(1.0), f(1.0), 1, 0, None) == KC_ERR_INVALID_ARG
    after = kc.stats()
    assert after["kernel_launches"] == before["kernel_launches"] and after["bytes_in_use"] == before["bytes_in_use"]
    with pytest.raises(kc.TexProError) as e:
        gray.blur(21.4)
    assert e.value.kind == "InvalidArgument"
    with pytest.raises(kc.TexProError) as e:
        gray.blur(1.0, channels=[1])
    assert e.value.kind == "InvalidArgument"
    assert gray.blur(21.3, 0.01, channels=[0]).size() == gray.size()  # the ends of the range are legal


# ------------------------------------------------------------------ the recipe
def test_a_height_map_smoothed_before_height_to_normal(kc):
    from oracle import oracle as orc
    w, h = 130, 70
    levels = (np.floor(plain(w, h, 3).clip(0, 1) * F(255)) / F(255)).astype(F)  # an 8-bit height
    smooth = kc.SlotImage.from_planes([levels]).blur(1.5, wrap=True)
    got = kc.height_to_normal_process(smooth).planes()
    ref = orc.height_to_normal(R.blur(levels, weights(kc, 1.5), weights(kc, 1.5), True))
    for c in range(3):
        assert bit_equal(got[c], ref[c]), c
