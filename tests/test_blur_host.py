"""The host half of the blur (kc_image_blur, include/kanter_core_amd.h), on a machine without a GPU: kc_blur_weights gives the
reference's radius and -- to the last bit of libm's exp -- its weights, kc_blur_texel equals the reference's texel rule bit for
bit, the reference itself stays within the running-error bound of an f64 convolution with the same weights, and the entry
points refuse as the header says as far as that is reachable without a device."""
import ctypes as C

import numpy as np
import pytest

import blur_ref as R
from util import EDGE_VALUES, bit_equal, ordered_bits, resize_source

KC_ERR_NO_DEVICE, KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 101, 102, 104
F = np.float32
SIGMAS = [0.01, 0.3, 1.0 / 3.0, 1.0, 1.5, 4.0, 21.3]  # R = 1, 1, 2 (the f32 third is above 1/3), 3, 5, 12, 64
REFUSED = [21.4, 0.0, np.nan, -1.0, np.inf]
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    return kc


@pytest.fixture(scope="module")
def L():
    from kanter_core_amd import _lib
    return _lib.load()


def fp(a):
    return a.ctypes.data_as(FP)


# ------------------------------------------------------------------ radius and weights
def test_the_radius(kc, L):
    assert [R.radius(s) for s in SIGMAS] == [1, 1, 2, 3, 5, 12, 64]
    for s in SIGMAS:
        assert len(kc.blur_weights(s)) == R.radius(s) + 1, s
    w, r = np.full(80, 7.0, F), C.c_uint32(77)
    for s in REFUSED:
        assert L.kc_blur_weights(C.c_float(s), fp(w), 80, C.byref(r)) == KC_ERR_INVALID_ARG, s
        assert r.value == 77 and (w == 7.0).all()
        with pytest.raises(kc.TexProError):
            kc.blur_weights(s)
    assert kc.BLUR_WRAP == 1 and kc.BLUR_MAX_RADIUS == 64 == R.MAX_RADIUS


@pytest.mark.parametrize("sigma", SIGMAS)
def test_the_weights(kc, sigma):
    got, want = kc.blur_weights(sigma), R.weights(sigma)
    assert got.dtype == F and got.shape == want.shape
    ulps = np.abs(ordered_bits(got) - ordered_bits(want))
    print(sigma, "largest distance to the numpy weights, ulp:", int(ulps.max()))
    assert ulps.max() <= 1  # exp may differ in its last f64 bit between libm and numpy: the only comparison that is not exact
    assert (np.diff(got) <= 0).all() and (got >= 0).all() and got[0] > 0
    total = float(got[0]) + 2.0 * float(got[1:].astype(np.float64).sum())
    print(sigma, "sum - 1:", total - 1.0)
    assert abs(total - 1.0) <= 2.0 ** -23  # each rounding moves the sum by at most 2^-24 w_k


def test_the_arguments_of_kc_blur_weights(L):
    w, r = np.full(80, 7.0, F), C.c_uint32(77)
    assert L.kc_blur_weights(C.c_float(1.0), None, 80, C.byref(r)) == KC_ERR_INVALID_ARG
    assert L.kc_blur_weights(C.c_float(1.0), fp(w), 80, None) == KC_ERR_INVALID_ARG
    assert L.kc_blur_weights(C.c_float(1.0), fp(w), 3, C.byref(r)) == KC_ERR_INVALID_ARG  # R = 3 needs four
    assert r.value == 77 and (w == 7.0).all()
    assert L.kc_blur_weights(C.c_float(1.0), fp(w), 4, C.byref(r)) == 0 and r.value == 3
    assert (w[:4] > 0).all() and (w[4:] == 7.0).all()
    assert L.kc_blur_weights(C.c_float(21.3), fp(w), 65, C.byref(r)) == 0 and r.value == 64


# ------------------------------------------------------------------ the texel
@pytest.mark.parametrize("sigma", SIGMAS)
def test_the_texel_equals_the_reference_bit_for_bit(kc, sigma):
    w = kc.blur_weights(sigma)
    n = 2 * len(w) - 1
    rng = np.random.default_rng([61, len(w)])
    taps = (rng.random((96, n), dtype=F) * F(1.5) - F(0.25))
    taps[32:64] *= F(1e30)
    salted = taps.copy()
    for i in range(len(salted)):  # every edge value meets others through the pair add, the multiply and the running sum
        at = rng.integers(0, n, size=1 + i % 5)
        salted[i, at] = EDGE_VALUES[rng.integers(0, len(EDGE_VALUES), size=len(at))]
    salted[0, 0], salted[0, -1] = np.inf, -np.inf  # the outermost pair: inf - inf
    salted[1, :] = F(3e38)  # every pair add overflows
    for name, t in (("random", taps), ("salted", salted)):
        got = np.array([kc.blur_texel(row, w) for row in t], F)
        assert bit_equal(got, R.texel(t, w)), (sigma, name)
        back = np.array([kc.blur_texel(row[::-1], w) for row in t], F)
        assert bit_equal(got, back) and np.array_equal(np.isnan(got), np.isnan(back)), (sigma, name)
    if w[-1] == 0:  # a weight that underflowed stays a tap: 0 * inf
        t = np.zeros(n, F)
        t[0] = np.inf
        assert np.isnan(kc.blur_texel(t, w))


def test_the_arguments_of_kc_blur_texel(kc, L):
    w = kc.blur_weights(1.0)
    t, v = np.ones(7, F), C.c_float(7.0)
    for args in ((None, fp(w), 3), (fp(t), None, 3), (fp(t), fp(w), 0), (fp(t), fp(w), 65), (fp(t), fp(w), 0xffffffff)):
        assert L.kc_blur_texel(*args, C.byref(v)) == KC_ERR_INVALID_ARG and v.value == 7.0, args[2]
    assert L.kc_blur_texel(fp(t), fp(w), 3, None) == KC_ERR_INVALID_ARG
    assert L.kc_blur_texel(fp(t), fp(w), 3, C.byref(v)) == 0
    assert F(v.value) == R.texel(t, w)
    with pytest.raises(ValueError):
        kc.blur_texel(np.ones(6, F), w)


# ------------------------------------------------------------------ the reference against an f64 convolution
@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("sigma", [0.3, 1.0, 1.5, 4.0, 21.3])
def test_the_reference_stays_within_the_running_error_of_an_f64_convolution(kc, sigma, wrap):
    """Per pass: a chain of R + 2 roundings of the running sum plus the pair add and the multiply of every term, each relative
    2^-24, so |f32 - f64| <= (R + 4) 2^-24 sum_k w_k (|t_-k| + |t_k|), against the f64 result of the pass's own f32 input."""
    w = kc.blur_weights(sigma)
    Rr = len(w) - 1
    for shape in ((37, 53), (1, 9), (9, 1), (70, 130)):
        plane = resize_source(71, 0, *shape)
        mid = R.blur_axis(plane, w, 1, wrap)
        out = R.blur_axis(mid, w, 0, wrap)
        assert bit_equal(out, R.blur(plane, w, w, wrap)) and bit_equal(mid, R.blur(plane, w, None, wrap))
        for name, src, got, axis in (("x", plane, mid, 1), ("y", mid, out, 0)):
            exact, mag = R.conv_axis_f64(src, w, axis, wrap)
            err = np.abs(got.astype(np.float64) - exact)
            bound = (Rr + 4) * 2.0 ** -24 * mag
            print(sigma, wrap, shape, name, "largest error / bound: %.3f" % float((err / bound).max()))
            assert (err <= bound).all(), (sigma, wrap, shape, name)


def test_the_reference_by_hand():
    w = np.array([0.5, 0.25], F)
    p = np.array([[1.0, 2.0, 4.0, 8.0]], F)
    assert np.array_equal(R.blur_axis(p, w, 1, False), np.array([[1.25, 2.25, 4.5, 7.0]], F))  # edges repeat
    assert np.array_equal(R.blur_axis(p, w, 1, True), np.array([[3.0, 2.25, 4.5, 5.25]], F))   # edges wrap
    assert np.array_equal(R.blur_axis(p, w, 0, False), p) and np.array_equal(R.blur_axis(p, w, 0, True), p)  # one row: all taps are it
    assert list(R.tap_index(3, -7, True)) == [2, 0, 1] and list(R.tap_index(3, 7, False)) == [2, 2, 2]  # more than one wrap


# ------------------------------------------------------------------ the entry point, without a device
def test_the_device_entry_point_refuses_without_a_device(kc, L):
    """KC_ERR_NO_DEVICE comes before every other check.  In a process that has bound a device (the whole suite on a GPU machine)
    the calls that name no image show the order of the other refusals instead; test_gpu_blur has the rest."""
    fake, out = C.c_void_p(0x1000), C.c_void_p(0x77)
    one, nan = C.c_float(1.0), C.c_float(np.nan)
    if not L.kc_is_initialized():
        for args in ((fake, one, one, 1, 0), (fake, one, one, 1, 1), (None, one, one, 1, 0), (fake, nan, nan, 0, 6)):
            assert L.kc_image_blur(*args, C.byref(out)) == KC_ERR_NO_DEVICE, args[3:]
        assert L.kc_image_blur(fake, one, one, 1, 0, None) == KC_ERR_NO_DEVICE
        with pytest.raises(kc.TexProError) as e:
            kc.SlotImage(None).blur(1.0, channels=[0])
        assert e.value.kind == "NoDevice"
    else:
        assert L.kc_image_blur(None, nan, nan, 0, 6, C.byref(out)) == KC_ERR_UNSUPPORTED
        assert L.kc_image_blur(None, one, one, 1, 0, C.byref(out)) == KC_ERR_INVALID_ARG
    assert out.value == 0x77
