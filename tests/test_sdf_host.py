"""The host half of signed distance fields (kc_image_distance_field, include/kanter_core_amd.h), on a machine without a GPU: the
reference tests/sdf_ref.py agrees with itself -- the windowed separable search equals the all-pairs definition after capping, on
random and structured masks, with and without wrap, also for spreads larger than either extent -- kc_sdf_texel equals its value
rule bit for bit for every squared distance up to the cap, kc_sdf_cap is S^2 + S + 1, and the entry points refuse as the header
says as far as that is reachable without a device."""
import ctypes as C

import numpy as np
import pytest

import sdf_ref as R

KC_ERR_NO_DEVICE, KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 101, 102, 104
F = np.float32
SPREADS = [1, 2, 7, 64, 254]


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    return kc


@pytest.fixture(scope="module")
def L():
    from kanter_core_amd import _lib
    return _lib.load()


def masks(w, h):
    rng = np.random.default_rng([31, w, h])
    out = {"d%g" % p: rng.random((h, w)) < p for p in (0.0, 0.05, 0.3, 0.5, 0.95, 1.0)}
    y, x = np.mgrid[0:h, 0:w]
    out["disc"] = (x - w / 2.0) ** 2 + (y - h / 3.0) ** 2 < (min(w, h) / 3.0) ** 2
    out["stripes"] = (x % 5 == 0) | (y % 7 == 3)
    lone = np.zeros((h, w), bool)
    lone[0, 0] = lone[-1, -1] = True
    out["corners"], out["hole"] = lone, ~lone
    return out


# ------------------------------------------------------------------ the reference against itself
@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("w,h", [(23, 17), (17, 23), (1, 9), (9, 1), (1, 1), (40, 6)])
def test_the_windowed_search_equals_the_definition_after_capping(w, h, wrap):
    for name, m in masks(w, h).items():
        full = R.d2_brute(m, wrap)
        for S in (1, 2, 3, 7, 30, 64):  # 30 and 64: larger than either extent
            win = R.d2_windowed(m, S, wrap)
            cap = R.cap(S)
            assert np.array_equal(np.minimum(win, cap), np.minimum(full, cap)), (name, S)
            assert np.array_equal(R.value(win, m, S).view(np.uint32), R.value(full, m, S).view(np.uint32)), (name, S)


def test_the_definition_on_masks_worked_by_hand():
    m = np.zeros((5, 7), bool)
    m[2, 3] = True
    d = R.d2_brute(m, False)
    assert d[2, 3] == 1 and d[0, 0] == 13 and d[4, 6] == 13 and d[2, 0] == 9
    assert R.d2_brute(m, True)[0, 0] == 13 and R.d2_brute(m, True)[2, 6] == 9 and R.d2_brute(m, False)[2, 6] == 9
    edge = np.zeros((4, 6), bool)
    edge[0, 0] = True
    assert R.d2_brute(edge, False)[3, 5] == 34 and R.d2_brute(edge, True)[3, 5] == 2  # torus: dx = 1, dy = 1
    assert (R.d2_brute(np.zeros((3, 3), bool), False) == R.NONE).all() and (R.d2_brute(np.ones((3, 3), bool), True) == R.NONE).all()
    v = R.value(R.d2_brute(np.zeros((3, 3), bool), False), np.zeros((3, 3), bool), 4)
    assert not v.view(np.uint32).any()  # +0.0 everywhere
    assert (R.value(R.d2_brute(np.ones((3, 3), bool), False), np.ones((3, 3), bool), 4) == 1.0).all()


def test_inside_is_the_covered_test(kc):
    for B in (1, 2, 127, 128, 254, 255):
        r = kc.alpha_ref_threshold(B)
        below = np.nextafter(r, F(-1))
        a = np.array([r, below, np.nextafter(r, F(2)), np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 2.0], F)
        assert list(R.inside(a, B)) == [True, False, True, True, True, False, False, False, True, True], B


# ------------------------------------------------------------------ the two functions against the reference
@pytest.mark.parametrize("S", SPREADS)
def test_the_texel_equals_the_value_rule_for_every_distance_up_to_the_cap(kc, S):
    cap = kc.sdf_cap(S)
    assert cap == S * S + S + 1 == R.cap(S)
    d2 = np.arange(0, cap + 1, dtype=np.int64)
    for inside in (False, True):
        got = np.array([kc.sdf_texel(int(d), inside, S) for d in d2], F)
        want = R.value(d2, np.full(d2.shape, inside), S)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (S, inside)
        body = got[1:cap].astype(np.float64)  # 1 <= d2 < cap: what a field holds before it saturates
        assert (np.diff(body) > 0).all() if inside else (np.diff(body) < 0).all()  # strictly monotone in d2
        assert (body > 0.0).all() and (body < 1.0).all()
        assert (body >= 0.5).all() if inside else (body < 0.5).all()
        near = F(0.5 + 0.25 / S) if inside else F(0.5 - 0.25 / S)  # d2 = 1: exact in f64, rounded once
        assert got[1].view(np.uint32) == near.view(np.uint32)
        sat = F(1.0) if inside else F(0.0)
        for d in (cap, cap + 1, 2 * cap, 0xffffffff):
            assert kc.sdf_texel(d, inside, S).view(np.uint32) == sat.view(np.uint32)


def test_the_arguments_of_the_two_functions(kc, L):
    cap, v = C.c_uint32(77), C.c_float(7.0)
    for S in (0, 255, 256, 0xffffffff):
        assert L.kc_sdf_cap(S, C.byref(cap)) == KC_ERR_INVALID_ARG and cap.value == 77
        assert L.kc_sdf_texel(1, 1, S, C.byref(v)) == KC_ERR_INVALID_ARG and v.value == 7.0
        with pytest.raises(kc.TexProError):
            kc.sdf_cap(S)
    assert L.kc_sdf_cap(8, None) == KC_ERR_INVALID_ARG and L.kc_sdf_texel(1, 1, 8, None) == KC_ERR_INVALID_ARG
    assert L.kc_sdf_cap(254, C.byref(cap)) == 0 and cap.value == 254 * 254 + 255
    assert L.kc_sdf_texel(1, 5, 8, C.byref(v)) == 0 and v.value == 0.5 + 0.25 / 8  # any non-zero `inside` is inside
    assert kc.SDF_WRAP == 1 and kc.SDF_MAX_SPREAD == 254


# ------------------------------------------------------------------ the entry point, without a device
def test_the_device_entry_point_refuses_without_a_device(kc, L):
    """KC_ERR_NO_DEVICE comes before every other check.  In a process that has bound a device (the whole suite on a GPU machine)
    the calls that name no image show the order of the other refusals instead; test_gpu_sdf has the rest."""
    fake, out = C.c_void_p(0x1000), C.c_void_p(0x77)
    if not L.kc_is_initialized():
        for args in ((fake, 0, 128, 8, 0), (fake, 0, 128, 8, 1), (None, 0, 128, 8, 0), (fake, 9, 0, 0, 6)):
            assert L.kc_image_distance_field(*args, C.byref(out)) == KC_ERR_NO_DEVICE, args
        assert L.kc_image_distance_field(fake, 0, 128, 8, 0, None) == KC_ERR_NO_DEVICE
        with pytest.raises(kc.TexProError) as e:
            kc.SlotImage(None).distance_field(channel=0)
        assert e.value.kind == "NoDevice"
    else:
        assert L.kc_image_distance_field(None, 0, 128, 8, 6, C.byref(out)) == KC_ERR_UNSUPPORTED
        assert L.kc_image_distance_field(None, 0, 128, 8, 0, C.byref(out)) == KC_ERR_INVALID_ARG
    assert out.value == 0x77
