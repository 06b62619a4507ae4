"""The host half of KC_MIP_COVERAGE (include/kanter_core_amd.h), on a machine without a GPU: r_B is the smallest f32 that
quantises to at least B, kc_mip_coverage_target equals Python's integers, kc_mip_coverage_scale equals tests/mip_coverage_ref.py
bit for bit, and the flag is refused where and in the order the contract says."""
import ctypes as C

import numpy as np
import pytest

import mip_coverage_ref as R
import mip_ref

KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED, KC_ERR_NO_DEVICE = 102, 104, 101
BC_SRGB, MIP_PER_LEVEL, MIP_NORMALS, MIP_COVERAGE, BC7 = 1, 2, 32, 64, 98
F = np.float32
REFS = [1, 85, 128, 255]


def cov(b):
    return MIP_COVERAGE | b << 24


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    return kc


@pytest.fixture(scope="module")
def L():
    from kanter_core_amd import _lib
    return _lib.load()


def test_the_python_flag_word(kc):
    assert kc.MIP_COVERAGE == MIP_COVERAGE and kc.mip_coverage_ref(128) == cov(128)
    for bad in (0, 256, -1):
        with pytest.raises(ValueError):
            kc.mip_coverage_ref(bad)


def test_the_threshold_is_the_smallest_float_that_quantises_to_the_byte(kc):
    for b in range(1, 256):
        r = kc.alpha_ref_threshold(b)
        assert r.dtype == F and r.view(np.uint32) == R.threshold(b).view(np.uint32), b
        below = np.nextafter(r, F(0.0))
        assert R.quant_u8(r) >= b and R.quant_u8(below) < b, (b, r)
        assert R.quant_u8(r) == b
    # covered two ways: the byte against B, the clamped value against r_B
    a = np.concatenate([np.linspace(-0.5, 1.5, 4001, dtype=F), np.array([np.nan, np.inf, -np.inf, -0.0, 1e-45], F)])
    for b in (1, 2, 85, 127, 128, 254, 255):
        assert np.array_equal(R.quant_u8(a) >= b, R.key(a) >= R.threshold(b)), b


def test_threshold_and_scale_refuse_bad_arguments(L):
    r = C.c_float(7.0)
    for bad in (0, 256, 1 << 24):
        assert L.kc_alpha_ref_threshold(bad, C.byref(r)) == KC_ERR_INVALID_ARG
        assert L.kc_mip_coverage_scale(0.5, bad, C.byref(r)) == KC_ERR_INVALID_ARG
    assert L.kc_alpha_ref_threshold(128, None) == KC_ERR_INVALID_ARG
    assert L.kc_mip_coverage_scale(0.5, 128, None) == KC_ERR_INVALID_ARG
    assert r.value == 7.0


@pytest.mark.parametrize("size", [(1, 1), (1, 5), (130, 70), (4096, 4096)], ids=lambda s: "%dx%d" % s)
def test_target_equals_python_integers(kc, L, size):
    w, h = size
    n0 = w * h
    rng = np.random.default_rng([3, w, h])
    c0s = sorted({0, 1, n0 // 2, n0 - 1, n0} | {int(x) for x in rng.integers(0, n0 + 1, size=40)})
    for c0 in (c for c in c0s if 0 <= c <= n0):
        for k in range(mip_ref.level_count(w, h)):
            lw, lh = mip_ref.level_size(w, h, k)
            want = c0 if k == 0 else R.target(n0, lw * lh, c0)
            assert kc.mip_coverage_target(w, h, c0, k) == want, (c0, k)
            if c0 == 0:
                assert want == 0
            if c0 == n0:
                assert want == lw * lh
            if c0 > 0:
                assert 1 <= want <= lw * lh
    t = C.c_uint64(77)
    assert L.kc_mip_coverage_target(w, h, n0 + 1, 0, C.byref(t)) == KC_ERR_INVALID_ARG
    assert L.kc_mip_coverage_target(w, h, 0, mip_ref.level_count(w, h), C.byref(t)) == KC_ERR_INVALID_ARG
    assert L.kc_mip_coverage_target(w, h, 0, 0, None) == KC_ERR_INVALID_ARG
    assert L.kc_mip_coverage_target(0, h, 0, 0, C.byref(t)) == KC_ERR_INVALID_ARG
    assert t.value == 77


def test_target_refuses_more_than_2_31_texels(L):
    t = C.c_uint64(77)
    assert L.kc_mip_coverage_target(1 << 16, (1 << 15) + 1, 0, 0, C.byref(t)) == KC_ERR_INVALID_ARG and t.value == 77
    assert L.kc_mip_coverage_target(1 << 16, 1 << 15, 1 << 31, 1, C.byref(t)) == 0 and t.value == 1 << 29


def scale_values():
    floor = F(2.0 ** -16)
    edge = [floor, np.nextafter(floor, F(0.0)), np.nextafter(floor, F(1.0)), F(2.0 ** -17), F(0.0), F(1e-45), F(1e-40), F(1.17549435e-38), F(1.0),
            np.nextafter(F(1.0), F(0.0)), F(0.5), F(1.0 / 255.0), F(254.5 / 255.0)]
    rng = np.random.default_rng(11)
    rand = rng.random(3000, dtype=F)
    small = (rng.random(1000, dtype=F) * F(2.0 ** -12)).astype(F)
    thresholds = np.array([R.threshold(b) for b in range(1, 256)], F)
    near = np.concatenate([thresholds, np.nextafter(thresholds, F(0.0)), np.nextafter(thresholds, F(2.0))])
    return np.concatenate([np.array(edge, F), rand, small, near]).astype(F)


@pytest.mark.parametrize("ref", REFS)
def test_scale_equals_the_reference(kc, ref):
    steps = 0
    for v in scale_values():
        got, want = kc.mip_coverage_scale(v, ref), R.scale(v, ref)
        assert got.view(np.uint32) == want.view(np.uint32), (v, ref, got, want)
        ve = max(v, F(2.0 ** -16))
        assert np.isfinite(got) and got > 0
        assert R.quant_u8(ve * got) >= ref  # what the bump loop is for
        steps = max(steps, int(got.view(np.uint32)) - int((R.threshold(ref) / ve).view(np.uint32)))
    print("B = %d: at most %d steps above r_B / ve" % (ref, steps))


def test_flag_errors_come_first_and_in_order(L, tmp_path):
    img = C.c_void_p(1 << 20)  # never looked at: every call below is refused before it would be
    buf = (C.c_uint8 * 64)()
    levels, count = (C.c_void_p * 16)(), C.c_uint32()
    from kanter_core_amd import _lib
    recs = (_lib.kc_mip_coverage_level * 16)()
    path = str(tmp_path / "x.dds").encode()
    bad_words = [MIP_COVERAGE, 128 << 24, 1 << 24, cov(128) | 4, cov(128) | 8, cov(128) | 16, MIP_COVERAGE | MIP_NORMALS]
    for flags in bad_words:
        # refused with the other flag errors: before the NULL arguments
        assert L.kc_image_build_mips(None, flags, None, 0, None) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_to_bc_mips(None, 3, flags, None, 0) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_to_bc_mips_device(None, 3, flags, None, 0, None) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_live_graph_buffer_bc_mips(None, 0, 0, 3, flags, None, 0, None) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_write_dds(None, None, 3, flags, 1) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_mip_coverage_info(None, flags, None, 0, None) == KC_ERR_UNSUPPORTED, flags
    assert L.kc_image_mip_coverage_info(None, 0, None, 0, None) == KC_ERR_UNSUPPORTED  # the query is about the flag
    assert L.kc_image_mip_coverage_info(None, MIP_PER_LEVEL, None, 0, None) == KC_ERR_UNSUPPORTED
    # sRGB where there is no colour stays refused with the flag; a vector is still not a colour
    assert L.kc_image_to_bc_mips(img, 5, cov(128) | BC_SRGB, buf, 64) == KC_ERR_UNSUPPORTED
    assert L.kc_image_to_bc_mips(img, 3, cov(128) | MIP_NORMALS | BC_SRGB, buf, 64) == KC_ERR_UNSUPPORTED
    assert L.kc_image_build_mips(img, cov(128) | BC_SRGB, levels, 16, C.byref(count)) == KC_ERR_UNSUPPORTED
    # a good word: then the NULL arguments
    for flags in (cov(1), cov(128), cov(255), cov(85) | MIP_PER_LEVEL, cov(85) | MIP_NORMALS):
        assert L.kc_image_build_mips(None, flags, levels, 16, C.byref(count)) == KC_ERR_INVALID_ARG, flags
        assert L.kc_image_to_bc_mips(img, 3, flags, None, 64) == KC_ERR_INVALID_ARG, flags
        assert L.kc_image_to_bc_mips_device(img, 3, flags, None, 64, None) == KC_ERR_INVALID_ARG, flags
        assert L.kc_live_graph_buffer_bc_mips(None, 0, 0, 3, flags, buf, 64, None) == KC_ERR_INVALID_ARG, flags
        assert L.kc_image_write_dds(img, None, 3, flags, 1) == KC_ERR_INVALID_ARG, flags
        assert L.kc_image_mip_coverage_info(img, flags, None, 16, C.byref(count)) == KC_ERR_INVALID_ARG, flags
    # then the device (this suite also runs where another test has initialised one: the fake image stays untouched there)
    if not L.kc_is_initialized():
        assert L.kc_image_to_bc_mips(img, 3, cov(128) | BC_SRGB, buf, 64) == KC_ERR_NO_DEVICE
        assert L.kc_image_to_bc_mips(img, BC7, cov(128) | BC_SRGB | MIP_PER_LEVEL, buf, 64) == KC_ERR_NO_DEVICE
        assert L.kc_image_build_mips(img, cov(128), levels, 16, C.byref(count)) == KC_ERR_NO_DEVICE
        assert L.kc_image_to_bc_mips_device(img, 3, cov(1), C.c_void_p(1 << 20), 64, None) == KC_ERR_NO_DEVICE
        assert L.kc_image_write_dds(img, path, 3, cov(255), 1) == KC_ERR_NO_DEVICE
        assert L.kc_image_write_dds(img, path, 3, cov(255), 0) == KC_ERR_NO_DEVICE
        assert L.kc_image_mip_coverage_info(img, cov(128), recs, 16, C.byref(count)) == KC_ERR_NO_DEVICE
    assert not (tmp_path / "x.dds").exists()


def test_the_header_refuses_the_flag(L):
    out = (C.c_uint8 * 148)()
    for fmt in (3, BC7):
        for flags in (cov(128), MIP_COVERAGE, 128 << 24, cov(128) | BC_SRGB):
            assert L.kc_dds_header(64, 64, fmt, flags, 7, out, None) == KC_ERR_UNSUPPORTED, (fmt, flags)
        assert L.kc_dds_header(64, 64, fmt, BC_SRGB, 7, out, None) == 0


# ------------------------------------------------------------------ the reference itself
def lines_mask(w, h):
    """One-texel lines: every 7th row and every 5th column"""
    a = np.zeros((h, w), F)
    a[::7, :] = 1.0
    a[:, ::5] = 1.0
    return a


def dots_mask(w, h, share=0.3):
    return (np.random.default_rng([17, w, h]).random((h, w)) < share).astype(F)


@pytest.mark.parametrize("mask", ["lines", "dots"])
def test_the_reference_keeps_the_coverage_the_plain_chain_loses(mask):
    w = h = 256
    a = lines_mask(w, h) if mask == "lines" else dots_mask(w, h)
    levels, info = R.chain(a, 128)
    plain = mip_ref.chain(a)
    c0 = R.covered(a, 128)
    assert R.covered(plain[2], 128) / plain[2].size < 0.5 * c0 / a.size
    for k in range(1, len(levels)):
        i = info[k]
        assert i.texels == levels[k].size and i.target == R.target(a.size, i.texels, c0)
        if i.scale == F(1.0):
            assert np.array_equal(levels[k].view(np.uint32), plain[k].view(np.uint32))
            continue
        ck = R.covered(levels[k], 128)
        upper = int((R.key(plain[k]).astype(np.float64) >= float(i.v) * (1.0 - 2.0 ** -20)).sum())
        assert i.target <= ck <= upper, (k, i, ck, upper)


@pytest.mark.parametrize("value", [0.0, 1.0])
def test_an_empty_or_opaque_plane_never_changes(value):
    a = np.full((70, 130), value, F)
    levels, info = R.chain(a, 128)
    for lv, p, i in zip(levels, mip_ref.chain(a), info):
        assert np.array_equal(lv.view(np.uint32), p.view(np.uint32)) and i.scale == F(1.0)
