"""Mip chains without a GPU: worked values of the reference (tests/mip_ref.py), level counts and sizes, and the entries that
are arithmetic -- kc_mip_level_count, kc_bc_mip_layout, kc_dds_header -- through ctypes before kc_init, with their refusals;
the pixel entries answer KC_ERR_NO_DEVICE after their argument checks."""
import ctypes as C
import struct

import numpy as np
import pytest

import mip_ref

KC_OK, KC_ERR_NO_DEVICE, KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 0, 101, 102, 104
BC_SRGB, MIP_PER_LEVEL = 1, 2
BLOCK_BYTES = {1: 8, 3: 16, 4: 8, 5: 16}
SIZES = [(1, 1), (1, 5), (5, 1), (64, 64), (130, 70), (4096, 64), (4096, 4096)]  # (w, h)


def f32(*v):
    return np.array(v, np.float32)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ the reference's worked values
def test_two_by_two():
    assert mip_ref.reduce(f32(1, 2, 3, 4).reshape(2, 2)).tolist() == [[2.5]]


def test_a_column_and_a_row_clamp_the_extent_that_is_one():
    a, c = np.float32(0.3), np.float32(0.9)
    want = ((a + a) + (c + c)) * np.float32(0.25)
    col = mip_ref.reduce(f32(0.3, 0.9, 7.0, 8.0).reshape(4, 1))  # 1 wide, 4 high: x1 clamps to x0
    assert col.shape == (2, 1) and bits(col[0, 0]) == bits(want)
    # in a row the pair is horizontal: (a + c) + (a + c)
    row = mip_ref.reduce(f32(0.3, 0.9, 7.0, 8.0).reshape(1, 4))
    assert row.shape == (1, 2) and bits(row[0, 0]) == bits(((a + c) + (a + c)) * np.float32(0.25))
    assert bits(mip_ref.reduce(f32(0.3, 0.3, 0.9, 0.9).reshape(1, 4))[0, 0]) == bits(((a + a) + (a + a)) * np.float32(0.25))


def test_odd_extents_ignore_the_last_column_and_row():
    img = np.arange(15, dtype=np.float32).reshape(3, 5)  # 5 wide, 3 high
    poisoned = img.copy()
    poisoned[2, :] = np.nan
    poisoned[:, 4] = np.inf
    levels, again = mip_ref.chain(img), mip_ref.chain(poisoned)
    assert [l.shape for l in levels] == [(3, 5), (1, 2), (1, 1)]
    assert levels[1].tolist() == [[(0 + 1 + 5 + 6) / 4, (2 + 3 + 7 + 8) / 4]]
    assert levels[2].tolist() == [[((3.0 + 5.0) + (3.0 + 5.0)) * 0.25]]
    for a, b in zip(levels[1:], again[1:]):
        assert np.array_equal(bits(a), bits(b))


def test_special_values():
    assert np.isnan(mip_ref.reduce(f32(np.inf, -np.inf, 0, 0).reshape(2, 2))[0, 0])
    assert bits(mip_ref.reduce(f32(-0.0, -0.0, -0.0, -0.0).reshape(2, 2)))[0, 0] == 0x80000000
    tiny = np.float32(1e-45)  # the smallest denormal: the sum 4 tiny is exact, a quarter of it is tiny again
    assert bits(tiny) == 1
    assert bits(mip_ref.reduce(np.full((2, 2), tiny, np.float32)))[0, 0] == 1
    # three of them: 3 tiny / 4 rounds to tiny, two: tiny / 2 is a tie and rounds to even, 0
    assert bits(mip_ref.reduce(f32(tiny, tiny, tiny, 0).reshape(2, 2)))[0, 0] == 1
    assert bits(mip_ref.reduce(f32(tiny, tiny, 0, 0).reshape(2, 2)))[0, 0] == 0
    assert bits(mip_ref.reduce(f32(tiny, 0, 0, 0).reshape(2, 2)))[0, 0] == 0
    big = np.float32(3e38)
    assert np.isinf(mip_ref.reduce(np.full((2, 2), big, np.float32))[0, 0])  # a + b overflows although the mean would not


@pytest.mark.parametrize("w,h", SIZES)
def test_level_counts_and_sizes(w, h):
    want = {(1, 1): 1, (1, 5): 3, (5, 1): 3, (64, 64): 7, (130, 70): 8, (4096, 64): 13, (4096, 4096): 13}[(w, h)]
    assert mip_ref.level_count(w, h) == want
    if w * h <= 130 * 70:
        shapes = [l.shape for l in mip_ref.chain(np.zeros((h, w), np.float32))]
        assert shapes == [mip_ref.level_size(w, h, k)[::-1] for k in range(want)]
        assert shapes[-1] == (1, 1)
    assert mip_ref.level_size(w, h, want - 1) == (1, 1)
    assert want == 1 or mip_ref.level_size(w, h, want - 2) != (1, 1)


# ------------------------------------------------------------------ the arithmetic entries, through ctypes
@pytest.fixture(scope="module")
def L():
    from kanter_core_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("w,h", SIZES)
def test_kc_mip_level_count(L, w, h):
    n = C.c_uint32()
    assert L.kc_mip_level_count(w, h, C.byref(n)) == KC_OK
    assert n.value == mip_ref.level_count(w, h)


def test_kc_mip_level_count_refusals(L):
    n = C.c_uint32()
    assert L.kc_mip_level_count(0, 4, C.byref(n)) == KC_ERR_INVALID_ARG
    assert L.kc_mip_level_count(4, 0, C.byref(n)) == KC_ERR_INVALID_ARG
    assert L.kc_mip_level_count(4, 4, None) == KC_ERR_INVALID_ARG


def layout(L, w, h, fmt, cap=None, want_offsets=True):
    n, total = C.c_uint32(), C.c_size_t()
    cap = mip_ref.level_count(w, h) if cap is None else cap
    offs = (C.c_size_t * max(cap, 1))()
    status = L.kc_bc_mip_layout(w, h, fmt, C.byref(n), offs if want_offsets else None, cap, C.byref(total))
    return status, n.value, list(offs)[:cap], total.value


@pytest.mark.parametrize("fmt", [1, 3, 4, 5])
@pytest.mark.parametrize("w,h", SIZES)
def test_kc_bc_mip_layout(L, w, h, fmt):
    status, n, offs, total = layout(L, w, h, fmt)
    assert status == KC_OK and n == mip_ref.level_count(w, h)
    sizes = [((max(1, w >> k) + 3) // 4) * ((max(1, h >> k) + 3) // 4) * BLOCK_BYTES[fmt] for k in range(n)]
    assert offs == [sum(sizes[:k]) for k in range(n)]
    assert total == sum(sizes)
    assert sizes[-1] == BLOCK_BYTES[fmt]  # the 1 x 1 level is one edge block
    # without an offsets array the cap does not matter
    assert layout(L, w, h, fmt, cap=0, want_offsets=False)[::3] == (KC_OK, total)


def test_kc_bc_mip_layout_refusals(L):
    assert layout(L, 0, 8, 1)[0] == KC_ERR_INVALID_ARG
    assert layout(L, 8, 0, 1)[0] == KC_ERR_INVALID_ARG
    for fmt in (0, 2, 6, 7):
        assert layout(L, 8, 8, fmt)[0] == KC_ERR_INVALID_ARG
    status, n, _, _ = layout(L, 130, 70, 3, cap=7)  # eight levels
    assert status == KC_ERR_INVALID_ARG and n == 8


def header(L, w, h, fmt, flags, levels):
    out, n = (C.c_uint8 * 148)(), C.c_size_t()
    status = L.kc_dds_header(w, h, fmt, flags, levels, out, C.byref(n))
    return status, bytes(out), n.value


@pytest.mark.parametrize("w,h,fmt,flags,levels,dxgi", [
    (130, 70, 3, 0, 8, 77), (130, 70, 3, BC_SRGB, 8, 78), (64, 64, 1, 0, 7, 71), (64, 64, 1, BC_SRGB, 1, 72), (5, 3, 4, 0, 2, 80),
    (4096, 64, 5, 0, 13, 83), (1, 1, 1, 0, 1, 71)])
def test_kc_dds_header(L, w, h, fmt, flags, levels, dxgi):
    status, got, n = header(L, w, h, fmt, flags, levels)
    assert status == KC_OK and n == 148
    mips = levels > 1
    linear = ((w + 3) // 4) * ((h + 3) // 4) * BLOCK_BYTES[fmt]
    want = b"DDS " + struct.pack("<7I", 124, 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000 | (0x20000 if mips else 0), h, w, linear, 0, levels)
    want += struct.pack("<11I", *[0] * 11)
    want += struct.pack("<2I4s5I", 32, 0x4, b"DX10", 0, 0, 0, 0, 0)
    want += struct.pack("<5I", 0x1000 | ((0x8 | 0x400000) if mips else 0), 0, 0, 0, 0)
    want += struct.pack("<5I", dxgi, 3, 0, 1, 0)
    assert len(want) == 148
    assert got == want
    from kanter_core_amd import api
    assert api.dds_header(w, h, fmt, srgb=bool(flags), levels=levels) == want


def test_kc_dds_header_refusals(L):
    assert header(L, 0, 8, 1, 0, 1)[0] == KC_ERR_INVALID_ARG
    assert header(L, 8, 0, 1, 0, 1)[0] == KC_ERR_INVALID_ARG
    assert header(L, 8, 8, 2, 0, 1)[0] == KC_ERR_INVALID_ARG
    assert header(L, 8, 8, 1, 0, 0)[0] == KC_ERR_INVALID_ARG
    assert header(L, 8, 8, 1, 0, 5)[0] == KC_ERR_INVALID_ARG  # 8 x 8 has four levels
    assert header(L, 8, 8, 1, 0, 4)[0] == KC_OK
    assert header(L, 8, 8, 4, BC_SRGB, 1)[0] == KC_ERR_UNSUPPORTED
    assert header(L, 8, 8, 5, BC_SRGB, 1)[0] == KC_ERR_UNSUPPORTED
    assert header(L, 8, 8, 1, 4, 1)[0] == KC_ERR_UNSUPPORTED
    assert header(L, 8, 8, 1, MIP_PER_LEVEL, 1)[0] == KC_ERR_UNSUPPORTED  # not a property of the file
    assert L.kc_dds_header(8, 8, 1, 0, 1, None, None) == KC_ERR_INVALID_ARG


def test_python_wrappers_of_the_arithmetic(L):
    from kanter_core_amd import api
    assert api.mip_level_count(130, 70) == 8
    offs, total = api.bc_mip_layout(130, 70, "bc3")
    assert (offs, total) == (layout(L, 130, 70, 3)[2], layout(L, 130, 70, 3)[3])
    assert len(api.dds_header(130, 70, 1)) == 148


# ------------------------------------------------------------------ the pixel entries: argument checks, then the device
def test_pixel_entries_check_arguments_then_the_device(L, tmp_path):
    img = C.c_void_p(1 << 20)  # never looked at: every call below is refused before it would be
    buf = (C.c_uint8 * 64)()
    levels, count = (C.c_void_p * 16)(), C.c_uint32()
    path = str(tmp_path / "x.dds").encode()
    # 1. unknown flag bits, sRGB where there is no colour
    assert L.kc_image_build_mips(img, 4, levels, 16, C.byref(count)) == KC_ERR_UNSUPPORTED
    assert L.kc_image_build_mips(img, BC_SRGB, levels, 16, C.byref(count)) == KC_ERR_UNSUPPORTED
    assert L.kc_image_to_bc_mips(img, 1, 8, buf, 64) == KC_ERR_UNSUPPORTED
    assert L.kc_image_to_bc_mips(img, 4, BC_SRGB, buf, 64) == KC_ERR_UNSUPPORTED
    assert L.kc_image_to_bc_mips_device(img, 5, BC_SRGB, buf, 64, None) == KC_ERR_UNSUPPORTED
    assert L.kc_image_to_bc_mips_device(img, 1, 16, buf, 64, None) == KC_ERR_UNSUPPORTED
    assert L.kc_image_write_dds(img, path, 4, BC_SRGB, 1) == KC_ERR_UNSUPPORTED
    assert L.kc_live_graph_buffer_bc_mips(None, 0, 0, 1, 4, buf, 64, None) == KC_ERR_UNSUPPORTED
    # 2. NULL arguments, zero sizes, unknown formats
    assert L.kc_image_build_mips(None, 0, levels, 16, C.byref(count)) == KC_ERR_INVALID_ARG
    assert L.kc_image_build_mips(img, 0, None, 16, C.byref(count)) == KC_ERR_INVALID_ARG
    assert L.kc_image_build_mips(img, 0, levels, 16, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_mips(None, 1, 0, buf, 64) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_mips(img, 1, 0, None, 64) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_mips(img, 2, 0, buf, 64) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_mips_device(None, 1, 0, buf, 64, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_mips_device(img, 1, 0, None, 64, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_mips_device(img, 0, 0, buf, 64, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_mips_device(img, 3, 0, C.c_void_p((1 << 20) + 8), 64, None) == KC_ERR_INVALID_ARG  # not a multiple of 16
    assert L.kc_image_write_dds(None, path, 1, 0, 1) == KC_ERR_INVALID_ARG
    assert L.kc_image_write_dds(img, None, 1, 0, 1) == KC_ERR_INVALID_ARG
    assert L.kc_image_write_dds(img, path, 6, 0, 1) == KC_ERR_INVALID_ARG
    assert L.kc_live_graph_buffer_bc_mips(None, 0, 0, 1, 0, buf, 64, None) == KC_ERR_INVALID_ARG
    # 3. then the device (this suite also runs where another test has initialised one: the fake image stays untouched there)
    if not L.kc_is_initialized():
        assert L.kc_image_build_mips(img, 0, levels, 16, C.byref(count)) == KC_ERR_NO_DEVICE
        assert L.kc_image_build_mips(img, MIP_PER_LEVEL, levels, 16, C.byref(count)) == KC_ERR_NO_DEVICE
        assert L.kc_image_to_bc_mips(img, 1, BC_SRGB | MIP_PER_LEVEL, buf, 64) == KC_ERR_NO_DEVICE
        assert L.kc_image_to_bc_mips_device(img, 3, BC_SRGB, C.c_void_p(1 << 20), 64, None) == KC_ERR_NO_DEVICE
        assert L.kc_image_write_dds(img, path, 5, 0, 0) == KC_ERR_NO_DEVICE
    assert not (tmp_path / "x.dds").exists()
