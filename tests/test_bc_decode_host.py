"""Block decode without a device: the numpy reference of the decode contract (tests/bc_decode_ref.py) against the decoders the
encoder tests already hold and against Pillow's, the coverage of the random blocks every decode test uses, kc_dds_parse
through the library against the reference parser, and the argument checks of the decode and compare entries before kc_init."""
import ctypes as C
import io
import os
import struct

import numpy as np
import pytest

import bc7_ref
import bc_decode_ref as R
import bc_ref
from pngio import read_png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
BC7 = R.BC7
BC6H = 95  # KC_BC6H
KC_OK, KC_ERR_NO_DEVICE, KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = R.KC_OK, R.KC_ERR_NO_DEVICE, R.KC_ERR_INVALID_ARG, R.KC_ERR_UNSUPPORTED
N_RANDOM = 96  # BC7: four rounds of the 24-block cycle of random_blocks


@pytest.fixture(scope="module")
def L():
    from kanter_core_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ the reference against the decoders of the encoder tests
@pytest.mark.parametrize("name", ["heart_110.png", "clouds.png"])
def test_reference_decodes_the_encoders_output_like_the_existing_decoders(name):
    a = R.as_rgba8(read_png(os.path.join(INPUTS, name)))
    h, w = a.shape[:2]
    b1 = bc_ref.encode(a, 1)
    px, n = R.decode(b1, 1, h, w)
    assert n == 0 and np.array_equal(px[..., :3], bc_ref.unblock(bc_ref.decode_bc1(b1), h, w))
    assert (px[..., 3] == 255).all()  # the encoder never writes a three-colour block with index 3
    b3 = bc_ref.encode(a, 3)
    px = R.decode(b3, 3, h, w)[0]
    assert np.array_equal(px[..., :3], bc_ref.unblock(bc_ref.decode_bc1(b3[..., 8:]), h, w))
    assert np.array_equal(px[..., 3], bc_ref.unblock(bc_ref.decode_bc4(b3[..., :8])[..., None], h, w)[..., 0])
    b4 = bc_ref.encode(a, 4)
    px = R.decode(b4, 4, h, w)[0]
    assert np.array_equal(px[..., 0], bc_ref.unblock(bc_ref.decode_bc4(b4)[..., None], h, w)[..., 0])
    assert (px[..., 1:3] == 0).all() and (px[..., 3] == 255).all()
    b5 = bc_ref.encode(a, 5)
    px = R.decode(b5, 5, h, w)[0]
    assert np.array_equal(px[..., 1], bc_ref.unblock(bc_ref.decode_bc4(b5[..., 8:])[..., None], h, w)[..., 0])
    assert (px[..., 2] == 0).all() and (px[..., 3] == 255).all()
    b7 = bc7_ref.encode(a)
    px, n = R.decode(b7, BC7, h, w)
    assert n == 0 and np.array_equal(px, bc7_ref.decode(b7, h, w))
    rec = R.error_record(a, b7, BC7)
    assert sum(rec["bc7_mode_blocks"]) == b7.shape[0] * b7.shape[1] == rec["bc7_mode_blocks"][5] + rec["bc7_mode_blocks"][6]
    assert rec["pixels"] == h * w and rec["sse"][0] == int(((px[..., 0].astype(np.int64) - a[..., 0]) ** 2).sum())


def test_bc3_colour_is_four_colour_mode_whatever_the_order():
    blk = R.random_blocks(3, 64)
    c0 = blk[:, 8].astype(int) | (blk[:, 9].astype(int) << 8)
    c1 = blk[:, 10].astype(int) | (blk[:, 11].astype(int) << 8)
    assert (c0 > c1).any() and (c0 < c1).any() and (c0 == c1).any()
    swapped = blk.copy()
    swapped[:, 8:10], swapped[:, 10:12] = blk[:, 10:12], blk[:, 8:10]
    swapped[:, 12:] = blk[:, 12:] ^ 0x55  # endpoints change places: indices 0 <-> 1 and 2 <-> 3
    a, b = R.decode_blocks(blk, 3)[0], R.decode_blocks(swapped, 3)[0]
    assert np.array_equal(a, b)
    assert (a[..., 3] == bc_ref.decode_bc4(blk[:, :8])).all()


# ------------------------------------------------------------------ Pillow
def pillow_decode(blk, fmt, h, w):
    Image = pytest.importorskip("PIL.Image")
    from kanter_core_amd import api
    data = api.dds_header(w, h, fmt, levels=1) + np.ascontiguousarray(blk, np.uint8).tobytes()
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def as_image(blk):
    """n blocks as an image one block high"""
    return blk.reshape(1, len(blk), -1), 4, 4 * len(blk)


def test_bc7_reference_equals_pillow_on_forced_modes():
    pytest.importorskip("PIL")
    blk = R.random_blocks(BC7, 192, seed=3)
    blk = blk[np.isin(R.bc7_modes(blk), (4, 5, 6))]
    modes = R.bc7_modes(blk)
    assert min((modes == m).sum() for m in (4, 5, 6)) >= 32
    b, h, w = as_image(blk)
    im = pillow_decode(b, BC7, h, w)
    assert im.mode == "RGBA"
    want = np.asarray(im)
    got, n = R.decode(b, BC7, h, w)
    assert n == 0
    assert np.array_equal(got, want), np.argwhere((got != want).any(-1))[:4]


@pytest.mark.parametrize("fmt", [1, 4])
def test_bc1_and_bc4_reference_stay_within_one_of_pillow(fmt):
    """Pillow floors the thirds (and BC4's sevenths and fifths) where this project rounds them, so the bytes differ, never by
    more than 1: the bound is the condition, equality is not asserted."""
    pytest.importorskip("PIL")
    blk = R.random_blocks(fmt, 256, seed=4)
    b, h, w = as_image(blk)
    im = pillow_decode(b, fmt, h, w)
    want = np.asarray(im.convert("RGBA") if fmt == 1 else im).astype(np.int64)
    got = R.decode(b, fmt, h, w)[0].astype(np.int64)
    if fmt == 4:
        want = want.reshape(h, w, -1)[..., 0]
        got = got[..., 0]
    assert np.abs(got - want).max() <= 1


# ------------------------------------------------------------------ what the random blocks cover
def test_the_random_blocks_cover_every_branch():
    blk = R.random_blocks(BC7, N_RANDOM)
    bits = ((blk[:, :, None] >> np.arange(8)) & 1).reshape(len(blk), 128).astype(np.int64)
    mode = R.bc7_modes(blk)
    for m in (4, 5, 6):
        assert (mode == m).sum() >= 12
    for m in (0, 1, 2, 3, 7, 8):  # the undecoded modes and the reserved block
        assert (mode == m).sum() >= 1
    assert R.undecoded(mode).sum() == 5 * (N_RANDOM // 24)
    rot4, rot5 = R._get(bits, 5, 2)[:, 0][mode == 4], R._get(bits, 6, 2)[:, 0][mode == 5]
    assert set(rot4) == {0, 1, 2, 3} and set(rot5) == {0, 1, 2, 3}
    assert set(R._get(bits, 7, 1)[:, 0][mode == 4]) == {0, 1}
    # the smallest image of the GPU tests that holds a whole cycle still has every mode
    small = R.bc7_modes(R.random_image_blocks(BC7, 64, 64).reshape(-1, 16))
    assert set(small) == {0, 1, 2, 3, 4, 5, 6, 7, 8}
    b1 = R.random_blocks(1, N_RANDOM)
    c0 = b1[:, 0].astype(int) | (b1[:, 1].astype(int) << 8)
    c1 = b1[:, 2].astype(int) | (b1[:, 3].astype(int) << 8)
    idx = (b1[:, 4:, None] >> (2 * np.arange(4))) & 3
    has3 = (idx == 3).any((1, 2))
    assert (has3 & (c0 > c1)).any() and (has3 & (c0 < c1)).any() and (has3 & (c0 == c1)).any()
    assert (R.decode_blocks(b1, 1)[0][..., 3] == 0).any()
    b4 = R.random_blocks(4, N_RANDOM)
    word = np.zeros(len(b4), np.uint64)
    for k in range(6):
        word |= b4[:, 2 + k].astype(np.uint64) << np.uint64(8 * k)
    i4 = (word[:, None] >> (np.uint64(3) * np.arange(16, dtype=np.uint64))) & np.uint64(7)
    for order in (b4[:, 0] > b4[:, 1], b4[:, 0] < b4[:, 1], b4[:, 0] == b4[:, 1]):
        assert ((i4 == 6).any(1) & order).any() and ((i4 == 7).any(1) & order).any()
    for fmt, at in ((3, 0), (5, 0), (5, 8)):  # the BC4 halves of BC3 and BC5 likewise
        b = R.random_blocks(fmt, N_RANDOM)
        assert (b[:, at] > b[:, at + 1]).any() and (b[:, at] < b[:, at + 1]).any() and (b[:, at] == b[:, at + 1]).any()


def test_weight_tables_are_the_kernels_expressions():
    # bc_decode.hip computes the weights instead of looking them up
    assert [(64 * i + 1) // 3 for i in range(4)] == list(R.W2)
    assert [(64 * i + 3) // 7 for i in range(8)] == list(R.W3)
    assert [(64 * i + 7) // 15 for i in range(16)] == list(R.W4)


def test_to_u8_of_a_decoded_byte_is_the_byte():
    b = np.arange(256, dtype=np.float32)
    v = b / np.float32(255.0)
    back = np.minimum(np.clip(v, 0, 1) * np.float32(255.0), np.float32(255.0)).astype(np.uint8)
    assert v.dtype == np.float32 and np.array_equal(back, np.arange(256))


# ------------------------------------------------------------------ kc_dds_parse
def parse(L, data):
    from kanter_core_amd import _lib
    info = _lib.kc_dds_info()
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
    status = L.kc_dds_parse(buf, len(data), C.byref(info))
    return status, {k: getattr(info, k) for k in ("width", "height", "format", "flags", "levels", "data_offset", "data_bytes")}


def both(L, data):
    """the library's answer, checked against the reference parser's"""
    status, got = parse(L, data)
    try:
        want = R.dds_parse(data)
    except R.DdsError as e:
        assert status == e.code, (status, e.code, str(e))
        return status, None
    assert status == KC_OK and got == want, (status, got, want)
    return status, got


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (64, 16), (64, 64), (130, 70)])
@pytest.mark.parametrize("fmt,srgb", sorted(R.DXGI))
@pytest.mark.parametrize("mips", [False, True])
def test_dds_header_parses_back(L, w, h, fmt, srgb, mips):
    """What kc_dds_header writes, kc_dds_parse reads back: every format it reads, with every sRGB flag the format allows."""
    from kanter_core_amd import api
    assert sorted(R.DXGI) == [(1, 0), (1, 1), (3, 0), (3, 1), (4, 0), (5, 0), (BC7, 0), (BC7, 1)]
    levels = api.mip_level_count(w, h) if mips else 1
    data = api.dds_header(w, h, fmt, bool(srgb), levels) + bytes(R.chain_bytes(w, h, fmt, levels))
    status, info = both(L, data)
    assert status == KC_OK
    assert info == dict(width=w, height=h, format=fmt, flags=srgb, levels=levels, data_offset=148, data_bytes=len(data) - 148)
    assert api.dds_parse(data) == api.DdsInfo(w, h, fmt, bool(srgb), levels, 148, len(data) - 148)
    assert both(L, data[:-1])[0] == KC_ERR_INVALID_ARG  # a short payload
    assert both(L, data + b"xyz")[0] == KC_OK            # bytes after the chain are not the parser's business


@pytest.mark.parametrize("w,h", [(64, 64), (130, 70)])
def test_a_bc6h_header_is_written_and_not_read_back(L, w, h):
    from kanter_core_amd import api
    for levels in (1, api.mip_level_count(w, h)):
        data = api.dds_header(w, h, BC6H, False, levels) + bytes(api.bc_mip_layout(w, h, BC6H)[1])
        assert struct.unpack("<I", data[128:132])[0] == 95
        assert parse(L, data)[0] == KC_ERR_UNSUPPORTED
    with pytest.raises(api.TexProError) as e:
        api.dds_header(w, h, BC6H, True, 1)  # no sRGB flag to go round with
    assert e.value.code == KC_ERR_UNSUPPORTED


@pytest.mark.parametrize("cc,fmt", [(b"DXT1", 1), (b"DXT5", 3), (b"ATI1", 4), (b"BC4U", 4), (b"ATI2", 5), (b"BC5U", 5)])
def test_legacy_fourcc_headers(L, cc, fmt):
    for levels in (1, 4):
        data = R.legacy_header(13, 9, cc, levels) + bytes(R.chain_bytes(13, 9, fmt, levels))
        status, info = both(L, data)
        assert status == KC_OK and info["format"] == fmt and info["data_offset"] == 128 and info["levels"] == levels and info["flags"] == 0
    for other in (b"DXT3", b"DXT2", b"BC4S", b"RGBG"):
        assert both(L, R.legacy_header(13, 9, other) + bytes(64))[0] == KC_ERR_UNSUPPORTED


def patched(data, word, value):
    return data[:4 * word] + struct.pack("<I", value) + data[4 * word + 4:]


def test_malformed_and_unsupported_headers(L):
    from kanter_core_amd import api
    good = api.dds_header(64, 16, BC7, False, 7) + bytes(R.chain_bytes(64, 16, BC7, 7))
    assert both(L, good)[0] == KC_OK
    for n in (0, 4, 127, 128, 147):
        assert both(L, good[:n])[0] == KC_ERR_INVALID_ARG, n
    assert L.kc_dds_parse(None, 200, None) == KC_ERR_INVALID_ARG
    assert both(L, b"DDZ " + good[4:])[0] == KC_ERR_INVALID_ARG
    assert both(L, patched(good, 1, 125))[0] == KC_ERR_INVALID_ARG   # dwSize
    assert both(L, patched(good, 19, 24))[0] == KC_ERR_INVALID_ARG   # the pixel format's size
    assert both(L, patched(good, 4, 0))[0] == KC_ERR_INVALID_ARG     # zero width
    assert both(L, patched(good, 7, 8))[0] == KC_ERR_INVALID_ARG     # 8 levels: a 64 x 16 chain has 7
    assert both(L, patched(good, 7, 0))[1]["levels"] == 1            # a zero count with the flag set reads as one level
    assert both(L, patched(good, 2, 0x81007))[1]["levels"] == 1      # no DDSD_MIPMAPCOUNT
    for dxgi in (95, 74, 28, 70, 81, 84, 97):  # BC6H, BC2, RGBA8, typeless BC1, signed BC4 and BC5, typeless BC7
        assert both(L, patched(good, 32, dxgi))[0] == KC_ERR_UNSUPPORTED, dxgi
    assert both(L, patched(good, 35, 2))[0] == KC_ERR_UNSUPPORTED         # array size
    assert both(L, patched(good, 34, 4))[0] == KC_ERR_UNSUPPORTED         # the DX10 cube flag
    assert both(L, patched(good, 28, 0x200))[0] == KC_ERR_UNSUPPORTED     # DDSCAPS2_CUBEMAP
    assert both(L, patched(good, 28, 0x200000))[0] == KC_ERR_UNSUPPORTED  # DDSCAPS2_VOLUME
    assert both(L, patched(good, 33, 4))[0] == KC_ERR_UNSUPPORTED         # TEXTURE3D
    assert both(L, patched(good, 20, 0x41))[0] == KC_ERR_UNSUPPORTED      # DDPF_RGB: uncompressed
    # malformed wins over unsupported, unsupported over the level and payload checks
    assert both(L, patched(patched(good, 32, 95), 1, 0))[0] == KC_ERR_INVALID_ARG
    assert both(L, patched(patched(good, 32, 95), 7, 99))[0] == KC_ERR_UNSUPPORTED


# ------------------------------------------------------------------ the decode and compare entries without a device
def test_decode_and_compare_refuse_in_the_documented_order(L, tmp_path):
    import torch
    from kanter_core_amd import _lib
    gpu = torch.cuda.is_available()  # the not-gpu suite also runs on a machine with a device, initialised or not
    needs_device = (KC_ERR_NO_DEVICE,) if not gpu else (KC_ERR_NO_DEVICE, KC_ERR_INVALID_ARG)
    img = C.c_void_p(1 << 20)  # never looked at: every call below returns before it would be
    out, n = C.c_void_p(), C.c_uint64()
    buf = (C.c_uint8 * 64)()
    err = _lib.kc_bc_error()
    D = _lib.kc_bc_image
    SRGB, GRAY = R.BC_SRGB, R.BC_GRAY
    # kc_image_from_bc: flags, then arguments, then the device
    for fmt in R.FORMATS:
        assert L.kc_image_from_bc(buf, 64, 8, 8, fmt, SRGB, C.byref(out), None) == KC_ERR_UNSUPPORTED
        assert L.kc_image_from_bc(buf, 64, 8, 8, fmt, 8, C.byref(out), None) == KC_ERR_UNSUPPORTED
        if fmt != 4:
            assert L.kc_image_from_bc(buf, 64, 8, 8, fmt, GRAY, C.byref(out), None) == KC_ERR_UNSUPPORTED
        bytes_needed = 4 * R.BLOCK_BYTES[fmt]
        assert L.kc_image_from_bc(buf, bytes_needed - 1, 8, 8, fmt, 0, C.byref(out), None) == KC_ERR_INVALID_ARG
        assert L.kc_image_from_bc(None, 64, 8, 8, fmt, 0, C.byref(out), None) == KC_ERR_INVALID_ARG
        assert L.kc_image_from_bc(buf, 64, 8, 8, fmt, 0, None, None) == KC_ERR_INVALID_ARG
        assert L.kc_image_from_bc(buf, 64, 0, 8, fmt, 0, C.byref(out), None) == KC_ERR_INVALID_ARG
        if not gpu:
            assert L.kc_image_from_bc(buf, bytes_needed, 8, 8, fmt, 0, C.byref(out), C.byref(n)) == KC_ERR_NO_DEVICE
    assert L.kc_image_from_bc(None, 0, 8, 8, 1, GRAY, None, None) == KC_ERR_UNSUPPORTED  # the flags come first
    assert L.kc_image_from_bc(buf, 64, 8, 8, 7, 0, C.byref(out), None) == KC_ERR_INVALID_ARG
    assert L.kc_image_from_bc(buf, 64, 1 << 18, 1 << 18, 4, 0, C.byref(out), None) == KC_ERR_INVALID_ARG  # 2^32 blocks
    if not gpu:
        assert L.kc_image_from_bc(buf, 32, 8, 8, 4, GRAY, C.byref(out), None) == KC_ERR_NO_DEVICE
    # kc_image_from_bc_device: flags, then kc_bc_image_validate (arithmetic, then the device)
    d = {f: D(1 << 20, 8, 8, f, 32) for f in R.FORMATS}
    for fmt in R.FORMATS:
        assert L.kc_image_from_bc_device(C.byref(d[fmt]), SRGB, None, C.byref(out), None) == KC_ERR_UNSUPPORTED
        if fmt != 4:
            assert L.kc_image_from_bc_device(C.byref(d[fmt]), GRAY, None, C.byref(out), None) == KC_ERR_UNSUPPORTED
        assert L.kc_image_from_bc_device(C.byref(d[fmt]), 0, None, None, None) == KC_ERR_INVALID_ARG
        assert L.kc_image_from_bc_device(C.byref(D(1 << 20, 8, 8, fmt, 8)), 0, None, C.byref(out), None) == KC_ERR_INVALID_ARG  # pitch
        assert L.kc_image_from_bc_device(C.byref(d[fmt]), 0, None, C.byref(out), C.byref(n)) in needs_device
    assert L.kc_image_from_bc_device(None, 0, None, C.byref(out), None) == KC_ERR_INVALID_ARG
    assert L.kc_image_from_bc_device(C.byref(D(1 << 20, 8, 8, 7, 32)), 0, None, C.byref(out), None) == KC_ERR_INVALID_ARG
    # the compare entries: kc_image_to_bc's flag rule, then arguments, then the device
    for fmt in (4, 5):
        assert L.kc_image_bc_error(img, fmt, SRGB, C.byref(err)) == KC_ERR_UNSUPPORTED
        assert L.kc_image_bc_compare(img, C.byref(d[fmt]), SRGB, C.byref(err)) == KC_ERR_UNSUPPORTED
        assert L.kc_live_graph_buffer_bc_error(None, 0, 0, fmt, SRGB, C.byref(err)) == KC_ERR_UNSUPPORTED
    for fmt in R.FORMATS:
        assert L.kc_image_bc_error(img, fmt, GRAY, C.byref(err)) == KC_ERR_UNSUPPORTED
        assert L.kc_image_bc_compare(img, C.byref(d[fmt]), GRAY, C.byref(err)) == KC_ERR_UNSUPPORTED
        assert L.kc_image_bc_error(None, fmt, 0, C.byref(err)) == KC_ERR_INVALID_ARG
        assert L.kc_image_bc_error(img, fmt, 0, None) == KC_ERR_INVALID_ARG
        assert L.kc_image_bc_compare(None, C.byref(d[fmt]), 0, C.byref(err)) == KC_ERR_INVALID_ARG
        assert L.kc_image_bc_compare(img, C.byref(d[fmt]), 0, None) == KC_ERR_INVALID_ARG
        assert L.kc_live_graph_buffer_bc_error(None, 0, 0, fmt, 0, C.byref(err)) == KC_ERR_INVALID_ARG
        if not gpu:
            assert L.kc_image_bc_error(img, fmt, 0, C.byref(err)) == KC_ERR_NO_DEVICE
            assert L.kc_image_bc_compare(img, C.byref(d[fmt]), 0, C.byref(err)) == KC_ERR_NO_DEVICE
    assert L.kc_image_bc_error(img, 7, 0, C.byref(err)) == KC_ERR_INVALID_ARG
    assert L.kc_image_bc_compare(img, None, 0, C.byref(err)) == KC_ERR_INVALID_ARG
    assert L.kc_image_bc_compare(img, C.byref(D(1 << 20, 8, 8, 7, 32)), 0, C.byref(err)) == KC_ERR_INVALID_ARG
    # kc_image_read_dds: flags, arguments, the file, the header, the level, then kc_image_from_bc
    from kanter_core_amd import api
    good = tmp_path / "good.dds"
    good.write_bytes(api.dds_header(8, 8, 1, False, 4) + bytes(R.chain_bytes(8, 8, 1, 4)))
    short = tmp_path / "short.dds"
    short.write_bytes(good.read_bytes()[:-1])
    bc6 = tmp_path / "bc6.dds"
    bc6.write_bytes(patched(good.read_bytes(), 32, 95))
    info = _lib.kc_dds_info()
    path = lambda p: str(p).encode()
    assert L.kc_image_read_dds(path(good), 0, SRGB, C.byref(out), None) == KC_ERR_UNSUPPORTED
    assert L.kc_image_read_dds(None, 0, 0, C.byref(out), None) == KC_ERR_INVALID_ARG
    assert L.kc_image_read_dds(path(good), 0, 0, None, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_read_dds(path(tmp_path / "none.dds"), 0, 0, C.byref(out), None) == R.KC_ERR_IO
    assert L.kc_image_read_dds(path(short), 0, 0, C.byref(out), None) == KC_ERR_INVALID_ARG
    assert L.kc_image_read_dds(path(bc6), 0, 0, C.byref(out), None) == KC_ERR_UNSUPPORTED
    assert L.kc_image_read_dds(path(good), 4, 0, C.byref(out), C.byref(info)) == KC_ERR_INVALID_ARG
    assert (info.width, info.height, info.format, info.levels, info.data_offset) == (8, 8, 1, 4, 148)  # written once the header parsed
    assert L.kc_image_read_dds(path(good), 0, GRAY, C.byref(out), None) == KC_ERR_UNSUPPORTED  # BC1 has no Gray form
    if not gpu:
        assert L.kc_image_read_dds(path(good), 3, 0, C.byref(out), None) == KC_ERR_NO_DEVICE


def test_struct_layouts_match_the_header(tmp_path):
    import shutil
    import subprocess
    from kanter_core_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kanter_core_amd.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %u\\n", '
                   'sizeof(kc_bc_error), offsetof(kc_bc_error, sse), offsetof(kc_bc_error, undecoded_blocks), offsetof(kc_bc_error, bc7_mode_blocks), '
                   'sizeof(kc_dds_info), offsetof(kc_dds_info, data_offset), KC_BC_GRAY); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    E, I = _lib.kc_bc_error, _lib.kc_dds_info
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == [
        C.sizeof(E), E.sse.offset, E.undecoded_blocks.offset, E.bc7_mode_blocks.offset, C.sizeof(I), I.data_offset.offset, R.BC_GRAY]
