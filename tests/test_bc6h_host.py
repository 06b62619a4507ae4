"""BC6H without a device: the numpy reference of the contract (tests/bc6h_ref.py) against Pillow's decoder -- exactly, under the
one documented difference of the rounding term -- its encoder against its own decoder, the source quantiser on the values
where a half rounds, saturates or flushes, what the random blocks of the GPU tests cover, and the argument checks of every entry
point that takes KC_BC6H = 95 before kc_init, in the documented order."""
import ctypes as C
import io
import struct

import numpy as np
import pytest

import bc6h_ref as R

BC6H, BC7 = R.BC6H, 98
KC_OK, KC_ERR_NO_DEVICE, KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 0, 101, 102, 104
BC_SRGB, MIP_PER_LEVEL, BC_GRAY = 1, 2, 4


@pytest.fixture(scope="module")
def L():
    from kanter_core_amd import _lib
    return _lib.load()


def hdr_image(h, w, seed=5):
    """three f32 planes with an HDR range: mostly inside [0, 1], a tail up to a few hundred, some negatives"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = [np.sin(xx / 9 + c) * np.cos(yy / 7 - c) * 0.5 + 0.45 for c in range(3)]
    return [(b + rng.random((h, w), dtype=np.float32) ** 8 * 300 - 0.02).astype(np.float32) for b in base]


# ------------------------------------------------------------------ Pillow
def pillow_decode(blk, h, w):
    Image = pytest.importorskip("PIL.Image")
    from kanter_core_amd import api
    data = api.dds_header(w, h, BC6H, levels=1) + np.ascontiguousarray(blk, np.uint8).tobytes()
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == "RGB" and im.size == (w, h)
    return np.asarray(im)


def as_image(blk):
    """n blocks as an image one block high"""
    return blk.reshape(1, len(blk), 16), 4, 4 * len(blk)


@pytest.mark.parametrize("mode", [11, 12, 13, 14])
def test_reference_equals_pillow_on_every_single_subset_mode(mode):
    """500 blocks of the mode: 250 with any endpoints, 250 with endpoint 0 in the lower half of its range, so that most texels
    lie inside [0, 1] where Pillow's bytes tell values apart.  decode(round_term=0) is Pillow's rule; no block is left out."""
    pytest.importorskip("PIL")
    blk = np.concatenate([R.random_blocks(250, seed=mode, only=mode), R.random_blocks(250, seed=mode + 50, only=mode, low=True)])
    assert (R.modes(blk) == mode).all()
    b, h, w = as_image(blk)
    want = pillow_decode(b, h, w)
    px, modes, n = R.decode(b, h, w, round_term=0)
    assert n == 0 and px.max() <= R.HALF_MAX
    inside = (R.half_value(px[:, 250 * 4:]) < 1).mean()
    assert inside > 0.5, inside  # most texels of the lower-half blocks do land inside [0, 1]
    got = R.pillow_bytes(px)
    assert np.array_equal(got, want), np.argwhere((got != want).any(-1))[:4]
    # the contract's + 32 moves a few bytes by one, never more
    diff = np.abs(R.pillow_bytes(R.decode(b, h, w)[0]).astype(int) - want)
    assert diff.max() <= 1 and (diff != 0).mean() < 0.01


def test_reference_encoding_equals_pillow():
    pytest.importorskip("PIL")
    planes = hdr_image(64, 64)
    blk = R.encode(planes)
    assert blk.shape == (16, 16, 16) and (R.modes(blk.reshape(-1, 16)) == 11).all()
    px = R.decode(blk, 64, 64, round_term=0)[0]
    assert np.array_equal(R.pillow_bytes(px), pillow_decode(blk, 64, 64))


# ------------------------------------------------------------------ the encoder against the decoder
def test_encode_round_trip_is_consistent():
    planes = hdr_image(37, 53, seed=9)
    src = R.blocks(R.texels(planes)).reshape(-1, 16, 3)
    d = R.encode_detail(src)
    blk = d["blocks"]
    dec, modes = R.decode_blocks(blk)
    assert (modes == 11).all() and (d["idx"][:, 0] < 8).all()
    pal = R.palette(d["q0"], d["q1"])  # of the endpoints as stored
    assert np.array_equal(dec, np.take_along_axis(pal, d["idx"][:, :, None], 1))
    # every texel has the nearest entry of its block's palette, and no other block field changes what decodes
    dist = ((src[:, :, None, :] - pal[:, None, :, :]) ** 2).sum(-1)
    assert np.array_equal(dist.min(-1), ((src - dec) ** 2).sum(-1))
    bits = R._bits(blk)
    assert (R._get(bits, 0, 5)[:, 0] == 3).all()
    assert np.array_equal(R._get(bits, 5, 10, 3), d["q0"]) and np.array_equal(R._get(bits, 35, 10, 3), d["q1"])
    assert d["swap"].any() and not d["swap"].all()
    # the endpoints are the box corners, each quantised to the nearest value a 10-bit endpoint decodes to
    lo, hi = src.min(1), src.max(1)
    ends = np.sort(np.stack([R.E10[d["q0"]], R.E10[d["q1"]]], -1), -1)
    assert (np.abs(ends[..., 0] - lo) <= 23).all() and (np.abs(ends[..., 1] - hi) <= 23).all()  # half of E10's widest step, 46


def test_constant_block():
    for e in (0, 1, 23, 24, 15360, 31720, 31721, R.HALF_MAX):
        p = np.full((1, 16, 3), e, np.int64)
        d = R.encode_detail(p)
        assert (d["idx"] == 0).all() and np.array_equal(d["q0"], d["q1"]) and (d["q0"] == R.q10(e)).all(), e
        assert abs(int(R.decode_blocks(d["blocks"])[0][0, 0, 0]) - e) <= 23


def test_q10_is_the_nearest_endpoint_and_the_closed_form_needs_its_neighbours():
    e = np.arange(R.HALF_MAX + 1)
    q = R.q10(e)
    assert q[0] == 0 and q[23] == 0 and q[24] == 1 and q[31720] == 1022 and q[31721] == 1023 and q[-1] == 1023
    assert (np.diff(q) >= 0).all() and set(q) == set(range(1024))
    plain = np.clip(e // 31, 0, 1023)
    assert 0 < (plain != q).mean() < 0.001 and np.abs(plain - q).max() == 1


def test_quant_half_edge_values():
    f = np.float32
    tie = f(2.9802322e-8)  # 2^-25: halfway between 0 and the smallest denormal half, rounds to even
    assert tie == f(2.0) ** -25
    cases = [(65504.0, 0x7BFF), (65519.99, 0x7BFF), (65520.0, 0x7BFF), (1e30, 0x7BFF), (np.inf, 0x7BFF), (-np.inf, 0), (np.nan, 0),
             (-0.0, 0), (0.0, 0), (-1.0, 0), (6.1035e-5, 0x0400), (5.96e-8, 1), (tie, 0), (np.nextafter(tie, f(1)), 1),
             (1.0, 0x3C00), (1.0 + 2.0 ** -11, 0x3C00), (1.0 + 3 * 2.0 ** -11, 0x3C02), (0.5, 0x3800), (65503.99, 0x7BFF), (65472.0, 0x7BFE),
             (65488.0, 0x7BFF + 1 - 2)]  # the last: a tie between 0x7BFE and 0x7BFF, to even
    for v, want in cases:
        assert int(R.quant_half(f(v))) == want, (v, hex(int(R.quant_half(f(v)))), hex(want))
    got = R.quant_half(np.array([c[0] for c in cases], f))
    assert got.dtype == np.int64 and got.max() <= R.HALF_MAX and got.min() >= 0
    assert np.array_equal(R.half_value(got[:5]), np.full(5, 65504.0, f))


# ------------------------------------------------------------------ what the random blocks cover
def test_the_random_blocks_cover_every_mode_value():
    blk = R.random_blocks(2 * len(R.CYCLE))
    mode = R.modes(blk)
    assert [int((mode == m).sum()) for m in range(15)] == [8] + [2] * 10 + [8] * 4
    assert set(blk[mode == 0, 0] & 31) == set(R.RESERVED)
    assert R.undecoded(mode).sum() == 20
    for m in range(1, 15):
        f = blk[mode == m, 0] & (3 if m < 3 else 31)
        assert (f == R.FIELD[m]).all()
    dec, _ = R.decode_blocks(blk)
    assert not dec[mode <= 10].any() and all(dec[mode == m].any() for m in (11, 12, 13, 14))
    assert dec.max() <= R.HALF_MAX
    # the smallest image of the GPU tests that holds a whole cycle has every mode value
    small = R.random_image_blocks(64, 64).reshape(-1, 16)
    assert set(R.modes(small)) == set(range(15)) and set(small[R.modes(small) == 0, 0] & 31) == set(R.RESERVED)
    # deltas of both signs in each delta mode; the 160 x 120 image of the GPU tests also has sums that wrap modulo 2^n both ways
    for blocks, wraps in ((small, False), (R.random_image_blocks(120, 160, seed=2).reshape(-1, 16), True)):
        bits, mode = R._bits(blocks), R.modes(blocks)
        for m, (nb, db) in R.SINGLE.items():
            if db == 0:
                continue
            low, grp = R._get(bits, 5, 10, 3)[mode == m], R._get(bits, 35, 10, 3)[mode == m]
            delta = grp & ((1 << db) - 1)
            delta = delta - ((delta >> (db - 1)) << db)
            assert (delta < 0).any() and (delta > 0).any()
            if wraps and nb < 16:  # mode 14's four delta bits reach a wrap only from the sixteen values next to the ends
                high = sum(((grp >> (9 - j)) & 1) << (10 + j) for j in range(nb - 10))
                total = (low | high) + delta
                assert (total < 0).any() and (total >= 1 << nb).any(), m
    low = R.random_blocks(64, seed=3, low=True)
    assert np.array_equal(R.modes(low), R.modes(R.random_blocks(64, seed=3)))


def test_compare_record():
    planes = hdr_image(9, 14, seed=2)
    own = R.compare(planes, R.encode(planes))
    assert own["undecoded_blocks"] == 0 and own["channel_mask"] == 7 and own["pixels"] == 126 and own["sse"][3] == 0
    other = R.compare(planes, R.random_image_blocks(9, 14))
    assert sum(other["sse"]) > sum(own["sse"]) and max(other["max_abs"]) <= R.HALF_MAX
    assert R.psnr(own) > R.psnr(other)
    zero = R.compare([np.zeros((4, 4), np.float32)], np.zeros((1, 1, 16), np.uint8))  # a two-subset block: (0, 0, 0)
    assert zero["sse"] == [0, 0, 0, 0] and zero["undecoded_blocks"] == 1 and R.psnr(zero) == float("inf")


# ------------------------------------------------------------------ the library without a device
def test_python_names():
    from kanter_core_amd import api
    import kanter_core_amd as kc
    assert kc.BC6H == api.BC6H == 95 and api.BC_BLOCK_BYTES[95] == 16
    assert api._bc_format("bc6h") == api._bc_format("BC6H") == api._bc_format(95) == 95
    for bad in (6, "bc6", "6h", 96, "bc6s"):
        with pytest.raises(ValueError):
            api._bc_format(bad)
    e = api.BcError(95, 0, 7, 16, np.array([31743 ** 2 * 16, 0, 0, 0], np.uint64), np.zeros(4, np.uint32), 0, np.zeros(8, np.uint64))
    assert e.psnr(channels=[0]) == pytest.approx(0.0, abs=1e-9) and e.psnr(channels=[1]) == float("inf")
    assert "31743" in api.BcError.psnr.__doc__


def test_dds_header_and_mip_layout(L):
    from kanter_core_amd import api
    for w, h in ((1, 1), (5, 3), (64, 16), (130, 70)):
        h6, h7 = api.dds_header(w, h, BC6H), api.dds_header(w, h, BC7)
        assert len(h6) == 148 and struct.unpack("<I", h6[128:132])[0] == 95
        assert h6[:128] == h7[:128] and h6[132:] == h7[132:]  # nothing but the dxgiFormat differs: the blocks are 16 bytes too
        assert api.bc_mip_layout(w, h, BC6H) == api.bc_mip_layout(w, h, BC7)
        assert api.dds_header(w, h, "bc6h", levels=1)[128:132] == h6[128:132]
    out = (C.c_uint8 * 148)()
    assert L.kc_dds_header(8, 8, BC6H, BC_SRGB, 1, out, None) == KC_ERR_UNSUPPORTED  # no sRGB form
    assert L.kc_dds_header(8, 8, BC6H, 2, 1, out, None) == KC_ERR_UNSUPPORTED
    assert L.kc_dds_header(8, 8, BC6H, 0, 5, out, None) == KC_ERR_INVALID_ARG
    assert L.kc_dds_header(8, 8, BC6H, 0, 4, None, None) == KC_ERR_INVALID_ARG
    assert L.kc_dds_header(8, 8, 96, 0, 1, out, None) == KC_ERR_INVALID_ARG  # the signed form is not a format
    assert L.kc_bc_mip_layout(0, 8, BC6H, None, None, 0, None) == KC_ERR_INVALID_ARG


def test_reading_a_bc6h_dds_stays_unsupported(L, tmp_path):
    """The file kc_image_write_dds writes for KC_BC6H is not read back by this library: the one stated gap."""
    from kanter_core_amd import _lib, api
    data = api.dds_header(8, 8, BC6H, levels=1) + bytes(64)
    info = _lib.kc_dds_info()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    assert L.kc_dds_parse(buf, len(data), C.byref(info)) == KC_ERR_UNSUPPORTED
    path = tmp_path / "hdr.dds"
    path.write_bytes(data)
    out = C.c_void_p()
    assert L.kc_image_read_dds(str(path).encode(), 0, 0, C.byref(out), None) == KC_ERR_UNSUPPORTED


def test_every_entry_point_refuses_in_the_documented_order(L, tmp_path):
    import torch
    from kanter_core_amd import _lib
    gpu = torch.cuda.is_available()  # the not-gpu suite also runs on a machine with a device, initialised or not
    needs_device = (KC_ERR_NO_DEVICE,) if not gpu else (KC_ERR_NO_DEVICE, KC_ERR_INVALID_ARG)
    img = C.c_void_p(1 << 20)  # never looked at: every call below returns before it would be
    out, n, ext = C.c_void_p(), C.c_uint64(), C.c_size_t()
    buf = (C.c_uint8 * 64)()
    err = _lib.kc_bc_error()
    D = _lib.kc_bc_image
    d = D(1 << 20, 8, 8, BC6H, 32)
    # kc_bc_image_validate: arithmetic, then the device
    assert L.kc_bc_image_validate(C.byref(d), C.byref(ext)) in needs_device and ext.value == 64
    assert L.kc_bc_image_validate(C.byref(D(1 << 20, 8, 8, BC6H, 24)), None) == KC_ERR_INVALID_ARG      # pitch below a row
    assert L.kc_bc_image_validate(C.byref(D((1 << 20) + 8, 8, 8, BC6H, 32)), None) == KC_ERR_INVALID_ARG  # 8 is not 16-byte aligned
    assert L.kc_bc_image_validate(C.byref(D(1 << 20, 0, 8, BC6H, 32)), None) == KC_ERR_INVALID_ARG
    assert L.kc_bc_image_validate(C.byref(D(1 << 20, 8, 8, 96, 32)), None) == KC_ERR_INVALID_ARG
    # the encoders: flags (sRGB has no meaning for half floats), then arguments, then the device
    assert L.kc_image_to_bc(None, BC6H, BC_SRGB, None, 0) == KC_ERR_UNSUPPORTED
    assert L.kc_image_to_bc(img, BC6H, MIP_PER_LEVEL, buf, 64) == KC_ERR_UNSUPPORTED
    assert L.kc_image_to_bc(None, BC6H, 0, buf, 64) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc(img, BC6H, 0, None, 64) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_device(img, C.byref(d), BC_SRGB, None) == KC_ERR_UNSUPPORTED
    assert L.kc_image_to_bc_device(img, C.byref(D(1 << 20, 8, 8, BC6H, 24)), 0, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_device(img, C.byref(d), 0, None) in needs_device
    assert L.kc_live_graph_buffer_bc(None, 0, 0, C.byref(d), 0, None) == KC_ERR_INVALID_ARG
    for flags in (BC_SRGB, BC_SRGB | MIP_PER_LEVEL, 8):
        assert L.kc_image_to_bc_mips(img, BC6H, flags, buf, 64) == KC_ERR_UNSUPPORTED
        assert L.kc_image_to_bc_mips_device(img, BC6H, flags, C.c_void_p(1 << 20), 64, None) == KC_ERR_UNSUPPORTED
        assert L.kc_image_write_dds(img, b"x.dds", BC6H, flags, 1) == KC_ERR_UNSUPPORTED
    assert L.kc_live_graph_buffer_bc_mips(None, 0, 0, BC6H, 8, C.c_void_p(1 << 20), 64, None) == KC_ERR_UNSUPPORTED
    assert L.kc_image_to_bc_mips(None, BC6H, MIP_PER_LEVEL, buf, 64) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_mips_device(img, BC6H, 0, C.c_void_p((1 << 20) + 8), 64, None) == KC_ERR_INVALID_ARG  # alignment
    assert L.kc_image_to_bc_mips_device(None, BC6H, 0, C.c_void_p(1 << 20), 64, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_write_dds(None, b"x.dds", BC6H, 0, 1) == KC_ERR_INVALID_ARG
    assert L.kc_image_write_dds(img, None, BC6H, MIP_PER_LEVEL, 0) == KC_ERR_INVALID_ARG
    if not gpu:
        assert L.kc_image_to_bc(img, BC6H, 0, buf, 64) == KC_ERR_NO_DEVICE
        assert L.kc_image_to_bc_mips(img, BC6H, 0, buf, 64) == KC_ERR_NO_DEVICE
        assert L.kc_image_to_bc_mips_device(img, BC6H, 0, C.c_void_p(1 << 20), 64, None) == KC_ERR_NO_DEVICE
        assert L.kc_image_write_dds(img, b"x.dds", BC6H, 0, 1) == KC_ERR_NO_DEVICE
    # kc_image_from_bc: flags, then arguments, then the device
    assert L.kc_image_from_bc(None, 0, 8, 8, BC6H, BC_SRGB, None, None) == KC_ERR_UNSUPPORTED
    assert L.kc_image_from_bc(buf, 64, 8, 8, BC6H, BC_GRAY, C.byref(out), None) == KC_ERR_UNSUPPORTED  # KC_BC_GRAY stays BC4's
    assert L.kc_image_from_bc(buf, 64, 8, 8, BC6H, 8, C.byref(out), None) == KC_ERR_UNSUPPORTED
    assert L.kc_image_from_bc(buf, 63, 8, 8, BC6H, 0, C.byref(out), None) == KC_ERR_INVALID_ARG
    assert L.kc_image_from_bc(None, 64, 8, 8, BC6H, 0, C.byref(out), None) == KC_ERR_INVALID_ARG
    assert L.kc_image_from_bc(buf, 64, 8, 8, BC6H, 0, None, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_from_bc(buf, 64, 0, 8, BC6H, 0, C.byref(out), None) == KC_ERR_INVALID_ARG
    assert L.kc_image_from_bc(buf, 64, 1 << 18, 1 << 18, BC6H, 0, C.byref(out), None) == KC_ERR_INVALID_ARG  # 2^32 blocks
    assert L.kc_image_from_bc(buf, 64, 8, 8, 96, 0, C.byref(out), None) == KC_ERR_INVALID_ARG
    if not gpu:
        assert L.kc_image_from_bc(buf, 64, 8, 8, BC6H, 0, C.byref(out), C.byref(n)) == KC_ERR_NO_DEVICE
    # kc_image_from_bc_device: flags, then kc_bc_image_validate
    assert L.kc_image_from_bc_device(C.byref(d), BC_SRGB, None, C.byref(out), None) == KC_ERR_UNSUPPORTED
    assert L.kc_image_from_bc_device(C.byref(d), BC_GRAY, None, C.byref(out), None) == KC_ERR_UNSUPPORTED
    assert L.kc_image_from_bc_device(C.byref(d), 0, None, None, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_from_bc_device(C.byref(D(1 << 20, 8, 8, BC6H, 16)), 0, None, C.byref(out), None) == KC_ERR_INVALID_ARG  # pitch
    assert L.kc_image_from_bc_device(C.byref(d), 0, None, C.byref(out), C.byref(n)) in needs_device
    # the compare entries: kc_image_to_bc's flag rule, then arguments, then the device
    for flags in (BC_SRGB, BC_GRAY):
        assert L.kc_image_bc_error(img, BC6H, flags, C.byref(err)) == KC_ERR_UNSUPPORTED
        assert L.kc_image_bc_compare(img, C.byref(d), flags, C.byref(err)) == KC_ERR_UNSUPPORTED
        assert L.kc_live_graph_buffer_bc_error(None, 0, 0, BC6H, flags, C.byref(err)) == KC_ERR_UNSUPPORTED
    assert L.kc_image_bc_error(None, BC6H, 0, C.byref(err)) == KC_ERR_INVALID_ARG
    assert L.kc_image_bc_error(img, BC6H, 0, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_bc_compare(None, C.byref(d), 0, C.byref(err)) == KC_ERR_INVALID_ARG
    assert L.kc_image_bc_compare(img, C.byref(d), 0, None) == KC_ERR_INVALID_ARG
    assert L.kc_live_graph_buffer_bc_error(None, 0, 0, BC6H, 0, C.byref(err)) == KC_ERR_INVALID_ARG
    if not gpu:
        assert L.kc_image_bc_error(img, BC6H, 0, C.byref(err)) == KC_ERR_NO_DEVICE
        assert L.kc_image_bc_compare(img, C.byref(d), 0, C.byref(err)) == KC_ERR_NO_DEVICE
