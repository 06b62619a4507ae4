"""The host half of KC_BC_PUNCH_THROUGH (include/kanter_core_amd.h), on a machine without a GPU: tests/bc1a_ref.py is held to the
contract's own words, kc_bc1_punch_through_block equals it bit for bit, the flag is accepted and refused where and in the order
the contract says, and on a cutout with magenta under the transparent texels the rule is at least as close to the visible pixels
as plain BC1."""
import ctypes as C

import numpy as np
import pytest

import bc1a_ref as R
import bc_decode_ref
import bc_ref
import mip_coverage_ref

KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 102, 104
BC_SRGB, MIP_PER_LEVEL, BC_GRAY, BC_ALL_MODES, MIP_NORMALS, MIP_COVERAGE, MIP_ALPHA_WEIGHT, BC_PUNCH_THROUGH = 1, 2, 4, 16, 32, 64, 128, 256
REFS = [1, 2, 127, 128, 254, 255]


def pt(b):
    return BC_PUNCH_THROUGH | b << 24


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    return kc


@pytest.fixture(scope="module")
def L():
    from kanter_core_amd import _lib
    return _lib.load()


def class_image(h, w, ref, seed=0):
    """RGBA8 bytes with random colour and bc1a_ref.class_alpha's alpha, quantised as kc_image_to_u8 quantises it"""
    rng = np.random.default_rng([seed, ref])
    a = mip_coverage_ref.quant_u8(R.class_alpha(h, w, mip_coverage_ref.threshold(ref), seed))
    return np.concatenate([rng.integers(0, 256, (h, w, 3)), a[..., None]], -1).astype(np.uint8)


# ------------------------------------------------------------------ the reference against the contract's own words
@pytest.mark.parametrize("ref", [1, 128, 255])
def test_the_reference_follows_the_contract(ref):
    h, w = 37, 41  # edge blocks on both sides
    px = class_image(h, w, ref)
    assert min(R.class_counts(px, ref)) > 0, R.class_counts(px, ref)
    t = bc_ref.blocks(px).reshape(-1, 16, 4)
    blk = R.encode(px, ref)
    flat = blk.reshape(-1, 8)
    op = t[..., 3] >= ref
    n = op.sum(-1)
    assert np.array_equal(flat[n == 16], bc_ref.encode_bc1(t[n == 16][..., :3]))
    assert (flat[n == 0] == np.array([0, 0, 0, 0, 255, 255, 255, 255], np.uint8)).all()
    mixed = (n > 0) & (n < 16)
    b = flat[mixed].astype(np.int64)
    c0, c1 = b[:, 0] | b[:, 1] << 8, b[:, 2] | b[:, 3] << 8
    assert (c0 <= c1).all()
    word = b[:, 4] | b[:, 5] << 8 | b[:, 6] << 16 | b[:, 7] << 24
    idx = (word[:, None] >> (2 * np.arange(16))) & 3
    assert np.array_equal(idx == 3, ~op[mixed])
    # the palette as the decoder yields it: the same endpoints with texels 0, 1, 2 on indices 0, 1, 2
    probe = flat[mixed].copy()
    probe[:, 4:] = [0b00100100, 0, 0, 0]
    pal = bc_ref.decode_bc1(probe)[:, :3, :]  # (blocks, 3 entries, 3 channels)
    p = t[mixed][..., :3]
    best = np.full(idx.shape, -1)
    best_d = np.full(idx.shape, np.iinfo(np.int64).max)
    for j in range(3):
        d = ((p - pal[:, None, j, :]) ** 2).sum(-1)
        best = np.where(d < best_d, j, best)  # strictly lower: the lowest j keeps a tie
        best_d = np.minimum(d, best_d)
    assert np.array_equal(idx[op[mixed]], best[op[mixed]])
    # decoded alpha is 0 exactly where the source is not opaque
    dec, undecoded = bc_decode_ref.decode(blk, 1, h, w)
    assert undecoded == 0
    assert np.array_equal(dec[..., 3] == 0, px[..., 3] < ref) and set(np.unique(dec[..., 3])) <= {0, 255}
    assert np.array_equal(dec, R.decode(blk, h, w))


def test_an_opaque_image_gives_plain_bc1():
    px = class_image(21, 30, 128)
    px[..., 3] = np.maximum(px[..., 3], 128)
    assert np.array_equal(R.encode(px, 128), bc_ref.encode(px, 1))


# ------------------------------------------------------------------ kc_bc1_punch_through_block
def special_blocks(rng, ref, count):
    """One colour; one opaque texel; equal opaque texels under differing transparent ones (c0 == c1)"""
    t = rng.integers(0, 256, (3 * count, 16, 4))
    t[:count, :, :3] = t[:count, :1, :3]
    alpha = rng.integers(0, 256, (count, 16))
    t[:count, :, 3] = alpha
    t[count:2 * count, :, 3] = ref - 1
    t[np.arange(count, 2 * count), rng.integers(0, 16, count), 3] = ref
    op = rng.random((count, 16)) < 0.5
    op[:, 0] = True
    t[2 * count:, :, :3] = np.where(op[..., None], t[2 * count:, :1, :3], t[2 * count:, :, :3])
    t[2 * count:, :, 3] = np.where(op, 255, 0)
    return t


def test_the_block_function_equals_the_reference(L):
    total = 0
    for ref in REFS:
        rng = np.random.default_rng([5, ref])
        t = rng.integers(0, 256, (3600, 16, 4))
        cls = np.arange(len(t)) % 3
        t[cls == 1, :, 3] = rng.integers(0, ref, (int((cls == 1).sum()), 16))
        t[cls == 2, :, 3] = rng.integers(ref, 256, (int((cls == 2).sum()), 16))
        narrow = np.arange(len(t)) % 2 == 1  # colours of a small range: equal endpoints and index ties
        t[narrow, :, :3] = 100 + t[narrow, :, :3] // 32
        t = np.concatenate([t, special_blocks(rng, ref, 60)]).astype(np.uint8)
        n = (t[..., 3] >= ref).sum(-1)
        if ref not in (1, 255):  # at B = 1 a random byte is practically never below; at 255 practically never at it
            assert (n == 0).sum() > 100 and (n == 16).sum() > 100 and ((n > 0) & (n < 16)).sum() > 100
        want = R.encode_blocks(t, ref)
        got = np.zeros_like(want)
        for i in range(len(t)):
            assert L.kc_bc1_punch_through_block(t[i].ctypes.data, ref, got[i].ctypes.data) == 0
        bad = np.flatnonzero((got != want).any(-1))
        assert bad.size == 0, (ref, len(bad), t[bad[0]].tolist(), got[bad[0]].tobytes().hex(), want[bad[0]].tobytes().hex())
        b = want.astype(np.int64)
        assert ((b[:, 0] | b[:, 1] << 8) == (b[:, 2] | b[:, 3] << 8))[(n > 0) & (n < 16)].any()  # c0 == c1 among the mixed blocks
        total += len(t)
    assert total >= 20000


def test_the_block_function_refuses_bad_arguments_and_writes_nothing(L, kc):
    t = np.full((16, 4), 200, np.uint8)
    out = np.full(8, 0xa5, np.uint8)
    for ref in (0, 256, 1 << 24):
        assert L.kc_bc1_punch_through_block(t.ctypes.data, ref, out.ctypes.data) == KC_ERR_INVALID_ARG
    assert L.kc_bc1_punch_through_block(None, 128, out.ctypes.data) == KC_ERR_INVALID_ARG
    assert L.kc_bc1_punch_through_block(t.ctypes.data, 128, None) == KC_ERR_INVALID_ARG
    assert (out == 0xa5).all()
    assert np.array_equal(kc.bc1_punch_through_block(t.reshape(4, 4, 4), 128), bc_ref.encode_bc1(t[None, :, :3].astype(np.int64))[0])
    with pytest.raises(ValueError):
        kc.bc1_punch_through_block(t[:15], 128)


# ------------------------------------------------------------------ the flag
def test_the_python_flag_word(kc):
    from kanter_core_amd import api
    assert kc.BC_PUNCH_THROUGH == BC_PUNCH_THROUGH and kc.bc_punch_through_ref(128) == pt(128)
    for bad in (0, 256, -1):
        with pytest.raises(ValueError):
            kc.bc_punch_through_ref(bad)
    assert api._punch_flags(None) == 0 and api._punch_flags(7) == pt(7)
    assert api._mip_flags(True, False, False, 128, False, True) == BC_SRGB | MIP_COVERAGE | BC_PUNCH_THROUGH | 128 << 24
    assert api._mip_flags(False, True, False, 128, True, 128) == MIP_PER_LEVEL | MIP_COVERAGE | MIP_ALPHA_WEIGHT | BC_PUNCH_THROUGH | 128 << 24
    assert api._mip_flags(False, False, False, None, False, 1) == pt(1)  # a byte, not True
    with pytest.raises(ValueError):
        api._mip_flags(False, False, False, 128, False, 127)  # the two share one byte
    with pytest.raises(ValueError):
        api._mip_flags(False, False, False, None, False, True)  # True reuses coverage's byte
    with pytest.raises(ValueError):
        api._punch_flags(256)


def test_flag_errors_come_first_and_in_order(L, tmp_path):
    from kanter_core_amd import _lib
    img = C.c_void_p(1 << 20)  # never looked at: every call below is refused before it would be
    lg = C.c_void_p(1 << 20)
    buf = (C.c_uint8 * 64)()
    err = _lib.kc_bc_error()
    path = str(tmp_path / "x.dds").encode()
    d1 = _lib.kc_bc_image(None, 8, 8, 1, 16)  # BC1, and a NULL pointer: the first argument error after the flags
    d3 = _lib.kc_bc_image(None, 8, 8, 3, 32)

    def single(fmt, flags, d, host=buf, out=C.byref(err)):
        """the entry points of one level"""
        return [L.kc_image_to_bc(img, fmt, flags, host, 64), L.kc_image_to_bc_device(img, C.byref(d), flags, None),
                L.kc_live_graph_buffer_bc(lg if host is None else None, 0, 0, None if host is None else C.byref(d), flags, None),
                L.kc_image_bc_error(img, fmt, flags, out), L.kc_live_graph_buffer_bc_error(None, 0, 0, fmt, flags, out),
                L.kc_image_bc_compare(img, C.byref(d), flags, None),
                L.kc_image_levels_to_bc_mips(None, 1, fmt, flags, host, 64), L.kc_image_levels_write_dds(None, 1, path, fmt, flags)]

    def chain(fmt, flags, host=buf):
        """the entry points that build the chain themselves"""
        return [L.kc_image_to_bc_mips(img, fmt, flags, host, 64), L.kc_image_to_bc_mips_device(img, fmt, flags, None, 64, None),
                L.kc_live_graph_buffer_bc_mips(None, 0, 0, fmt, flags, buf, 64, None), L.kc_image_write_dds(img, None, fmt, flags, 1)]

    # a legal word gets past the flags everywhere: the next error is the NULL argument's
    for flags in (pt(1), pt(128), pt(255), pt(128) | BC_SRGB):
        assert single(1, flags, d1, host=None, out=None) == [KC_ERR_INVALID_ARG] * 8, flags
    for flags in (pt(1), pt(255) | BC_SRGB, pt(128) | MIP_COVERAGE, pt(85) | MIP_PER_LEVEL, pt(85) | MIP_ALPHA_WEIGHT,
                  pt(128) | MIP_COVERAGE | MIP_ALPHA_WEIGHT | MIP_PER_LEVEL | BC_SRGB):
        assert chain(1, flags, host=None) == [KC_ERR_INVALID_ARG] * 4, flags
    # the illegal words, refused before the NULL arguments: the flag with another format, with a zero byte, a byte with neither
    # flag, the flag with normals (elsewhere an unknown bit), and the bits that stay refused
    for fmt, flags, d in [(3, pt(128), d3), (4, pt(128), d3), (98, pt(128) | BC_SRGB, d3), (1, BC_PUNCH_THROUGH, d1), (1, 128 << 24, d1),
                          (1, 1 << 24 | BC_SRGB, d1), (1, pt(128) | MIP_NORMALS, d1), (1, pt(128) | 8, d1), (1, pt(128) | 512, d1)]:
        assert single(fmt, flags, d) == [KC_ERR_UNSUPPORTED] * 8, (fmt, flags)
        assert chain(fmt, flags) == [KC_ERR_UNSUPPORTED] * 4, (fmt, flags)
    assert chain(1, BC_PUNCH_THROUGH | MIP_COVERAGE) == [KC_ERR_UNSUPPORTED] * 4  # coverage does not bring a byte either
    # one level knows no chain flags, with or without the flag
    for flags in (pt(128) | MIP_COVERAGE, pt(128) | MIP_PER_LEVEL, pt(128) | MIP_ALPHA_WEIGHT, pt(128) | BC_GRAY):
        assert single(1, flags, d1) == [KC_ERR_UNSUPPORTED] * 8, flags
    assert L.kc_image_bc_compare(img, C.byref(d1), pt(128) | BC_ALL_MODES, None) == KC_ERR_INVALID_ARG  # the comparison's own flag stays
    assert not (tmp_path / "x.dds").exists()


def test_the_other_entry_points_refuse_the_flag(L):
    from kanter_core_amd import _lib
    img = C.c_void_p(1 << 20)
    out = (C.c_uint8 * 148)()
    levels, count, res = (C.c_void_p * 16)(), C.c_uint32(), C.c_void_p()
    recs = (_lib.kc_mip_coverage_level * 16)()
    reqs = (_lib.kc_preview_request * 1)()
    d1 = _lib.kc_bc_image(None, 8, 8, 1, 16)
    for flags in (pt(128), BC_PUNCH_THROUGH, pt(128) | BC_SRGB):
        assert L.kc_dds_header(64, 64, 1, flags, 7, out, None) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_build_mips(img, flags, levels, 16, C.byref(count)) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_build_mips(img, flags | MIP_COVERAGE, levels, 16, C.byref(count)) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_build_roughness_mips(img, 0, img, 1.0, flags, levels, 16, C.byref(count)) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_mip_coverage_info(img, flags | MIP_COVERAGE, recs, 16, C.byref(count)) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_previews(reqs, 1, flags, out, 148) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_previews_device(reqs, 1, flags, out, 148, None) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_live_graph_buffer_previews(None, None, None, reqs, 1, flags, out, 148) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_from_bc(out, 148, 8, 8, 1, flags, C.byref(res), None) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_from_bc_device(C.byref(d1), flags, None, C.byref(res), None) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_read_dds(b"nowhere.dds", 0, flags, C.byref(res), None) == KC_ERR_UNSUPPORTED, flags
    assert L.kc_dds_header(64, 64, 1, BC_SRGB, 7, out, None) == 0


# ------------------------------------------------------------------ quality, on the reference alone
def cutout(size=64, ref=128):
    """Smooth colour under a soft-edged disk of alpha; magenta wherever the alpha test fails"""
    y, x = np.mgrid[0:size, 0:size].astype(np.float64) / (size - 1)
    rgb = np.stack([0.2 + 0.6 * x, 0.3 + 0.5 * y, 0.7 - 0.4 * x * y], -1)
    r = np.hypot(x - 0.5, y - 0.5)
    alpha = np.clip((0.38 - r) / 0.1 + 0.5, 0.0, 1.0)
    px = np.floor(np.concatenate([rgb, alpha[..., None]], -1) * 255.0 + 0.5).astype(np.uint8)
    px[px[..., 3] < ref, :3] = (255, 0, 255)
    return px


def test_the_rule_beats_plain_bc1_on_the_visible_pixels_of_a_cutout():
    ref, px = 128, cutout()
    h, w = px.shape[:2]
    assert min(R.class_counts(px, ref)) > 0
    op = px[..., 3] >= ref
    src = px[..., :3].astype(np.int64)
    sse = lambda dec: int((((dec[..., :3].astype(np.int64) - src) ** 2) * op[..., None]).sum())
    punch = sse(R.decode(R.encode(px, ref), h, w))
    plain = sse(bc_ref.unblock(bc_ref.decode_bc1(bc_ref.encode(px, 1)), h, w))
    assert punch <= plain, (punch, plain)
    # and not by a hair: the magenta drags plain BC1's endpoints away from every block on the disk's edge
    psnr = lambda s: 10 * np.log10(255.0 ** 2 * 3 * op.sum() / s)
    assert psnr(punch) > psnr(plain) + 1.0, (psnr(punch), psnr(plain))
