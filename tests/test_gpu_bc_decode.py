"""Block decode and the error of an encoding on the device (kc_image_from_bc, kc_image_from_bc_device, kc_image_bc_compare,
kc_image_bc_error, kc_image_read_dds; csrc/bc_decode.*): the pixels are bc_decode_ref's, byte for byte and as f32 planes, for
random blocks of every format at the sizes where the kernels can go wrong -- (1, 1) a single edge block, (5, 3) / (7, 9)
clipping on each axis and on both, (130, 67) an odd plane pitch, (1028, 16) 257 blocks in a row: more than one workgroup and a
wave that straddles the end of a block row; the device form ignores the padding between block rows and is ordered on torch's
stream; encode -> decode round trips equal the references'; the error record is the reference's, integer for integer; .dds
files read back level by level; kc_stats counts what the header documents and refusals launch nothing."""
import ctypes as C
import os

import numpy as np
import pytest

import bc7_ref
import bc_decode_ref as R
import bc_ref
from pngio import read_png
from util import SEED_A, synthetic_rgba, with_edge_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
BC7 = R.BC7
SHAPES = [(1, 1), (4, 4), (5, 3), (7, 9), (64, 64), (130, 67), (1028, 16)]  # (w, h)
FORMS = [(1, False), (1, True), (3, False), (3, True), (4, False), (5, False), (BC7, False), (BC7, True)]
PLANES = {1: 4, 3: 4, 4: 1, 5: 2, BC7: 4}  # resident planes a decode writes


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    return kc


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def ref_encode(rgba8, fmt):
    return bc7_ref.encode(rgba8) if fmt == BC7 else bc_ref.encode(rgba8, fmt)


def edge_rgba(h, w, seed=SEED_A):
    """f32 planes with out-of-range values, infinities and NaN"""
    return [with_edge_cases(p * 1.2 - 0.1, shift=c) for c, p in enumerate(synthetic_rgba(seed, h, w))]


def check_decoded(img, want, rgba=True):
    """to_u8(0) is the decoded bytes; the planes are bytes / 255 in f32"""
    assert img.is_rgba() == rgba
    got = img.to_u8()
    if not rgba:  # Gray exports as (v, v, v, 255)
        want = np.concatenate([np.repeat(want[..., :1], 3, -1), np.full_like(want[..., :1], 255)], -1)
    bad = np.argwhere((got != want).any(-1))
    assert bad.size == 0, "%d pixels differ, first %s: %s vs %s" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    for c, p in enumerate(img.planes()):
        assert p.dtype == np.float32 and np.array_equal(p, want[..., c].astype(np.float32) / np.float32(255.0)), c


def record(e):
    """BcError -> the dict bc_decode_ref.error_record returns"""
    return dict(format=e.format, channel_mask=e.channel_mask, pixels=e.pixels, sse=[int(v) for v in e.sse], max_abs=[int(v) for v in e.max_abs],
                undecoded_blocks=e.undecoded_blocks, bc7_mode_blocks=[int(v) for v in e.bc7_mode_blocks])


# ------------------------------------------------------------------ decode from host blocks
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_random_blocks_decode_to_the_reference(kc, fmt, w, h):
    blk = R.random_image_blocks(fmt, h, w)
    want, undecoded = R.decode(blk, fmt, h, w)
    img, n = kc.SlotImage.from_bc(blk, w, h, fmt, return_undecoded=True)
    assert n == undecoded and (undecoded > 0) == (fmt == BC7 and w * h >= 64 * 64)
    check_decoded(img, want)
    check_decoded(kc.SlotImage.from_bc(blk, w, h, fmt), want)  # without the count: the other BC7 instantiation
    if fmt == 4:
        check_decoded(kc.SlotImage.from_bc(blk, w, h, 4, gray=True), want, rgba=False)


@pytest.mark.parametrize("fmt,consts", [(4, {1: 0.0, 2: 0.0, 3: 1.0}), (5, {2: 0.0, 3: 1.0}), (1, {}), (BC7, {})])
def test_planes_a_format_does_not_hold_are_constants(kc, fmt, consts):
    from kanter_core_amd import _lib
    L = _lib.load()
    img = kc.SlotImage.from_bc(R.random_image_blocks(fmt, 9, 7), 7, 9, fmt)
    for c, p in enumerate(img.plane_handles()):
        is_const, v = C.c_int(), C.c_float()
        assert L.kc_plane_is_const(p, C.byref(is_const), C.byref(v)) == 0
        assert bool(is_const.value) == (c in consts), (fmt, c)
        if c in consts:
            assert v.value == consts[c]


# ------------------------------------------------------------------ decode from device blocks
@pytest.mark.parametrize("w,h", [(5, 3), (130, 67), (1028, 16)])
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_device_form_ignores_the_padding_between_block_rows(kc, torch, fmt, w, h):
    blk = R.random_image_blocks(fmt, h, w)
    by, bx, bb = blk.shape
    want, undecoded = R.decode(blk, fmt, h, w)
    rng = np.random.default_rng(17)
    for poison in (0x00, 0xff, None):  # whatever lies between the block rows, the pixels are the same
        fill = rng.integers(0, 256, (by + 2, bx + 3, bb), dtype=np.uint8) if poison is None else np.full((by + 2, bx + 3, bb), poison, np.uint8)
        fill[1:1 + by, 2:2 + bx] = blk
        big = torch.from_numpy(fill).cuda()
        img, n = kc.SlotImage.from_bc_torch(big[1:1 + by, 2:2 + bx, :], w, h, fmt, return_undecoded=True)
        assert n == undecoded
        check_decoded(img, want)
    assert np.array_equal(big.cpu().numpy(), fill)  # the caller's blocks are read, never written
    del big  # nothing aliases the caller's memory: the image outlives it
    check_decoded(img, want)


@pytest.mark.parametrize("which", ["side stream", "default stream"])
def test_stream_ordering_without_sync(kc, torch, which):
    w, h = 1024, 512
    blk = R.random_image_blocks(BC7, h, w)
    host = torch.from_numpy(blk).pin_memory()
    s = torch.cuda.Stream() if which == "side stream" else torch.cuda.default_stream()
    with torch.cuda.stream(s):
        t = torch.zeros(blk.shape, dtype=torch.uint8, device="cuda")
        torch.cuda._sleep(20_000_000)  # the producer is late: the library's stream must wait for it
        t.copy_(host, non_blocking=True)
        img = kc.SlotImage.from_bc_torch(t, w, h, BC7)
        t.zero_()  # and torch may overwrite the blocks as soon as the call has returned
    want = R.decode(blk, BC7, h, w)[0]
    assert np.array_equal(img.to_u8(), want)


# ------------------------------------------------------------------ round trip
@pytest.fixture(scope="module")
def sources(kc):
    """name -> image: the golden inputs and one f32 image with out-of-range values and NaN; read by several tests, never changed"""
    out = {n: kc.SlotImage.from_u8(read_png(os.path.join(INPUTS, n))) for n in ("clouds.png", "image_1.png", "heart_110.png")}
    out["edge f32"] = kc.SlotImage.from_planes(edge_rgba(67, 130))
    return out


@pytest.mark.parametrize("fmt,srgb", FORMS)
@pytest.mark.parametrize("name", ["clouds.png", "heart_110.png", "edge f32"])
def test_round_trip_equals_the_references(kc, sources, name, fmt, srgb):
    img = sources[name]
    s = img.size()
    want, undecoded = R.decode(ref_encode(img.to_u8(srgb), fmt), fmt, s.height, s.width)
    got, n = kc.SlotImage.from_bc(img.to_bc(fmt, srgb), s.width, s.height, fmt, return_undecoded=True)
    assert n == undecoded == 0
    check_decoded(got, want)


# ------------------------------------------------------------------ the error of an encoding
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("fmt,srgb", FORMS)
def test_bc_error_equals_the_reference_record(kc, torch, fmt, srgb, w, h):
    img = kc.SlotImage.from_planes(edge_rgba(h, w))
    src = img.to_u8(srgb)
    e = img.bc_error(fmt, srgb)
    assert record(e) == R.error_record(src, ref_encode(src, fmt), fmt)
    assert e.flags == (R.BC_SRGB if srgb else 0) and e.undecoded_blocks == 0
    assert record(img.bc_error(fmt, srgb, blocks=img.to_bc_torch(fmt, srgb))) == record(e)
    # other blocks than the image's own: random ones, undecoded BC7 modes among them, behind a row pitch
    blk = R.random_image_blocks(fmt, h, w, seed=5)
    by, bx, bb = blk.shape
    big = torch.full((by + 1, bx + 2, bb), 0x5a, dtype=torch.uint8, device="cuda")
    big[:by, 1:1 + bx] = torch.from_numpy(blk).cuda()
    other = img.bc_error(fmt, srgb, blocks=big[:by, 1:1 + bx, :])
    assert record(other) == R.error_record(src, blk, fmt)
    assert other.psnr() == pytest.approx(R.psnr(record(other)), rel=1e-12)


def test_gray_and_constant_images(kc):
    w, h = 30, 21
    gray = kc.SlotImage.from_planes([edge_rgba(h, w)[1]])
    const = kc.SlotImage.from_value(kc.Size(w, h), 0.3, True)
    blocks = ((w + 3) // 4) * ((h + 3) // 4)
    for fmt, srgb in FORMS:
        for img in (gray, const):
            src = img.to_u8(srgb)
            assert record(img.bc_error(fmt, srgb)) == R.error_record(src, ref_encode(src, fmt), fmt), (fmt, srgb)
        # a constant image: no plane is read, by the encoder or by the comparison
        st0 = kc.stats()
        const.bc_error(fmt, srgb)
        st1 = kc.stats()
        assert st1["kernel_launches"] - st0["kernel_launches"] == 3
        assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == 2 * blocks * R.BLOCK_BYTES[fmt]


@pytest.mark.parametrize("name", ["clouds.png", "image_1.png"])
def test_bc7_is_closer_than_bc1(kc, sources, name):
    img = sources[name]
    e1, e7 = img.bc_error(1), img.bc_error(BC7)
    assert sum(int(v) for v in e7.sse[:3]) < sum(int(v) for v in e1.sse[:3])
    assert e7.psnr(channels=(0, 1, 2)) > e1.psnr()
    src = img.to_u8()
    for e, fmt in ((e1, 1), (e7, BC7)):
        want = R.error_record(src, ref_encode(src, fmt), fmt)
        assert record(e) == want
        assert e.psnr() == pytest.approx(R.psnr(want), rel=1e-12)
        assert e.psnr(channels=[1]) == pytest.approx(R.psnr(want, channels=[1]), rel=1e-12)
    assert int(e7.bc7_mode_blocks.sum()) == 64 * 64 == int(e7.bc7_mode_blocks[5] + e7.bc7_mode_blocks[6])


def test_psnr_of_an_exact_encoding_is_infinite(kc):
    img = kc.SlotImage.from_value(kc.Size(8, 8), 1.0, True)
    e = img.bc_error(BC7)
    assert [int(v) for v in e.sse] == [0, 0, 0, 0] and e.psnr() == float("inf")
    with pytest.raises(ValueError):
        img.bc_error(1).psnr(channels=[3])  # BC1's alpha is outside the mask


# ------------------------------------------------------------------ the other instantiations and the grid-stride loops
@pytest.mark.parametrize("fmt,srgb", FORMS)
def test_nontemporal_instantiations_and_grid_stride_loops(kc, fmt, srgb):
    """With a cache budget of 0 nothing fits and both kernels take their nontemporal forms; with a grid cap of 2 workgroups a
    thread of the 33 x 17 block image takes two blocks, edge blocks in the later round among them."""
    w, h = 130, 67
    img = kc.SlotImage.from_planes(edge_rgba(h, w)).materialize()
    src = img.to_u8(srgb)
    blk = R.random_image_blocks(fmt, h, w, seed=9)
    want_px, want_n = R.decode(blk, fmt, h, w)
    want_rec = R.error_record(src, ref_encode(src, fmt), fmt)
    for option, value in (("cache_budget_mb", 0), ("tune_cap", 2)):
        saved = kc.get_option(option)
        kc.set_option(option, value)
        try:
            got, n = kc.SlotImage.from_bc(blk, w, h, fmt, return_undecoded=True)
            plain = kc.SlotImage.from_bc(blk, w, h, fmt)
            e = img.bc_error(fmt, srgb)
        finally:
            kc.set_option(option, saved)
        assert n == want_n, option
        check_decoded(got, want_px)
        check_decoded(plain, want_px)
        assert record(e) == want_rec, option


# ------------------------------------------------------------------ DDS and the live graph
@pytest.mark.parametrize("fmt,srgb", FORMS)
def test_dds_files_read_back_level_by_level(kc, tmp_path, fmt, srgb):
    img = kc.SlotImage.from_planes(edge_rgba(67, 130))
    path = tmp_path / "t.dds"
    img.write_dds(path, fmt, srgb, mips=True)
    levels = img.to_bc_mips(fmt, srgb)
    assert len(levels) == 8
    for k in (0, 3, 7):
        W, H = max(1, 130 >> k), max(1, 67 >> k)
        got, info = kc.SlotImage.read_dds(path, level=k, return_info=True)
        assert info == kc.DdsInfo(130, 67, fmt, srgb, 8, 148, os.path.getsize(path) - 148)
        assert (got.size().width, got.size().height) == (W, H)
        check_decoded(got, R.decode(levels[k], fmt, H, W)[0])
    assert kc.dds_parse(path.read_bytes()) == info
    if fmt == 4:
        check_decoded(kc.SlotImage.read_dds(path, level=1, gray=True), R.decode(levels[1], 4, 33, 65)[0], rgba=False)
    with pytest.raises(kc.TexProError):
        kc.SlotImage.read_dds(path, level=8)
    img.write_dds(path, fmt, srgb, mips=False)
    got, info = kc.SlotImage.read_dds(path, return_info=True)
    assert info.levels == 1
    check_decoded(got, R.decode(levels[0], fmt, 67, 130)[0])


def test_live_graph_buffer_bc_error(kc):
    tp = kc.TextureProcessor.new()
    lg = tp.new_live_graph()
    path = os.path.join(INPUTS, "heart_110.png")
    src = lg.add_node(kc.Node.new(kc.NodeType.Image(path)))
    lg.await_clean(src)
    img = kc.SlotImage.read_png(path)
    for fmt, srgb in FORMS:
        assert record(lg.buffer_bc_error(src, 0, fmt, srgb)) == record(img.bc_error(fmt, srgb))
    with pytest.raises(kc.TexProError):
        lg.buffer_bc_error(src, 5, BC7)  # no such slot


# ------------------------------------------------------------------ accounting
def test_launches_and_algorithmic_bytes(kc, torch):
    w, h = 42, 30
    bx, by = (w + 3) // 4, (h + 3) // 4
    rgba = kc.SlotImage.from_planes(edge_rgba(h, w)).materialize()
    gray = kc.SlotImage.from_planes([edge_rgba(h, w)[0]]).materialize()

    def delta(call):
        st0 = kc.stats()
        call()
        st1 = kc.stats()
        return st1["kernel_launches"] - st0["kernel_launches"], st1["algorithmic_bytes"] - st0["algorithmic_bytes"]

    for fmt in R.FORMATS:
        blk = R.random_image_blocks(fmt, h, w)
        nblk = bx * by * R.BLOCK_BYTES[fmt]
        # decode: the blocks plus 4 w h per resident plane written; BC7's count is a second launch
        assert delta(lambda: kc.SlotImage.from_bc(blk, w, h, fmt)) == (1, nblk + 4 * w * h * PLANES[fmt])
        assert delta(lambda: kc.SlotImage.from_bc(blk, w, h, fmt, return_undecoded=True)) == (2 if fmt == BC7 else 1, nblk + 4 * w * h * PLANES[fmt])
        if fmt == 4:
            assert delta(lambda: kc.SlotImage.from_bc(blk, w, h, fmt, gray=True)) == (1, nblk + 4 * w * h)
        # compare: the planes the format reads plus the blocks; bc_error: the encoder's launch and bytes first
        t = torch.from_numpy(blk).cuda()
        read = {1: 3, 3: 4, 4: 1, 5: 2, BC7: 4}[fmt]
        assert delta(lambda: rgba.bc_error(fmt, blocks=t)) == (2, nblk + 4 * w * h * read)
        assert delta(lambda: rgba.bc_error(fmt)) == (3, 2 * (nblk + 4 * w * h * read))
        assert delta(lambda: gray.bc_error(fmt)) == (3, 2 * (nblk + 4 * w * h))


def test_a_refused_call_launches_nothing(kc, torch):
    w, h = 12, 8
    img = kc.SlotImage.from_planes(edge_rgba(h, w)).materialize()
    blk = R.random_image_blocks(1, h, w)
    t = torch.from_numpy(blk).cuda()
    before = kc.stats()
    with pytest.raises(kc.TexProError):
        kc.SlotImage.from_bc(blk, w, h, 1, gray=True)            # KC_BC_GRAY is for BC4
    with pytest.raises(kc.TexProError):
        kc.SlotImage.from_bc(blk[:1], w, h, 1)                    # fewer bytes than the blocks
    with pytest.raises(kc.TexProError):
        kc.SlotImage.from_bc(blk, 0, h, 1)                        # a zero size
    with pytest.raises(kc.TexProError):
        img.bc_error(4, srgb=True)                                # KC_BC_SRGB with BC4
    with pytest.raises(ValueError):
        img.bc_error(1, blocks=t[:1])                             # not the image's block grid
    from kanter_core_amd import _lib
    big = torch.zeros((2, 4, 8), dtype=torch.uint8, device="cuda")
    d = _lib.kc_bc_image(big.data_ptr(), w + 4, h, 1, big.stride(0))  # a valid descriptor, but not of the image's size
    err = _lib.kc_bc_error()
    assert _lib.load().kc_image_bc_compare(img._h, C.byref(d), 0, C.byref(err)) == R.KC_ERR_INVALID_ARG
    after = kc.stats()
    assert after["kernel_launches"] == before["kernel_launches"] and after["algorithmic_bytes"] == before["algorithmic_bytes"]
