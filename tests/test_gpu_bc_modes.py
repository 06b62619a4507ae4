"""Every BC7 and BC6H mode on the device (KC_BC_ALL_MODES; csrc/bc_modes.*): with the flag the pixels of kc_image_from_bc,
kc_image_from_bc_device and kc_image_read_dds and the record of kc_image_bc_compare are bc_modes_ref's, bit for bit, for blocks
that walk every (mode, partition) pair; without it the same calls still give bc_decode_ref's and bc6h_ref's pixels and counts.
Sizes: (96, 80) holds a whole cycle of either format; (97, 83) is 25 x 21 blocks with width % 4 = 1 and height % 4 = 3, edge
blocks on both sides; (4, 4), (1, 1) and (5, 3) are single blocks and clipping on each axis."""
import numpy as np
import pytest

import bc6h_ref
import bc_decode_ref as R
import bc_modes_ref as M
from util import SEED_A, synthetic_rgba, with_edge_cases

pytestmark = pytest.mark.gpu

BC7, BC6H = M.BC7, M.BC6H
SHAPES = [(96, 80), (97, 83), (4, 4), (1, 1), (5, 3)]  # (w, h)


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    return kc


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def edge_rgba(h, w, seed=SEED_A):
    """f32 planes with out-of-range values, infinities and NaN"""
    return [with_edge_cases(p * 1.2 - 0.1, shift=c) for c, p in enumerate(synthetic_rgba(seed, h, w))]


def hdr_rgba(h, w, seed=SEED_A):
    """the same spread over the halves' range"""
    return [with_edge_cases((p * 1.2 - 0.1) * 40.0, shift=c) for c, p in enumerate(synthetic_rgba(seed, h, w))]


def check_bc7(img, want):
    got = img.to_u8()
    bad = np.argwhere((got != want).any(-1))
    assert bad.size == 0, "%d pixels differ, first %s: %s vs %s" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def check_bc6h(img, want):
    assert img.is_rgba()
    for c, (p, q) in enumerate(zip(img.planes(), want)):
        assert p.dtype == np.float32 and np.array_equal(p, q), c


def check(img, blk, fmt, h, w):
    if fmt == BC7:
        check_bc7(img, M.decode(blk, BC7, h, w))
    else:
        check_bc6h(img, M.decode_planes(blk, h, w))


def record(e):
    return dict(format=e.format, channel_mask=e.channel_mask, pixels=e.pixels, sse=[int(v) for v in e.sse], max_abs=[int(v) for v in e.max_abs],
                undecoded_blocks=e.undecoded_blocks, bc7_mode_blocks=[int(v) for v in e.bc7_mode_blocks])


def source(kc, fmt, h, w):
    """an image and what bc_modes_ref.error_record takes for it"""
    img = kc.SlotImage.from_planes(edge_rgba(h, w) if fmt == BC7 else hdr_rgba(h, w)).materialize()
    return img, (img.to_u8() if fmt == BC7 else img.planes())


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("fmt", [BC7, BC6H])
def test_every_mode_decodes_with_the_flag_and_the_default_is_untouched(kc, fmt, w, h):
    blk = M.random_image_blocks(fmt, h, w)
    if (w, h) == (96, 80):
        assert set(M.pairs(blk, fmt)) == set(M.BC7_CYCLE if fmt == BC7 else M.BC6H_CYCLE)
    img, n = kc.SlotImage.from_bc(blk, w, h, fmt, return_undecoded=True, all_modes=True)
    assert n == 0
    check(img, blk, fmt, h, w)
    check(kc.SlotImage.from_bc(blk, w, h, fmt, all_modes=True), blk, fmt, h, w)
    # the same call without the flag: the single-subset decoders and their counts
    img, n = kc.SlotImage.from_bc(blk, w, h, fmt, return_undecoded=True)
    if fmt == BC7:
        want, undecoded = R.decode(blk, BC7, h, w)
        check_bc7(img, want)
    else:
        undecoded = bc6h_ref.decode(blk, h, w)[2]
        check_bc6h(img, bc6h_ref.decode_planes(blk, h, w))
    assert n == undecoded > 0  # even the single block of the smallest sizes is of a partitioned mode: the cycles begin with them


@pytest.mark.parametrize("fmt", [1, 3, 4, 5])
def test_the_flag_changes_nothing_for_the_formats_without_modes(kc, fmt):
    w, h = 37, 22
    blk = R.random_image_blocks(fmt, h, w)
    want = R.decode(blk, fmt, h, w)[0]
    img, n = kc.SlotImage.from_bc(blk, w, h, fmt, return_undecoded=True, all_modes=True)
    assert n == 0 and np.array_equal(img.to_u8(), want)
    if fmt == 4:
        gray = kc.SlotImage.from_bc(blk, w, h, 4, gray=True, all_modes=True)
        assert not gray.is_rgba() and np.array_equal(gray.to_u8()[..., 0], want[..., 0])


@pytest.mark.parametrize("fmt", [BC7, BC6H])
def test_device_form_behind_a_row_pitch(kc, torch, fmt):
    w, h = 130, 67
    blk = M.random_image_blocks(fmt, h, w)
    by, bx, bb = blk.shape
    fill = np.random.default_rng(17).integers(0, 256, (by + 2, bx + 3, bb), dtype=np.uint8)  # junk in the padding
    fill[1:1 + by, 2:2 + bx] = blk
    big = torch.from_numpy(fill).cuda()
    img, n = kc.SlotImage.from_bc_torch(big[1:1 + by, 2:2 + bx, :], w, h, fmt, return_undecoded=True, all_modes=True)
    assert n == 0
    check(img, blk, fmt, h, w)
    assert np.array_equal(big.cpu().numpy(), fill)  # the caller's blocks are read, never written


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("fmt,srgb", [(BC7, False), (BC7, True), (BC6H, False)])
def test_compare_with_the_flag_equals_the_reference_record(kc, torch, fmt, srgb, w, h):
    img = kc.SlotImage.from_planes(edge_rgba(h, w) if fmt == BC7 else hdr_rgba(h, w)).materialize()
    src = img.to_u8(srgb) if fmt == BC7 else img.planes()
    blk = M.random_image_blocks(fmt, h, w, seed=5)
    by, bx, bb = blk.shape
    big = torch.full((by + 1, bx + 2, bb), 0x5a, dtype=torch.uint8, device="cuda")
    big[:by, 1:1 + bx] = torch.from_numpy(blk).cuda()
    e = img.bc_error(fmt, srgb, blocks=big[:by, 1:1 + bx, :], all_modes=True)
    want = M.error_record(src, blk, fmt)
    assert record(e) == want
    assert e.undecoded_blocks == 0 and e.flags == M.BC_ALL_MODES | (R.BC_SRGB if srgb else 0)
    if fmt == BC7:
        assert int(e.bc7_mode_blocks.sum()) == sum(m != 8 for m, _ in M.pairs(blk, BC7))
    # the library's own blocks: the same record with and without the flag
    own = img.to_bc_torch(fmt, srgb)
    plain = img.bc_error(fmt, srgb, blocks=own)
    assert record(img.bc_error(fmt, srgb, blocks=own, all_modes=True)) == record(plain) and plain.undecoded_blocks == 0
    with pytest.raises(ValueError):
        img.bc_error(fmt, srgb, all_modes=True)


@pytest.mark.parametrize("fmt,srgb", [(BC7, False), (BC7, True), (BC6H, False)])
def test_nontemporal_instantiations_and_grid_stride_loops(kc, torch, fmt, srgb):
    """With a cache budget of 0 nothing fits and the kernels take their nontemporal forms; with a grid cap of 2 workgroups a
    thread of the 33 x 17 block image takes two blocks, edge blocks in the later round among them."""
    w, h = 130, 67
    img = kc.SlotImage.from_planes(edge_rgba(h, w) if fmt == BC7 else hdr_rgba(h, w)).materialize()
    src = img.to_u8(srgb) if fmt == BC7 else img.planes()
    blk = M.random_image_blocks(fmt, h, w, seed=9)
    t = torch.from_numpy(blk).cuda()
    want_rec = M.error_record(src, blk, fmt)
    for option, value in (("cache_budget_mb", 0), ("tune_cap", 2)):
        saved = kc.get_option(option)
        kc.set_option(option, value)
        try:
            got, n = kc.SlotImage.from_bc(blk, w, h, fmt, return_undecoded=True, all_modes=True)
            e = img.bc_error(fmt, srgb, blocks=t, all_modes=True)
        finally:
            kc.set_option(option, saved)
        assert n == 0, option
        check(got, blk, fmt, h, w)
        assert record(e) == want_rec, option


def test_a_dds_file_of_every_mode_reads_back_level_by_level(kc, tmp_path):
    w, h = 96, 80
    levels = kc.mip_level_count(w, h)
    sizes = [(max(1, w >> k), max(1, h >> k)) for k in range(levels)]
    blocks = [M.random_image_blocks(BC7, H, W, seed=k) for k, (W, H) in enumerate(sizes)]
    path = tmp_path / "foreign.dds"
    path.write_bytes(kc.dds_header(w, h, BC7, False, levels) + b"".join(b.tobytes() for b in blocks))
    for k in (0, 1, 3, levels - 1):
        W, H = sizes[k]
        got, info = kc.SlotImage.read_dds(path, level=k, return_info=True, all_modes=True)
        assert (info.width, info.height, info.format, info.levels) == (w, h, BC7, levels)
        assert (got.size().width, got.size().height) == (W, H)
        check_bc7(got, M.decode(blocks[k], BC7, H, W))
    # without the flag level 0 has holes: the default decoder's pixels
    check_bc7(kc.SlotImage.read_dds(path), R.decode(blocks[0], BC7, h, w)[0])


def test_launches_and_algorithmic_bytes(kc, torch):
    w, h = 42, 30
    bx, by = (w + 3) // 4, (h + 3) // 4
    nblk = bx * by * 16

    def delta(call):
        st0 = kc.stats()
        call()
        st1 = kc.stats()
        return st1["kernel_launches"] - st0["kernel_launches"], st1["algorithmic_bytes"] - st0["algorithmic_bytes"]

    for fmt, planes, read in ((BC7, 4, 4), (BC6H, 3, 3)):
        blk = M.random_image_blocks(fmt, h, w)
        img = source(kc, fmt, h, w)[0]
        t = torch.from_numpy(blk).cuda()
        # one launch under the flag, where the counted form takes two
        assert delta(lambda: kc.SlotImage.from_bc(blk, w, h, fmt, all_modes=True)) == (1, nblk + 4 * w * h * planes)
        assert delta(lambda: kc.SlotImage.from_bc(blk, w, h, fmt, return_undecoded=True, all_modes=True)) == (1, nblk + 4 * w * h * planes)
        assert delta(lambda: kc.SlotImage.from_bc(blk, w, h, fmt, return_undecoded=True)) == (2, nblk + 4 * w * h * planes)
        assert delta(lambda: img.bc_error(fmt, blocks=t, all_modes=True)) == (2, nblk + 4 * w * h * read)


def test_a_refused_call_launches_nothing(kc):
    w, h = 12, 8
    img = kc.SlotImage.from_planes(edge_rgba(h, w)).materialize()
    blk = M.random_image_blocks(BC7, h, w)
    from kanter_core_amd import _lib
    import ctypes as C
    L = _lib.load()
    err = _lib.kc_bc_error()
    out = (C.c_uint8 * blk.nbytes)()
    before = kc.stats()
    with pytest.raises(kc.TexProError):
        kc.SlotImage.from_bc(blk, w, h, BC7, gray=True, all_modes=True)    # KC_BC_GRAY is for BC4, with the flag too
    with pytest.raises(kc.TexProError):
        kc.SlotImage.from_bc(blk[:1], w, h, BC7, all_modes=True)            # fewer bytes than the blocks
    with pytest.raises(ValueError):
        img.bc_error(BC7, all_modes=True)                                   # the library's own blocks need no flag
    assert L.kc_image_bc_error(img._h, BC7, M.BC_ALL_MODES, C.byref(err)) == R.KC_ERR_UNSUPPORTED
    assert L.kc_image_to_bc(img._h, BC7, M.BC_ALL_MODES, out, blk.nbytes) == R.KC_ERR_UNSUPPORTED
    after = kc.stats()
    assert after["kernel_launches"] == before["kernel_launches"] and after["algorithmic_bytes"] == before["algorithmic_bytes"]
