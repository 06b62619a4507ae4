"""Every BC7 and BC6H mode without a device: what the random blocks of bc_modes_ref cover, the numpy reference of the all-modes
contract (tests/bc_modes_ref.py) against Pillow's decoders block by block, the partition tables probed through Pillow
independently of the reference's decode path, the all-modes record against bc_decode_ref's and bc6h_ref's on the library's own
kind of blocks, and the argument checks of KC_BC_ALL_MODES before kc_init."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import bc6h_ref
import bc7_ref
import bc_decode_ref as R
import bc_modes_ref as M
from pngio import read_png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
BC7, BC6H = M.BC7, M.BC6H
KC_OK, KC_ERR_NO_DEVICE, KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = R.KC_OK, R.KC_ERR_NO_DEVICE, R.KC_ERR_INVALID_ARG, R.KC_ERR_UNSUPPORTED
ALL = M.BC_ALL_MODES


@pytest.fixture(scope="module")
def L():
    from kanter_core_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ 1. the generator
def test_the_random_blocks_walk_every_mode_and_partition():
    assert len(M.BC7_CYCLE) == 276 == 16 + 4 * 64 + 3 + 1 and len(set(M.BC7_CYCLE)) == 276
    assert len(M.BC6H_CYCLE) == 328 == 10 * 32 + 4 + 4 and len(set(M.BC6H_CYCLE)) == 328
    for fmt, cycle in ((BC7, M.BC7_CYCLE), (BC6H, M.BC6H_CYCLE)):
        blk = M.random_blocks(fmt, 2 * len(cycle), seed=1)
        assert M.pairs(blk, fmt) == cycle + cycle                      # what was asked for is what the blocks say
        assert len({b.tobytes() for b in blk}) == len(blk)            # and the other bits are random
        image = M.random_image_blocks(fmt, 80, 96)                    # 24 x 20 = 480 blocks: a whole cycle of either format
        assert image.shape == (20, 24, 16) and set(M.pairs(image, fmt)) == set(cycle)
    modes = [m for m, _ in M.BC7_CYCLE]
    assert [modes.count(m) for m in range(9)] == [16, 64, 64, 64, 1, 1, 1, 64, 1]
    modes = [m for m, _ in M.BC6H_CYCLE]
    assert [modes.count(m) for m in range(1, 15)] == [32] * 10 + [1] * 4 and sorted(m for m in modes if m < 0) == [-31, -27, -23, -19]


def test_the_bc6h_layouts_fill_the_header_exactly_once():
    for mode, (nb, delta, _) in M.BC6H_TWO.items():
        have = {}
        for name, lo, cnt, at in M.bc6h_fields(mode):
            for k in range(cnt):
                assert (name, lo + k) not in have
                have[(name, lo + k)] = at + k
        assert sorted(have.values()) == list(range(82))
        for c, ch in enumerate("rgb"):
            assert sorted(b for (n, b) in have if n == ch + "0") == list(range(nb))
            for e in "123":
                assert sorted(b for (n, b) in have if n == ch + e) == list(range(delta[c] or nb))
        assert sorted(b for (n, b) in have if n == "d") == list(range(5))


# ------------------------------------------------------------------ 2. the reference against Pillow
def pillow_decode(blk, fmt):
    """n blocks as an image one block high -> Pillow's pixels (4, 4 n, channels)"""
    Image = pytest.importorskip("PIL.Image")
    from kanter_core_amd import api
    blk = np.ascontiguousarray(blk, np.uint8).reshape(-1, 16)
    data = api.dds_header(4 * len(blk), 4, fmt, levels=1) + blk.tobytes()
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im)


def per_block(px):
    """(4, 4 n, c) -> (n, 16, c), texel t = 4 y + x"""
    return px.reshape(4, -1, 4, px.shape[-1]).transpose(1, 0, 2, 3).reshape(-1, 16, px.shape[-1])


def test_bc7_reference_equals_pillow_on_every_mode_and_partition():
    """Byte equality on every block of three cycles.  The one place where Pillow and the format definition part is the reserved
    block (byte 0 == 0): the definition returns (0, 0, 0, 0), Pillow 12 (0, 0, 0, 255).  The definition wins (the header has
    said so since the single-subset decoder); for those blocks R, G and B are compared and Pillow's alpha is asserted to be 255."""
    pytest.importorskip("PIL")
    blk = M.random_blocks(BC7, 3 * 276, seed=3)
    want = per_block(pillow_decode(blk, BC7)).astype(np.int64)
    got, mode = M.decode_bc7(blk)
    assert set(M.pairs(blk, BC7)) == set(M.BC7_CYCLE)
    reserved = mode == 8
    assert reserved.sum() == 3 and (got[reserved] == 0).all() and (want[reserved][..., :3] == 0).all() and (want[reserved][..., 3] == 255).all()
    bad = np.nonzero((got != want).any((1, 2)) & ~reserved)[0]
    assert bad.size == 0, [M.pairs(blk, BC7)[i] for i in bad[:8]]
    assert (got[np.isin(mode, (0, 1, 2, 3))][..., 3] == 255).all()


def test_bc6h_reference_equals_pillow_on_every_mode_and_partition():
    """Pillow shows a half v as floor(255 clamp(v, 0, 1)) and leaves out interp's + 32 (bc6h_ref's docstring), so byte equality
    is asked of round_term = 0; with the contract's + 32 the bytes are within 1 and under 1 % of them differ.  Every second
    cycle has endpoint 0 in the lower half of its range, so that more than half of the texels lie inside [0, 1] where Pillow's
    bytes can tell patterns apart."""
    pytest.importorskip("PIL")
    blk = M.random_blocks(BC6H, 4 * 328, seed=2)
    low = (np.arange(len(blk)) // 328) % 2 == 1  # the second and the fourth cycle: both halves see every pair
    blk[low] = M.low_endpoint0(blk[low])
    pairs = M.pairs(blk, BC6H)
    assert {p for p, k in zip(pairs, low) if k} == {p for p, k in zip(pairs, low) if not k} == set(M.BC6H_CYCLE)
    px = pillow_decode(blk, BC6H)
    assert px.shape[-1] == 3
    want = per_block(px)
    t0, mode = M.decode_bc6h(blk, round_term=0)
    two = (mode >= 1) & (mode <= 10)
    assert (bc6h_ref.half_value(t0[two]) <= 1.0).mean() > 0.5
    got = bc6h_ref.pillow_bytes(t0)
    bad = np.nonzero((got != want).any((1, 2)))[0]
    assert bad.size == 0, [pairs[i] for i in bad[:8]]
    d = np.abs(bc6h_ref.pillow_bytes(M.decode_bc6h(blk)[0]).astype(np.int64) - want)
    assert d.max() <= 1 and (d != 0).mean() < 0.01


# ------------------------------------------------------------------ 3. the partition tables, probed
def bc7_probe(mode, part, ones):
    """A block of `mode` (1: two subsets, 2: three) and partition `part` whose indices are all 0 and whose endpoints are all
    zero bits, except the endpoints of the subsets in `ones`, which are all one bits: texel t decodes to endpoint 0 of its subset"""
    ns, pb, _, _, cb, _, _, _, _ = M.BC7_MODES[mode]
    blk = np.zeros((1, 16), np.uint8)
    blk[0, 0] = 1 << mode
    M.set_field(blk, mode + 1, pb, part)
    for c in range(3):
        for s in ones:
            for k in (0, 1):
                M.set_field(blk, mode + 1 + pb + (c * 2 * ns + 2 * s + k) * cb, cb, (1 << cb) - 1)
    return blk[0]


def test_the_two_subset_table_is_what_pillow_decodes():
    pytest.importorskip("PIL")
    px = per_block(pillow_decode(np.stack([bc7_probe(1, p, (1,)) for p in range(64)]), BC7))
    r = px[..., 0].astype(np.int64)
    assert set(np.unique(r)) == {0, 253}  # six one bits above a zero p-bit, the top bit repeated below: 1111110 1
    masks = ((r > 0) << np.arange(16)).sum(-1)
    assert len(set(masks.tolist())) == 64
    assert [hex(v) for v in masks[:4]] == ["0xcccc", "0x8888", "0xeeee", "0xecc8"]
    assert np.array_equal(masks, M.P2)


def test_the_three_subset_table_is_what_pillow_decodes():
    pytest.importorskip("PIL")
    one = per_block(pillow_decode(np.stack([bc7_probe(2, p, (1,)) for p in range(64)]), BC7))[..., 0] > 0
    both = per_block(pillow_decode(np.stack([bc7_probe(2, p, (1, 2)) for p in range(64)]), BC7))[..., 0] > 0
    assert (one <= both).all()
    subset = np.where(one, 1, np.where(both, 2, 0))
    assert np.array_equal((subset << (2 * np.arange(16))).sum(-1), M.P3)
    assert all(set(np.unique(s)) == {0, 1, 2} for s in subset)


def test_bc6h_uses_the_first_32_two_subset_entries():
    """Mode 10 stores plain 6-bit endpoints: those of subset 1 (endpoints 2 and 3 of every channel) all ones, the others 0"""
    pytest.importorskip("PIL")
    fields = M.bc6h_fields(10)
    blocks = []
    for p in range(32):
        blk = np.zeros((1, 16), np.uint8)
        M.set_field(blk, 0, 5, bc6h_ref.FIELD[10])
        for name, lo, cnt, at in fields:
            if name[0] in "rgb" and name[1] in "23":
                M.set_field(blk, at, cnt, (1 << cnt) - 1)
        M.set_field(blk, 77, 5, p)
        blocks.append(blk[0])
    px = per_block(pillow_decode(np.stack(blocks), BC6H))
    masks = ((px[..., 0] > 0) << np.arange(16)).sum(-1)
    assert np.array_equal(masks, M.P2[:32])


def test_the_anchors_lie_in_their_subsets():
    # what else the anchor tables must satisfy is test 2's: a wrong anchor shifts every later index of its block
    assert ((M.P2 & 1) == 0).all() and ((M.P3 & 3) == 0).all()  # texel 0 is subset 0's
    assert (((M.P2 >> M.A2) & 1) == 1).all()
    assert (((M.P3 >> (2 * M.A3_1)) & 3) == 1).all() and (((M.P3 >> (2 * M.A3_2)) & 3) == 2).all()


# ------------------------------------------------------------------ 4. a superset of the single-subset references
def test_the_reference_is_a_superset_of_the_single_subset_ones():
    blk = R.random_blocks(BC7, 96)
    t, mode = R.decode_bc7(blk)
    keep = ~R.undecoded(mode)
    assert keep.sum() >= 70 and np.array_equal(M.decode_bc7(blk)[0][keep], t[keep]) and np.array_equal(M.decode_bc7(blk)[1], mode)
    blk = bc6h_ref.random_blocks(120)
    t, mode = bc6h_ref.decode_blocks(blk)
    keep = ~bc6h_ref.undecoded(mode)
    assert keep.sum() >= 80 and np.array_equal(M.decode_bc6h(blk)[0][keep], t[keep]) and np.array_equal(M.decode_bc6h(blk)[1], mode)


@pytest.mark.parametrize("name", ["heart_110.png", "clouds.png"])
def test_the_record_of_the_librarys_own_blocks_is_the_single_subset_one(name):
    a = R.as_rgba8(read_png(os.path.join(INPUTS, name)))[:40, :52]
    assert M.error_record(a, bc7_ref.encode(a), BC7) == R.error_record(a, bc7_ref.encode(a), BC7)
    planes = [(a[..., c].astype(np.float32) / np.float32(255.0)) * np.float32(8.0) for c in range(3)]
    blk = bc6h_ref.encode(planes)
    assert M.error_record(planes, blk, BC6H) == bc6h_ref.compare(planes, blk)


# ------------------------------------------------------------------ 5. the argument checks
def test_the_flag_is_accepted_where_blocks_are_decoded_and_refused_where_they_are_made(L, tmp_path):
    import torch
    from kanter_core_amd import _lib, api
    gpu = torch.cuda.is_available()  # the not-gpu suite also runs on a machine with a device, initialised or not
    needs_device = (KC_ERR_NO_DEVICE,) if not gpu else (KC_ERR_NO_DEVICE, KC_ERR_INVALID_ARG)
    img = C.c_void_p(1 << 20)  # never looked at: every call below returns before it would be
    out, n = C.c_void_p(), C.c_uint64()
    buf = (C.c_uint8 * 64)()
    err = _lib.kc_bc_error()
    D = _lib.kc_bc_image
    SRGB, GRAY = R.BC_SRGB, R.BC_GRAY
    formats = R.FORMATS + (BC6H,)
    bytes_of = dict(R.BLOCK_BYTES)
    bytes_of[BC6H] = 16
    assert api.BC_ALL_MODES == ALL == 16
    header = open(os.path.join(ROOT, "include", "kanter_core_amd.h")).read()
    assert re.search(r"#define KC_BC_ALL_MODES (\d+)u", header).group(1) == str(api.BC_ALL_MODES)
    d = {f: D(1 << 20, 8, 8, f, 32) for f in formats}
    for fmt in formats:
        need = 4 * bytes_of[fmt]
        # kc_image_from_bc: past the flags, the next errors in the documented order
        assert L.kc_image_from_bc(buf, need - 1, 8, 8, fmt, ALL, C.byref(out), None) == KC_ERR_INVALID_ARG
        assert L.kc_image_from_bc(None, 64, 8, 8, fmt, ALL, C.byref(out), None) == KC_ERR_INVALID_ARG
        assert L.kc_image_from_bc(buf, 64, 0, 8, fmt, ALL, C.byref(out), None) == KC_ERR_INVALID_ARG
        assert L.kc_image_from_bc(buf, 64, 8, 8, fmt, ALL | SRGB, C.byref(out), None) == KC_ERR_UNSUPPORTED
        assert L.kc_image_from_bc(buf, 64, 8, 8, fmt, ALL | 8, C.byref(out), None) == KC_ERR_UNSUPPORTED
        assert L.kc_image_from_bc(buf, need - 1, 8, 8, fmt, ALL | GRAY, C.byref(out), None) == (KC_ERR_INVALID_ARG if fmt == 4 else KC_ERR_UNSUPPORTED)
        if not gpu:
            assert L.kc_image_from_bc(buf, need, 8, 8, fmt, ALL, C.byref(out), C.byref(n)) == KC_ERR_NO_DEVICE
        # kc_image_from_bc_device
        assert L.kc_image_from_bc_device(C.byref(d[fmt]), ALL, None, None, None) == KC_ERR_INVALID_ARG
        assert L.kc_image_from_bc_device(C.byref(D(1 << 20, 8, 8, fmt, 8)), ALL, None, C.byref(out), None) == KC_ERR_INVALID_ARG  # pitch
        assert L.kc_image_from_bc_device(C.byref(d[fmt]), ALL | SRGB, None, C.byref(out), None) == KC_ERR_UNSUPPORTED
        assert L.kc_image_from_bc_device(C.byref(d[fmt]), ALL, None, C.byref(out), C.byref(n)) in needs_device
        # kc_image_bc_compare: with and without KC_BC_SRGB, which keeps its own rule
        assert L.kc_image_bc_compare(None, C.byref(d[fmt]), ALL, C.byref(err)) == KC_ERR_INVALID_ARG
        assert L.kc_image_bc_compare(img, C.byref(d[fmt]), ALL, None) == KC_ERR_INVALID_ARG
        assert L.kc_image_bc_compare(img, C.byref(d[fmt]), ALL | GRAY, C.byref(err)) == KC_ERR_UNSUPPORTED
        assert L.kc_image_bc_compare(None, C.byref(d[fmt]), ALL | SRGB, C.byref(err)) == (KC_ERR_INVALID_ARG if fmt in (1, 3, BC7) else KC_ERR_UNSUPPORTED)
        if not gpu:
            assert L.kc_image_bc_compare(img, C.byref(d[fmt]), ALL, C.byref(err)) == KC_ERR_NO_DEVICE
        # refused where the library's own blocks are made: the encoders' flag rule
        assert L.kc_image_bc_error(img, fmt, ALL, C.byref(err)) == KC_ERR_UNSUPPORTED
        assert L.kc_live_graph_buffer_bc_error(None, 0, 0, fmt, ALL, C.byref(err)) == KC_ERR_UNSUPPORTED
        assert L.kc_image_to_bc(img, fmt, ALL, buf, 64) == KC_ERR_UNSUPPORTED
        assert L.kc_image_to_bc_device(img, C.byref(d[fmt]), ALL, None) == KC_ERR_UNSUPPORTED
        assert L.kc_image_to_bc_mips(img, fmt, ALL, buf, 64) == KC_ERR_UNSUPPORTED
        assert L.kc_image_to_bc_mips_device(img, fmt, ALL, buf, 64, None) == KC_ERR_UNSUPPORTED
        assert L.kc_image_write_dds(img, str(tmp_path / "x.dds").encode(), fmt, ALL, 0) == KC_ERR_UNSUPPORTED
        assert L.kc_dds_header(8, 8, fmt, ALL, 1, (C.c_uint8 * 148)(), None) == KC_ERR_UNSUPPORTED
    assert not (tmp_path / "x.dds").exists()
    assert L.kc_image_from_bc(None, 0, 8, 8, 7, ALL, None, None) == KC_ERR_INVALID_ARG  # an unknown format comes after the flags
    # kc_image_read_dds: flags, arguments, the file, the header, the level, then kc_image_from_bc
    good = tmp_path / "good.dds"
    good.write_bytes(api.dds_header(8, 8, BC7, False, 4) + bytes(R.chain_bytes(8, 8, BC7, 4)))
    bc6 = tmp_path / "bc6.dds"
    bc6.write_bytes(api.dds_header(8, 8, BC6H, False, 4) + bytes(R.chain_bytes(8, 8, BC7, 4)))
    path = lambda p: str(p).encode()
    assert L.kc_image_read_dds(path(good), 0, ALL | SRGB, C.byref(out), None) == KC_ERR_UNSUPPORTED
    assert L.kc_image_read_dds(None, 0, ALL, C.byref(out), None) == KC_ERR_INVALID_ARG
    assert L.kc_image_read_dds(path(tmp_path / "none.dds"), 0, ALL, C.byref(out), None) == R.KC_ERR_IO
    assert L.kc_image_read_dds(path(bc6), 0, ALL, C.byref(out), None) == KC_ERR_UNSUPPORTED  # dxgiFormat 95 stays unread, flag or not
    assert L.kc_image_read_dds(path(good), 4, ALL, C.byref(out), None) == KC_ERR_INVALID_ARG
    assert L.kc_image_read_dds(path(good), 0, ALL | GRAY, C.byref(out), None) == KC_ERR_UNSUPPORTED  # BC7 has no Gray form
    if not gpu:
        assert L.kc_image_read_dds(path(good), 3, ALL, C.byref(out), None) == KC_ERR_NO_DEVICE


def test_all_modes_needs_blocks_in_the_python_api():
    from kanter_core_amd import api
    img = api.SlotImage(0)  # no handle: the check comes before any call
    with pytest.raises(ValueError):
        img.bc_error(BC7, all_modes=True)
