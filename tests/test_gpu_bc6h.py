"""BC6H on the device (the block entry points with KC_BC6H = 95, csrc/bc6h.hip): the blocks are bc6h_ref.encode of the image's f32
planes, byte for byte -- values above 1, edge-case floats, the values where a half rounds, saturates or flushes, Gray and
constant channels, wrapped planes with padding, edge blocks of odd sizes, both cache policies, the grid-stride loop, and every
value an endpoint can take; the device form agrees with the host form, writes nothing outside the blocks and is ordered on
torch's stream; mip chains and DDS files carry the format; random blocks of every mode decode to bc6h_ref.decode exactly as f32;
the error record is the reference's, integer for integer; kc_stats counts what the header documents and refusals launch
nothing."""
import ctypes as C
import os

import numpy as np
import pytest

import bc6h_ref as R
from util import SEED_A, SEED_B, synthetic_rgba, with_edge_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 102, 104
BC6H = R.BC6H
f32 = np.float32
TIE = f32(2.0) ** -25  # halfway between 0 and the smallest denormal half
HALF_EDGES = np.array([65504, 65519.99, 65520, 1e30, np.inf, -np.inf, np.nan, -0.0, 6.1035e-5, 5.96e-8, TIE, np.nextafter(TIE, f32(1)),
                       65472, 65488, 1.0, 1.0 + 2.0 ** -11], f32)


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    return kc


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def hdr_rgba(h, w, seed=SEED_A):
    """f32 planes over [-0.5, 7.5) with infinities, NaN, negatives and huge values among them"""
    return [with_edge_cases(p * 8 - 0.5, shift=c) for c, p in enumerate(synthetic_rgba(seed, h, w))]


def half_edge_plane(h, w, shift=0):
    """a plane that carries the values where the quantiser rounds, saturates or flushes, again and again"""
    n = h * w
    return np.roll(np.resize(HALF_EDGES, n), shift).reshape(h, w)


def check(img, got=None, planes=None):
    """planes: the image's planes where the caller knows them better than a download does"""
    got = img.to_bc(BC6H) if got is None else got
    want = R.encode(img.planes() if planes is None else planes)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere((got != want).any(-1))
    assert bad.size == 0, "BC6H: %d of %d blocks differ, first %s: %s vs %s" % (
        len(bad), want.shape[0] * want.shape[1], bad[0], got[tuple(bad[0])].tobytes().hex(), want[tuple(bad[0])].tobytes().hex())
    return got


def record(e):
    return dict(format=e.format, channel_mask=e.channel_mask, pixels=e.pixels, sse=[int(v) for v in e.sse], max_abs=[int(v) for v in e.max_abs],
                undecoded_blocks=e.undecoded_blocks, bc7_mode_blocks=[int(v) for v in e.bc7_mode_blocks])


# ------------------------------------------------------------------ encode
@pytest.mark.parametrize("shape", [(1, 1), (4, 4), (3, 5), (13, 17), (129, 257)])
def test_rgba_edge_cases(kc, shape):
    h, w = shape
    check(kc.SlotImage.from_planes(hdr_rgba(h, w)))
    planes = hdr_rgba(h, w, SEED_B)
    planes[1] = half_edge_plane(h, w)
    planes[2] = half_edge_plane(h, w, 5)
    check(kc.SlotImage.from_planes(planes))


def test_gray_and_constants(kc):
    h, w = 21, 30
    check(kc.SlotImage.from_planes([with_edge_cases(synthetic_rgba(SEED_B, h, w)[1] * 8 - 0.5)]))
    check(kc.SlotImage.from_planes([half_edge_plane(h, w, 3)]))
    for value in (0.3, 2.75, 70000.0, -1.0):
        check(kc.SlotImage.from_value(kc.Size(w, h), value, True))
        check(kc.SlotImage.from_value(kc.Size(w, h), value, False))
    p = hdr_rgba(h, w)
    combined = kc.combine_rgba_process([kc.SlotImage.from_planes([p[0]]), kc.SlotImage.from_planes([p[1]]),
                                        kc.value_process(3.5), kc.SlotImage.from_planes([p[3]])])
    # value_process makes a 1 x 1 constant plane that every size reads: the reference takes it at the image's size
    check(combined, planes=[p[0], p[1], np.full((h, w), 3.5, f32)])


@pytest.mark.parametrize("w", [9, 10, 11, 12])
def test_wrapped_plane_with_padding(kc, torch, w):
    from kanter_core_amd import _lib
    L = _lib.load()
    h, pitch_f = 19, 20
    p = with_edge_cases(synthetic_rgba(SEED_A, h, w)[2] * 8 - 0.5, shift=2)
    t = torch.empty((h, pitch_f), dtype=torch.float32, device="cuda")
    pad = torch.tensor([float("nan"), -float("inf"), 1e30, -1e30], dtype=torch.float32)
    t[:, :] = pad.repeat(pitch_f // 4).cuda()  # poison: what lies past the width must not reach a block
    t[:, :w] = torch.from_numpy(p).cuda()
    torch.cuda.synchronize()
    plane, img = C.c_void_p(), C.c_void_p()
    assert L.kc_plane_wrap(t.data_ptr(), w, h, pitch_f * 4, C.byref(plane)) == 0
    assert L.kc_image_gray(plane, C.byref(img)) == 0
    L.kc_plane_release(plane)
    src = kc.SlotImage(img.value)
    got = src.to_bc(BC6H)
    assert np.array_equal(got, R.encode([p]))
    del src
    torch.cuda.synchronize()


def test_device_form_equals_host_form_and_keeps_guard_bytes(kc, torch):
    h, w = 37, 53
    img = kc.SlotImage.from_planes(hdr_rgba(h, w))
    host = check(img)
    assert np.array_equal(img.to_bc_torch(BC6H).cpu().numpy(), host)
    assert np.array_equal(img.to_bc_torch("bc6h").cpu().numpy(), host)
    by, bx, bb = host.shape
    assert bb == 16
    big = torch.full((by + 3, bx + 5, bb), 0xa5, dtype=torch.uint8, device="cuda")  # a row pitch above the row's bytes
    img.to_bc_torch(BC6H, out=big[1:1 + by, 2:2 + bx, :])
    got = big.cpu().numpy()
    expect = np.full(got.shape, 0xa5, np.uint8)
    expect[1:1 + by, 2:2 + bx, :] = host
    assert np.array_equal(got, expect)


def test_one_launch_and_algorithmic_bytes(kc):
    h, w = 30, 42
    bx, by = (w + 3) // 4, (h + 3) // 4
    rgba = kc.SlotImage.from_planes(hdr_rgba(h, w)).materialize()
    gray = kc.SlotImage.from_planes([hdr_rgba(h, w)[0]]).materialize()
    const = kc.SlotImage.from_value(kc.Size(w, h), 2.5, True)
    for img, planes in ((rgba, 3), (gray, 1), (const, 0)):  # alpha is never read
        st0 = kc.stats()
        img.to_bc(BC6H)
        st1 = kc.stats()
        assert st1["kernel_launches"] - st0["kernel_launches"] == 1
        assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == w * h * 4 * planes + bx * by * 16


def test_stream_ordering_without_sync(kc, torch):
    h, w = 256, 256
    rng = np.random.default_rng(91)
    px = (rng.random((h, w, 4), dtype=np.float32) * 8 - 0.5).astype(np.float32)
    host = torch.from_numpy(px).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        torch.cuda._sleep(20_000_000)  # the producer is late: the library's stream must wait for it
        t.copy_(host, non_blocking=True)
        img = kc.SlotImage.from_torch(t)
        out = img.to_bc_torch(BC6H)
        flipped = out ^ 0xff  # a torch op on the same stream sees the blocks
        got = flipped.cpu().numpy() ^ 0xff
    assert np.array_equal(got, R.encode([px[..., c] for c in range(3)]))


def test_live_graph_buffer(kc, torch):
    tp = kc.TextureProcessor.new()
    lg = tp.new_live_graph()
    src = lg.add_node(kc.Node.new(kc.NodeType.Image(os.path.join(INPUTS, "heart_110.png"))))
    sep = lg.add_node(kc.Node.new(kc.NodeType.SeparateRgba))
    lg.connect(src, sep, 0, 0)
    lg.await_clean(sep)
    got = lg.buffer_bc_torch(sep, 1, BC6H).cpu().numpy()
    image = lg.slot_data(sep, 1).image
    assert got.shape == (28, 28, 16)
    check(image, got)
    chain, offs = lg.buffer_bc_mips_torch(sep, 1, "bc6h")
    assert offs == kc.bc_mip_layout(110, 110, BC6H)[0]
    assert np.array_equal(chain.cpu().numpy(), np.concatenate([l.reshape(-1) for l in image.to_bc_mips(BC6H)]))
    assert record(lg.buffer_bc_error(sep, 1, BC6H)) == R.compare(image.planes(), got)
    torch.cuda.synchronize()


def test_nontemporal_instantiation(kc):
    img = kc.SlotImage.from_planes(hdr_rgba(256, 256)).materialize()
    saved = kc.get_option("cache_budget_mb")
    kc.set_option("cache_budget_mb", 0)  # nothing fits: the planes are streamed
    try:
        got = img.to_bc(BC6H)
    finally:
        kc.set_option("cache_budget_mb", saved)
    check(img, got)
    assert np.array_equal(got, img.to_bc(BC6H))


def test_grid_stride_loop(kc):
    """1024 x 1024 is 256 workgroups of one block a thread; capped at 48 a thread takes five or six.  The small image has edge
    blocks in the loop's later rounds."""
    big = kc.SlotImage.from_planes(hdr_rgba(1024, 1024)).materialize()
    small = kc.SlotImage.from_planes(hdr_rgba(131, 257, SEED_B)).materialize()
    saved = kc.get_option("tune_cap")
    try:
        kc.set_option("tune_cap", 48)
        got_big = big.to_bc(BC6H)
        kc.set_option("tune_cap", 2)
        got_small = small.to_bc(BC6H)
    finally:
        kc.set_option("tune_cap", saved)
    check(big, got_big)
    check(small, got_small)


def test_every_endpoint_value(kc):
    """Block (i, j) of a 1024 x 496 image is the constant colour R = e, G = 7919 e mod 31744, B = 31743 - e with e = 256 j + i,
    built from half bits: every one of the 31 744 values goes through the device's quantiser and its endpoint search."""
    e = (256 * np.arange(124)[:, None] + np.arange(256)[None, :]).astype(np.int64)
    assert e.max() == R.HALF_MAX and len(np.unique(e)) == R.HALF_MAX + 1
    bits = [e, (7919 * e) % 31744, R.HALF_MAX - e]
    assert all(len(np.unique(b)) == R.HALF_MAX + 1 for b in bits)
    planes = [np.repeat(np.repeat(R.half_value(b), 4, 0), 4, 1) for b in bits]
    assert planes[0].shape == (496, 1024) and all(np.array_equal(R.quant_half(p[::4, ::4]), b) for p, b in zip(planes, bits))
    img = kc.SlotImage.from_planes(planes + [np.ones((496, 1024), f32)])
    got = check(img)
    q = np.stack([R.q10(b) for b in bits], -1).reshape(-1, 3)
    fields = R._bits(got.reshape(-1, 16))
    assert np.array_equal(R._get(fields, 5, 10, 3), q) and np.array_equal(R._get(fields, 35, 10, 3), q)
    assert not fields[:, 65:].any()


# ------------------------------------------------------------------ mip chains and DDS
@pytest.mark.parametrize("shape", [(64, 64), (130, 70)], ids=lambda s: "%dx%d" % s)
def test_chain_equals_the_reference_of_every_level(kc, shape):
    w, h = shape
    img = kc.SlotImage.from_planes(hdr_rgba(h, w))
    want = [R.encode(level.planes()) for level in img.mips()]
    assert len(want) == kc.mip_level_count(w, h)
    for per_level in (False, True):
        got = img.to_bc_mips(BC6H, per_level=per_level)
        assert len(got) == len(want)
        for k, (g, r) in enumerate(zip(got, want)):
            assert g.shape == r.shape, (k, g.shape, r.shape)
            assert np.array_equal(g, r), "per_level=%s level %d differs" % (per_level, k)
    assert np.array_equal(got[0], img.to_bc(BC6H))
    flat, offs = img.to_bc_mips_torch(BC6H)
    assert offs == kc.bc_mip_layout(w, h, BC6H)[0]
    assert np.array_equal(flat.cpu().numpy(), np.concatenate([l.reshape(-1) for l in want]))


def test_write_dds(kc, tmp_path):
    w, h = 130, 70
    planes = hdr_rgba(h, w)
    planes[0] = np.abs(synthetic_rgba(SEED_B, h, w)[0])  # one channel that stays inside [0, 1], where Pillow's bytes tell values apart
    img = kc.SlotImage.from_planes(planes)
    chain = b"".join(l.tobytes() for l in img.to_bc_mips(BC6H))
    img.write_dds(tmp_path / "chain.dds", BC6H)
    data = (tmp_path / "chain.dds").read_bytes()
    assert data == kc.dds_header(w, h, BC6H) + chain
    assert data[128:132] == (95).to_bytes(4, "little")  # DXGI_FORMAT_BC6H_UF16
    img.write_dds(tmp_path / "top.dds", "bc6h", mips=False)
    top = img.to_bc(BC6H)
    assert (tmp_path / "top.dds").read_bytes() == kc.dds_header(w, h, BC6H, levels=1) + top.tobytes()
    with pytest.raises(kc.TexProError):
        img.write_dds(tmp_path / "srgb.dds", BC6H, srgb=True)
    with pytest.raises(kc.TexProError):
        kc.SlotImage.read_dds(tmp_path / "chain.dds")  # reading format 95 back is the stated gap
    # the payload goes back through from_bc instead
    back = kc.SlotImage.from_bc(np.frombuffer(data[148:148 + top.nbytes], np.uint8), w, h, BC6H)
    for got, want in zip(back.planes(), R.decode_planes(top, h, w)):
        assert np.array_equal(got, want)
    Image = pytest.importorskip("PIL.Image")
    with Image.open(tmp_path / "chain.dds") as im:
        assert im.size == (w, h) and im.mode == "RGB"
        pix = np.asarray(im)
    assert np.array_equal(pix, R.pillow_bytes(R.decode(top, h, w, round_term=0)[0]))


# ------------------------------------------------------------------ decode
def check_decoded(img, blk, w, h):
    assert img.is_rgba() and (img.size().width, img.size().height) == (w, h)
    want = R.decode_planes(blk, h, w)
    for c, (got, ref) in enumerate(zip(img.planes(), want)):
        assert got.dtype == np.float32 and got.shape == ref.shape
        bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
        assert bad.size == 0, "plane %d: %d pixels differ, first %s: %r vs %r" % (c, len(bad), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


@pytest.mark.parametrize("w,h", [(4, 4), (17, 13), (64, 64), (160, 120)])
def test_random_blocks_decode_to_the_reference(kc, torch, w, h):
    from kanter_core_amd import _lib
    L = _lib.load()
    blk = R.random_image_blocks(h, w, seed=2 if (w, h) == (160, 120) else 0)
    by, bx, _ = blk.shape
    undecoded = R.decode(blk, h, w)[2]
    assert (undecoded > 0) == (by * bx > 16)  # the two-subset modes follow the first sixteen blocks of a cycle
    img, n = kc.SlotImage.from_bc(blk, w, h, BC6H, return_undecoded=True)
    assert n == undecoded
    check_decoded(img, blk, w, h)
    check_decoded(kc.SlotImage.from_bc(blk, w, h, "bc6h"), blk, w, h)  # without the count: the other instantiation
    # alpha is a constant plane of 1, the colour planes are resident
    for c, p in enumerate(img.plane_handles()):
        is_const, v = C.c_int(), C.c_float()
        assert L.kc_plane_is_const(p, C.byref(is_const), C.byref(v)) == 0
        assert bool(is_const.value) == (c == 3) and (c < 3 or v.value == 1.0)
    # the device form: behind a row pitch and an offset, whatever lies between the block rows
    fill = np.random.default_rng(17).integers(0, 256, (by + 2, bx + 3, 16), dtype=np.uint8)
    fill[1:1 + by, 2:2 + bx] = blk
    big = torch.from_numpy(fill).cuda()
    dev, n = kc.SlotImage.from_bc_torch(big[1:1 + by, 2:2 + bx, :], w, h, BC6H, return_undecoded=True)
    assert n == undecoded
    check_decoded(dev, blk, w, h)
    check_decoded(kc.SlotImage.from_bc_torch(big[1:1 + by, 2:2 + bx, :], w, h, BC6H), blk, w, h)
    assert np.array_equal(big.cpu().numpy(), fill)  # the caller's blocks are read, never written
    with pytest.raises(kc.TexProError):
        kc.SlotImage.from_bc(blk, w, h, BC6H, gray=True)  # KC_BC_GRAY stays BC4's


def test_round_trip_decodes_to_the_reference(kc):
    h, w = 67, 130
    img = kc.SlotImage.from_planes(hdr_rgba(h, w))
    blk = check(img)
    got, n = kc.SlotImage.from_bc(blk, w, h, BC6H, return_undecoded=True)
    assert n == 0
    check_decoded(got, blk, w, h)
    # a decoded image holds halves: encoding it again quantises nothing away
    assert np.array_equal(R.texels(got.planes()), R.decode(blk, h, w)[0])


# ------------------------------------------------------------------ the error of an encoding
@pytest.mark.parametrize("w,h", [(1, 1), (4, 4), (5, 3), (17, 13), (64, 64), (257, 129)])
def test_bc_error_equals_the_reference_record(kc, torch, w, h):
    planes = hdr_rgba(h, w)
    planes[2] = half_edge_plane(h, w, 1)
    img = kc.SlotImage.from_planes(planes)
    e = img.bc_error(BC6H)
    want = R.compare(planes, R.encode(planes))
    assert record(e) == want
    assert e.flags == 0 and e.undecoded_blocks == 0 and e.channel_mask == 0x7 and not e.bc7_mode_blocks.any()
    assert record(img.bc_error(BC6H, blocks=img.to_bc_torch(BC6H))) == want
    assert e.psnr() == pytest.approx(R.psnr(want), rel=1e-12)
    # other blocks than the image's own: random ones of every mode, behind a row pitch
    blk = R.random_image_blocks(h, w, seed=5)
    by, bx, bb = blk.shape
    big = torch.full((by + 1, bx + 2, bb), 0x5a, dtype=torch.uint8, device="cuda")
    big[:by, 1:1 + bx] = torch.from_numpy(blk).cuda()
    other = img.bc_error(BC6H, blocks=big[:by, 1:1 + bx, :])
    want = R.compare(planes, blk)
    assert record(other) == want and (want["undecoded_blocks"] > 0) == (by * bx > 16)
    assert other.psnr(channels=[1]) == pytest.approx(R.psnr(want, channels=[1]), rel=1e-12)
    with pytest.raises(ValueError):
        other.psnr(channels=[3])  # alpha is outside the mask


def test_gray_and_constant_images_compare(kc):
    w, h = 30, 21
    gray_plane = hdr_rgba(h, w)[1]
    gray = kc.SlotImage.from_planes([gray_plane])
    const = kc.SlotImage.from_value(kc.Size(w, h), 2.5, True)
    blocks = ((w + 3) // 4) * ((h + 3) // 4)
    assert record(gray.bc_error(BC6H)) == R.compare([gray_plane], R.encode([gray_plane]))
    flat = [np.full((h, w), 2.5, f32)] * 3
    assert record(const.bc_error(BC6H)) == R.compare(flat, R.encode(flat))
    # a constant image: no plane is read, by the encoder or by the comparison
    st0 = kc.stats()
    const.bc_error(BC6H)
    st1 = kc.stats()
    assert st1["kernel_launches"] - st0["kernel_launches"] == 3
    assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == 2 * blocks * 16


def test_other_instantiations_of_decode_and_compare(kc):
    """With a cache budget of 0 nothing fits and the kernels take their nontemporal forms; with a grid cap of 2 workgroups a
    thread of the 33 x 17 block image takes two blocks, edge blocks in the later round among them."""
    w, h = 130, 67
    planes = hdr_rgba(h, w)
    img = kc.SlotImage.from_planes(planes).materialize()
    blk = R.random_image_blocks(h, w, seed=9)
    want_n = R.decode(blk, h, w)[2]
    want_rec = R.compare(planes, R.encode(planes))
    for option, value in (("cache_budget_mb", 0), ("tune_cap", 2)):
        saved = kc.get_option(option)
        kc.set_option(option, value)
        try:
            got, n = kc.SlotImage.from_bc(blk, w, h, BC6H, return_undecoded=True)
            plain = kc.SlotImage.from_bc(blk, w, h, BC6H)
            e = img.bc_error(BC6H)
        finally:
            kc.set_option(option, saved)
        assert n == want_n, option
        check_decoded(got, blk, w, h)
        check_decoded(plain, blk, w, h)
        assert record(e) == want_rec, option


def test_launches_and_algorithmic_bytes_of_decode_and_compare(kc, torch):
    w, h = 42, 30
    bx, by = (w + 3) // 4, (h + 3) // 4
    rgba = kc.SlotImage.from_planes(hdr_rgba(h, w)).materialize()
    gray = kc.SlotImage.from_planes([hdr_rgba(h, w)[0]]).materialize()
    blk = R.random_image_blocks(h, w)
    t = torch.from_numpy(blk).cuda()
    nblk = bx * by * 16

    def delta(call):
        st0 = kc.stats()
        call()
        st1 = kc.stats()
        return st1["kernel_launches"] - st0["kernel_launches"], st1["algorithmic_bytes"] - st0["algorithmic_bytes"]

    # decode: the blocks plus 4 w h for each of the three planes written; the count is a second launch
    assert delta(lambda: kc.SlotImage.from_bc(blk, w, h, BC6H)) == (1, nblk + 4 * w * h * 3)
    assert delta(lambda: kc.SlotImage.from_bc(blk, w, h, BC6H, return_undecoded=True)) == (2, nblk + 4 * w * h * 3)
    # compare: the planes read plus the blocks; bc_error: the encoder's launch and bytes first
    assert delta(lambda: rgba.bc_error(BC6H, blocks=t)) == (2, nblk + 4 * w * h * 3)
    assert delta(lambda: rgba.bc_error(BC6H)) == (3, 2 * (nblk + 4 * w * h * 3))
    assert delta(lambda: gray.bc_error(BC6H)) == (3, 2 * (nblk + 4 * w * h))


# ------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(kc, torch):
    from kanter_core_amd import _lib
    L = _lib.load()
    img = kc.SlotImage.from_planes(synthetic_rgba(SEED_A, 8, 8)).materialize()
    t = torch.zeros((2, 3, 16), dtype=torch.uint8, device="cuda")
    buf = np.zeros(64, np.uint8)
    err = _lib.kc_bc_error()
    out = C.c_void_p()
    before = kc.stats()
    ok = _lib.kc_bc_image(t.data_ptr(), 8, 8, BC6H, 48)
    assert L.kc_image_to_bc_device(img._h, C.byref(ok), 1, None) == KC_ERR_UNSUPPORTED  # KC_BC_SRGB: half floats have no sRGB form
    assert L.kc_image_to_bc_device(img._h, C.byref(ok), 4, None) == KC_ERR_UNSUPPORTED  # an unknown flag bit
    assert L.kc_image_to_bc(img._h, BC6H, 1, buf.ctypes.data, 64) == KC_ERR_UNSUPPORTED
    assert L.kc_image_to_bc_mips(img._h, BC6H, 1, buf.ctypes.data, 64) == KC_ERR_UNSUPPORTED
    assert L.kc_image_bc_error(img._h, BC6H, 1, C.byref(err)) == KC_ERR_UNSUPPORTED
    assert L.kc_image_bc_compare(img._h, C.byref(ok), 1, C.byref(err)) == KC_ERR_UNSUPPORTED
    assert L.kc_image_from_bc_device(C.byref(ok), 1, None, C.byref(out), None) == KC_ERR_UNSUPPORTED
    assert L.kc_image_from_bc_device(C.byref(ok), 4, None, C.byref(out), None) == KC_ERR_UNSUPPORTED  # KC_BC_GRAY
    size = _lib.kc_bc_image(t.data_ptr(), 4, 8, BC6H, 48)  # not the image's size
    assert L.kc_image_to_bc_device(img._h, C.byref(size), 0, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_bc_compare(img._h, C.byref(size), 0, C.byref(err)) == KC_ERR_INVALID_ARG
    mis = _lib.kc_bc_image(t.data_ptr() + 8, 8, 8, BC6H, 48)  # misaligned for 16-byte blocks
    assert L.kc_image_to_bc_device(img._h, C.byref(mis), 0, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_from_bc_device(C.byref(mis), 0, None, C.byref(out), None) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc(img._h, BC6H, 0, buf.ctypes.data, 63) == KC_ERR_INVALID_ARG
    assert L.kc_image_from_bc(buf.ctypes.data, 63, 8, 8, BC6H, 0, C.byref(out), None) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc(img._h, 96, 0, buf.ctypes.data, 64) == KC_ERR_INVALID_ARG  # the signed form is not a format
    with pytest.raises(ValueError):
        img.to_bc(6)
    with pytest.raises(kc.TexProError):
        img.to_bc(BC6H, srgb=True)
    after = kc.stats()
    assert after["kernel_launches"] == before["kernel_launches"] and after["algorithmic_bytes"] == before["algorithmic_bytes"]
    assert not t.cpu().numpy().any() and not buf.any() and not out.value
    assert L.kc_image_to_bc_device(img._h, C.byref(ok), 0, None) == 0
    assert kc.stats()["kernel_launches"] == before["kernel_launches"] + 1
    torch.cuda.synchronize()
    got = t.cpu().numpy()
    check(img, got[:, :2, :])
    assert not got[:, 2, :].any()
