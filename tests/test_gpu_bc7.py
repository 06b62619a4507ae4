"""BC7 on the device (kc_image_to_bc and the other block entry points with KC_BC7 = 98, csrc/bc7.hip): the blocks are
bc7_ref.encode of the RGBA8 bytes kc_image_to_u8 writes, byte for byte -- linear and sRGB, edge-case floats, Gray and constant
channels, wrapped planes with padding, edge blocks of odd sizes, both cache policies, the grid-stride loop; the device form
agrees with the host form, writes nothing outside the blocks and is ordered on torch's stream; mip chains and DDS files carry
the format; refusals launch nothing."""
import ctypes as C
import os

import numpy as np
import pytest

import bc7_ref
from pngio import read_png
from util import SEED_A, SEED_B, synthetic_rgba, with_edge_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 102, 104
BC7 = 98
BOTH = [False, True]


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
    return [with_edge_cases(p * 1.2 - 0.1, shift=c) for c, p in enumerate(synthetic_rgba(seed, h, w))]


def check(img, srgb, got=None):
    got = img.to_bc(BC7, srgb) if got is None else got
    want = bc7_ref.encode(img.to_u8(srgb))
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere((got != want).any(-1))
    assert bad.size == 0, "BC7 srgb=%s: %d of %d blocks differ, first %s: %s vs %s" % (
        srgb, len(bad), want.shape[0] * want.shape[1], bad[0], got[tuple(bad[0])].tobytes().hex(), want[tuple(bad[0])].tobytes().hex())
    return got


@pytest.mark.parametrize("shape", [(1, 1), (4, 4), (3, 5), (13, 17), (129, 257)])
@pytest.mark.parametrize("srgb", BOTH)
def test_rgba_edge_cases(kc, srgb, shape):
    h, w = shape
    check(kc.SlotImage.from_planes(edge_rgba(h, w)), srgb)


@pytest.mark.parametrize("srgb", BOTH)
def test_gray_and_constants(kc, srgb):
    h, w = 21, 30
    check(kc.SlotImage.from_planes([with_edge_cases(synthetic_rgba(SEED_B, h, w)[1] * 1.1 - 0.05)]), srgb)
    check(kc.SlotImage.from_value(kc.Size(w, h), 0.3, True), srgb)
    check(kc.SlotImage.from_value(kc.Size(w, h), 0.7, False), srgb)
    p = edge_rgba(h, w)
    combined = kc.combine_rgba_process([kc.SlotImage.from_planes([p[0]]), kc.SlotImage.from_planes([p[1]]),
                                        kc.SlotImage.from_planes([p[2]]), kc.value_process(0.6)])
    check(combined, srgb)


@pytest.mark.parametrize("name", ["heart_110.png", "heart_256.png", "image_2.png", "clouds.png"])
def test_png_inputs(kc, name):
    img = kc.SlotImage.from_u8(read_png(os.path.join(INPUTS, name)))
    for srgb in BOTH:
        check(img, srgb)


@pytest.mark.parametrize("w", [9, 10, 11, 12])
def test_wrapped_plane_with_padding(kc, torch, w):
    from kanter_core_amd import _lib
    L = _lib.load()
    h, pitch_f = 19, 20
    p = with_edge_cases(synthetic_rgba(SEED_A, h, w)[2] * 0.8 + 0.1, shift=2)
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
    for srgb in BOTH:
        check(src, srgb)
    del src
    torch.cuda.synchronize()


@pytest.mark.parametrize("srgb", BOTH)
def test_device_form_equals_host_form_and_keeps_guard_bytes(kc, torch, srgb):
    h, w = 37, 53
    img = kc.SlotImage.from_planes(edge_rgba(h, w))
    host = check(img, srgb)
    assert np.array_equal(img.to_bc_torch(BC7, srgb).cpu().numpy(), host)
    by, bx, bb = host.shape
    assert bb == 16
    big = torch.full((by + 3, bx + 5, bb), 0xa5, dtype=torch.uint8, device="cuda")  # a row pitch above the row's bytes
    img.to_bc_torch(BC7, srgb, out=big[1:1 + by, 2:2 + bx, :])
    got = big.cpu().numpy()
    expect = np.full(got.shape, 0xa5, np.uint8)
    expect[1:1 + by, 2:2 + bx, :] = host
    assert np.array_equal(got, expect)


def test_one_launch_and_algorithmic_bytes(kc):
    h, w = 30, 42
    bx, by = (w + 3) // 4, (h + 3) // 4
    rgba = kc.SlotImage.from_planes(edge_rgba(h, w)).materialize()
    gray = kc.SlotImage.from_planes([edge_rgba(h, w)[0]]).materialize()
    const = kc.SlotImage.from_value(kc.Size(w, h), 0.5, True)
    for img, planes in ((rgba, 4), (gray, 1), (const, 0)):
        st0 = kc.stats()
        img.to_bc(BC7)
        st1 = kc.stats()
        assert st1["kernel_launches"] - st0["kernel_launches"] == 1
        assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == w * h * 4 * planes + bx * by * 16


def test_stream_ordering_without_sync(kc, torch):
    h, w = 256, 256
    rng = np.random.default_rng(91)
    px = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    host = torch.from_numpy(px).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
        torch.cuda._sleep(20_000_000)  # the producer is late: the library's stream must wait for it
        t.copy_(host, non_blocking=True)
        img = kc.SlotImage.from_torch(t)
        out = img.to_bc_torch(BC7)
        flipped = out ^ 0xff  # a torch op on the same stream sees the blocks
        got = flipped.cpu().numpy() ^ 0xff
    check(img, False, got)


def test_live_graph_buffer(kc, torch):
    tp = kc.TextureProcessor.new()
    lg = tp.new_live_graph()
    src = lg.add_node(kc.Node.new(kc.NodeType.Image(os.path.join(INPUTS, "heart_110.png"))))
    sep = lg.add_node(kc.Node.new(kc.NodeType.SeparateRgba))
    lg.connect(src, sep, 0, 0)
    lg.await_clean(sep)
    got = lg.buffer_bc_torch(sep, 1, BC7, True).cpu().numpy()
    image = lg.slot_data(sep, 1).image
    assert got.shape == (28, 28, 16)
    check(image, True, got)
    chain, offs = lg.buffer_bc_mips_torch(sep, 1, "bc7")
    assert offs == kc.bc_mip_layout(110, 110, BC7)[0]
    assert np.array_equal(chain.cpu().numpy(), np.concatenate([l.reshape(-1) for l in image.to_bc_mips(BC7)]))
    torch.cuda.synchronize()


def test_nontemporal_instantiation(kc):
    img = kc.SlotImage.from_planes(edge_rgba(256, 256)).materialize()
    saved = kc.get_option("cache_budget_mb")
    kc.set_option("cache_budget_mb", 0)  # nothing fits: the planes are streamed
    try:
        got = [img.to_bc(BC7, srgb) for srgb in BOTH]
    finally:
        kc.set_option("cache_budget_mb", saved)
    for srgb in BOTH:
        check(img, srgb, got[srgb])
        assert np.array_equal(got[srgb], img.to_bc(BC7, srgb))


def test_grid_stride_loop(kc):
    """1024 x 1024 is 256 workgroups of one block a thread; capped at 48 a thread takes five or six (the sRGB form: its
    first block before the loop, the others in it).  The small image has edge blocks in the loop's later rounds."""
    big = kc.SlotImage.from_planes(edge_rgba(1024, 1024)).materialize()
    small = kc.SlotImage.from_planes(edge_rgba(131, 257, SEED_B)).materialize()
    saved = kc.get_option("tune_cap")
    try:
        kc.set_option("tune_cap", 48)
        got_big = big.to_bc(BC7, True)
        kc.set_option("tune_cap", 2)
        got_small = [small.to_bc(BC7, srgb) for srgb in BOTH]
    finally:
        kc.set_option("tune_cap", saved)
    check(big, True, got_big)
    for srgb in BOTH:
        check(small, srgb, got_small[srgb])


@pytest.mark.parametrize("shape", [(64, 64), (130, 70)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("srgb", BOTH)
def test_chain_equals_the_reference_of_every_level(kc, shape, srgb):
    w, h = shape
    img = kc.SlotImage.from_planes(edge_rgba(h, w))
    want = [bc7_ref.encode(level.to_u8(srgb)) for level in img.mips()]
    assert len(want) == kc.mip_level_count(w, h)
    for per_level in (False, True):
        got = img.to_bc_mips(BC7, srgb, per_level=per_level)
        assert len(got) == len(want)
        for k, (g, r) in enumerate(zip(got, want)):
            assert g.shape == r.shape, (k, g.shape, r.shape)
            assert np.array_equal(g, r), "srgb=%s per_level=%s level %d differs" % (srgb, per_level, k)
    assert np.array_equal(got[0], img.to_bc(BC7, srgb))
    flat, offs = img.to_bc_mips_torch(BC7, srgb)
    assert offs == kc.bc_mip_layout(w, h, BC7)[0]
    assert np.array_equal(flat.cpu().numpy(), np.concatenate([l.reshape(-1) for l in want]))


def test_write_dds(kc, tmp_path):
    w, h = 130, 70
    img = kc.SlotImage.from_planes(edge_rgba(h, w))
    chain = b"".join(l.tobytes() for l in img.to_bc_mips(BC7, True))
    img.write_dds(tmp_path / "chain.dds", BC7, srgb=True)
    data = (tmp_path / "chain.dds").read_bytes()
    assert data == kc.dds_header(w, h, BC7, srgb=True) + chain
    assert data[128:132] == (99).to_bytes(4, "little")  # DXGI_FORMAT_BC7_UNORM_SRGB
    img.write_dds(tmp_path / "top.dds", "bc7", mips=False)
    assert (tmp_path / "top.dds").read_bytes() == kc.dds_header(w, h, BC7, levels=1) + img.to_bc(BC7).tobytes()
    Image = pytest.importorskip("PIL.Image")
    with Image.open(tmp_path / "chain.dds") as im:
        assert im.size == (w, h)
        pix = np.asarray(im.convert("RGBA"))
    assert np.array_equal(pix, bc7_ref.decode(img.to_bc(BC7, True), h, w))


def test_refusals_launch_nothing(kc, torch):
    from kanter_core_amd import _lib
    L = _lib.load()
    img = kc.SlotImage.from_planes(synthetic_rgba(SEED_A, 8, 8)).materialize()
    t = torch.zeros((2, 3, 16), dtype=torch.uint8, device="cuda")
    buf = np.zeros(64, np.uint8)
    n0 = kc.stats()["kernel_launches"]
    ok = _lib.kc_bc_image(t.data_ptr(), 8, 8, BC7, 48)
    assert L.kc_image_to_bc_device(img._h, C.byref(ok), 4, None) == KC_ERR_UNSUPPORTED  # an unknown flag bit
    assert L.kc_image_to_bc_device(img._h, C.byref(ok), 2, None) == KC_ERR_UNSUPPORTED  # KC_MIP_PER_LEVEL is not this call's
    assert L.kc_image_to_bc(img._h, BC7, 8, buf.ctypes.data, 64) == KC_ERR_UNSUPPORTED
    size = _lib.kc_bc_image(t.data_ptr(), 4, 8, BC7, 48)  # not the image's size
    assert L.kc_image_to_bc_device(img._h, C.byref(size), 0, None) == KC_ERR_INVALID_ARG
    mis = _lib.kc_bc_image(t.data_ptr() + 8, 8, 8, BC7, 48)  # misaligned for 16-byte blocks
    assert L.kc_image_to_bc_device(img._h, C.byref(mis), 0, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc(img._h, BC7, 0, buf.ctypes.data, 63) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc(img._h, 7, 0, buf.ctypes.data, 64) == KC_ERR_INVALID_ARG  # 7 is still not a format
    with pytest.raises(ValueError):
        img.to_bc(7)
    with pytest.raises(ValueError):
        img.to_bc("7")
    assert kc.stats()["kernel_launches"] == n0
    assert not t.cpu().numpy().any() and not buf.any()
    assert L.kc_image_to_bc_device(img._h, C.byref(ok), 1, None) == 0
    assert kc.stats()["kernel_launches"] == n0 + 1
    torch.cuda.synchronize()
    got = t.cpu().numpy()
    check(img, True, got[:, :2, :])
    assert not got[:, 2, :].any()
