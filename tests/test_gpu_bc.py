"""Block compression on the device (kc_image_to_bc / kc_image_to_bc_device / kc_live_graph_buffer_bc, csrc/bc.*): the blocks are
bc_ref.encode of the RGBA8 bytes kc_image_to_u8 writes, byte for byte -- every format, sRGB where it is allowed, edge-case
floats, Gray and constant channels, wrapped planes with padding, edge blocks of odd sizes -- the host and device forms agree,
bytes outside the blocks are never written, the device form is ordered on torch's stream, and refusals launch nothing."""
import ctypes as C
import os

import numpy as np
import pytest

import bc_ref
from pngio import read_png
from util import SEED_A, SEED_B, synthetic_rgba, with_edge_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 102, 104
FORMS = [(1, False), (1, True), (3, False), (3, True), (4, False), (5, False)]


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    return kc


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def launches(kc):
    return kc.stats()["kernel_launches"]


def edge_rgba(h, w, seed=SEED_A):
    return [with_edge_cases(p * 1.2 - 0.1, shift=c) for c, p in enumerate(synthetic_rgba(seed, h, w))]


def check(img, fmt, srgb, got=None):
    if got is None:
        got = img.to_bc(fmt, srgb)
    want = bc_ref.encode(img.to_u8(srgb), fmt)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere((got != want).any(-1))
    assert bad.size == 0, "BC%d srgb=%s: %d blocks differ, first %s: %s vs %s" % (
        fmt, srgb, len(bad), bad[0], got[tuple(bad[0])].tobytes().hex(), want[tuple(bad[0])].tobytes().hex())
    return got


@pytest.mark.parametrize("shape", [(1, 1), (4, 4), (3, 5), (13, 17), (129, 257)])
@pytest.mark.parametrize("fmt,srgb", FORMS)
def test_rgba_edge_cases(kc, fmt, srgb, shape):
    h, w = shape
    check(kc.SlotImage.from_planes(edge_rgba(h, w)), fmt, srgb)


@pytest.mark.parametrize("fmt,srgb", FORMS)
def test_gray_and_constants(kc, fmt, srgb):
    h, w = 21, 30
    g = kc.SlotImage.from_planes([with_edge_cases(synthetic_rgba(SEED_B, h, w)[1] * 1.1 - 0.05)])
    check(g, fmt, srgb)
    check(kc.SlotImage.from_value(kc.Size(w, h), 0.3, True), fmt, srgb)
    check(kc.SlotImage.from_value(kc.Size(w, h), 0.7, False), fmt, srgb)
    p = edge_rgba(h, w)
    combined = kc.combine_rgba_process([kc.SlotImage.from_planes([p[0]]), kc.SlotImage.from_planes([p[1]]),
                                        kc.SlotImage.from_planes([p[2]]), kc.value_process(0.6)])
    check(combined, fmt, srgb)


@pytest.mark.parametrize("name", ["heart_110.png", "heart_256.png", "image_2.png"])
def test_png_inputs(kc, name):
    img = kc.SlotImage.from_u8(read_png(os.path.join(INPUTS, name)))
    for fmt, srgb in FORMS:
        check(img, fmt, srgb)


@pytest.mark.parametrize("size", [1024, 4096])
def test_large(kc, size):
    img = kc.SlotImage.from_planes(edge_rgba(size, size))
    for fmt, srgb in FORMS if size == 1024 else [(1, False), (3, True), (5, False)]:
        check(img, fmt, srgb)


@pytest.mark.parametrize("option,value", [("tune_cap", 2), ("cache_budget_mb", 0)])
def test_grid_stride_loop(kc, option, value):
    """Capped at two workgroups, 512 threads, the 33 x 24 = 792 blocks of 131 x 93 take two rounds, the second partly out of
    range, with edge blocks in both (the sRGB forms: a thread's first block before the loop, its second in it).  5 x 3 is two
    blocks: nearly every thread of an sRGB form leaves after the barrier of the threshold table.  cache_budget_mb = 0: the
    same under the cap, in the nontemporal instantiations."""
    imgs = [kc.SlotImage.from_planes(edge_rgba(93, 131)).materialize(), kc.SlotImage.from_planes(edge_rgba(3, 5, SEED_B)).materialize()]
    saved = {o: kc.get_option(o) for o in ("tune_cap", option)}
    try:
        kc.set_option("tune_cap", 2)
        kc.set_option(option, value)
        got = [[img.to_bc(fmt, srgb) for fmt, srgb in FORMS] for img in imgs]
    finally:
        for o, v in saved.items():
            kc.set_option(o, v)
    for img, blocks in zip(imgs, got):
        for (fmt, srgb), g in zip(FORMS, blocks):
            check(img, fmt, srgb, g)


@pytest.mark.parametrize("w", [9, 10, 11, 12])
def test_wrapped_plane_with_padding(kc, torch, w):
    from kanter_core_amd import _lib
    L = _lib.load()
    h, pitch_f = 19, 20
    p = with_edge_cases(synthetic_rgba(SEED_A, h, w)[2] * 0.8 + 0.1, shift=2)
    t = torch.empty((h, pitch_f), dtype=torch.float32, device="cuda")
    pad = torch.tensor([float("nan"), -float("inf"), 1e30, -1e30], dtype=torch.float32)
    t[:, :] = pad.repeat(pitch_f // 4).cuda()
    t[:, :w] = torch.from_numpy(p).cuda()
    torch.cuda.synchronize()
    plane, img = C.c_void_p(), C.c_void_p()
    assert L.kc_plane_wrap(t.data_ptr(), w, h, pitch_f * 4, C.byref(plane)) == 0
    assert L.kc_image_gray(plane, C.byref(img)) == 0
    L.kc_plane_release(plane)
    src = kc.SlotImage(img.value)
    for fmt, srgb in FORMS:
        check(src, fmt, srgb)
    del src
    torch.cuda.synchronize()


@pytest.mark.parametrize("fmt,srgb", FORMS)
def test_device_form_equals_host_form_and_keeps_padding(kc, torch, fmt, srgb):
    h, w = 37, 53
    img = kc.SlotImage.from_planes(edge_rgba(h, w))
    host = img.to_bc(fmt, srgb)
    assert np.array_equal(img.to_bc_torch(fmt, srgb).cpu().numpy(), host)
    by, bx, bb = host.shape
    big = torch.full((by + 3, bx + 5, bb), 0xa5, dtype=torch.uint8, device="cuda")
    img.to_bc_torch(fmt, srgb, out=big[1:1 + by, 2:2 + bx, :])
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
    cases = [(rgba, 1, 3), (rgba, 3, 4), (rgba, 4, 1), (rgba, 5, 2), (gray, 1, 1), (gray, 3, 1), (gray, 5, 1), (const, 3, 0)]
    for img, fmt, planes in cases:
        st0 = kc.stats()
        img.to_bc(fmt)
        st1 = kc.stats()
        assert st1["kernel_launches"] - st0["kernel_launches"] == 1, fmt
        assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == w * h * 4 * planes + bx * by * bc_ref.BLOCK_BYTES[fmt], fmt


def test_pending_mix_chain_is_forced(kc):
    h, w = 45, 67
    a, b = edge_rgba(h, w, SEED_A), edge_rgba(h, w, SEED_B)
    m = kc.mix_process(kc.SlotImage.from_planes(a), kc.SlotImage.from_planes(b), kc.MixType.Multiply)
    got = m.to_bc(3, True)  # the pending chain runs first
    assert np.array_equal(got, bc_ref.encode(m.to_u8(True), 3))


@pytest.mark.parametrize("which", ["side stream", "default stream"])
def test_stream_ordering_without_sync(kc, torch, which):
    h, w = 1024, 1024
    rng = np.random.default_rng(91)
    px = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    host = torch.from_numpy(px).pin_memory()
    s = torch.cuda.Stream() if which == "side stream" else torch.cuda.default_stream()
    with torch.cuda.stream(s):
        t = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
        torch.cuda._sleep(20_000_000)  # the producer is late: the library's stream must wait for it
        t.copy_(host, non_blocking=True)
        img = kc.SlotImage.from_torch(t)
        out = img.to_bc_torch(3)
        flipped = out ^ 0xff  # a torch op on the same stream sees the blocks
        got = flipped.cpu().numpy() ^ 0xff
    assert np.array_equal(got, bc_ref.encode(img.to_u8(), 3))


def test_height_to_normal_bc5_through_live_graph(kc, torch):
    tp = kc.TextureProcessor.new()
    lg = tp.new_live_graph()
    src = lg.add_node(kc.Node.new(kc.NodeType.Image(os.path.join(INPUTS, "heart_256.png"))))
    sep = lg.add_node(kc.Node.new(kc.NodeType.SeparateRgba))
    h2n = lg.add_node(kc.Node.new(kc.NodeType.HeightToNormal))
    lg.connect(src, sep, 0, 0)
    lg.connect(sep, h2n, 0, 0)
    lg.await_clean(h2n)
    got = lg.buffer_bc_torch(h2n, 0, 5).cpu().numpy()
    assert got.shape == (64, 64, 16)
    assert np.array_equal(got, bc_ref.encode(lg.buffer_rgba(h2n, 0), 5))
    torch.cuda.synchronize()


def test_refusals_launch_nothing(kc, torch):
    from kanter_core_amd import _lib
    L = _lib.load()
    img = kc.SlotImage.from_planes(synthetic_rgba(SEED_A, 8, 8)).materialize()
    t = torch.zeros((2, 2, 16), dtype=torch.uint8, device="cuda")
    n0 = launches(kc)
    host = np.zeros((2, 2, 16), np.uint8)
    d = _lib.kc_bc_image(host.ctypes.data, 8, 8, 3, 32)
    ext = C.c_size_t()
    assert L.kc_bc_image_validate(C.byref(d), C.byref(ext)) == KC_ERR_INVALID_ARG  # a host pointer
    assert ext.value == 64
    assert L.kc_image_to_bc_device(img._h, C.byref(d), 0, None) == KC_ERR_INVALID_ARG
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), 4 << 20) == 0
    try:
        whole = _lib.kc_bc_image(p.value, 8, 4 << 17, 3, 32)  # exactly the allocation
        assert L.kc_bc_image_validate(C.byref(whole), C.byref(ext)) == 0, L.kc_last_error()
        assert ext.value == 4 << 20
        past = _lib.kc_bc_image(p.value, 8, (4 << 17) + 1, 3, 32)  # a block row past its end
        assert L.kc_bc_image_validate(C.byref(past), C.byref(ext)) == KC_ERR_INVALID_ARG
        assert b"allocation" in L.kc_last_error()
        assert L.kc_image_to_bc_device(img._h, C.byref(past), 0, None) == KC_ERR_INVALID_ARG
    finally:
        hip.hipFree(p)
    size = _lib.kc_bc_image(t.data_ptr(), 4, 8, 3, 32)  # not the image's size
    assert L.kc_image_to_bc_device(img._h, C.byref(size), 0, None) == KC_ERR_INVALID_ARG
    mis = _lib.kc_bc_image(t.data_ptr() + 8, 8, 4, 3, 32)  # misaligned for 16-byte blocks
    assert L.kc_image_to_bc_device(img._h, C.byref(mis), 0, None) == KC_ERR_INVALID_ARG
    ok = _lib.kc_bc_image(t.data_ptr(), 8, 8, 4, 32)
    assert L.kc_image_to_bc_device(img._h, C.byref(ok), 1, None) == KC_ERR_UNSUPPORTED  # sRGB with BC4
    assert L.kc_image_to_bc_device(img._h, C.byref(ok), 4, None) == KC_ERR_UNSUPPORTED  # unknown flag
    buf = np.zeros(64, np.uint8)
    assert L.kc_image_to_bc(img._h, 3, 0, buf.ctypes.data, 63) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc(img._h, 2, 0, buf.ctypes.data, 64) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc(img._h, 5, 1, buf.ctypes.data, 64) == KC_ERR_UNSUPPORTED
    assert launches(kc) == n0
    assert L.kc_image_to_bc_device(img._h, C.byref(ok), 0, None) == 0
    assert launches(kc) == n0 + 1
    torch.cuda.synchronize()
