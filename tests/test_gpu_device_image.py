"""Images in device memory (kc_image_from_device / kc_image_to_device / kc_live_graph_buffer_device, csrc/devimage.*): what an
import yields is deconstruct_image (src/shared.rs:16-56) of the caller's pixels, what an export writes is to_u8 / to_u8_srgb
(src/slot_image.rs:141-207) for U8 and the stated conversions for the other element types -- bit for bit, in both layouts,
through strided views, ordered against torch's stream without synchronisation, and refused descriptors never reach a kernel."""
import ctypes as C
import os

import numpy as np
import pytest

from util import SEED_A, SEED_B, assert_planes, synthetic_rgba, with_edge_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 102, 104


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    return kc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def launches(kc):
    return kc.stats()["kernel_launches"]


def rgba_rule(chans, h, w):
    """deconstruct_image's planes from the given channel planes: missing R, G, B = 0, missing A = 1."""
    return [chans[c] if c < len(chans) else np.full((h, w), 1.0 if c == 3 else 0.0, np.float32) for c in range(4)]


def srgb_threshold_values():
    """The floats at and just below every 8-bit sRGB threshold (csrc/srgb_thresholds.inc)."""
    import re
    text = open(os.path.join(ROOT, "kanter_core_amd", "csrc", "srgb_thresholds.inc")).read()
    t = np.array([int(x, 16) for x in re.findall(r"0x([0-9a-f]{8})u", text)], np.uint32).view(np.float32)[1:]
    return np.concatenate([t, np.nextafter(t, np.float32(-1))]).astype(np.float32)


def edge_planes(h, w):
    planes = synthetic_rgba(SEED_A, h, w)
    planes = [with_edge_cases(p * 1.2 - 0.1, shift=c) for c, p in enumerate(planes)]
    thr = srgb_threshold_values()
    for c in range(3):
        flat = planes[c].reshape(-1)
        if flat.size >= 2 * len(thr):
            flat[-len(thr):] = np.roll(thr, 37 * c)
    return planes


# ---- 1. U8 HWC import
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", [(17, 33), (5, 1), (1024, 768)])
def test_u8_import_is_deconstruct_image(kc, orc, torch, channels, shape):
    h, w = shape
    rng = np.random.default_rng(channels * 7919 + h)
    px = rng.integers(0, 256, size=(h, w, channels), dtype=np.uint8)
    t = torch.from_numpy(px).cuda()
    img = kc.SlotImage.from_torch(t)
    assert img.is_rgba() and tuple(img.size()) == (w, h)
    got = img.planes()
    assert_planes(got, kc.SlotImage.from_u8(px).planes(), what="against kc_image_from_u8")
    assert_planes(got, orc.deconstruct_u8(px), what="against the oracle")
    if channels == 1:
        g = kc.SlotImage.from_torch(t, gray=True)
        assert not g.is_rgba()
        assert_planes(g.planes(), orc.deconstruct_u8(px)[:1], what="gray")
        g2 = kc.SlotImage.from_torch(t[:, :, 0], gray=True)  # (H, W)
        assert_planes(g2.planes(), orc.deconstruct_u8(px)[:1], what="gray (H, W)")


# ---- 2. U16 / F16 / BF16 / F32 import, padded rows and gapped planes
def source_values(torch, name, shape, rng):
    if name == "uint16":
        return torch.from_numpy(rng.integers(0, 65536, size=shape, dtype=np.uint16))
    if name == "float32":  # any bits at all, NaN payloads included
        return torch.from_numpy(rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32).view(np.float32))
    bits = rng.integers(0, 65536, size=shape, dtype=np.uint64).astype(np.uint16)  # every half / bfloat16 pattern class
    return torch.from_numpy(bits.view(np.int16)).view(getattr(torch, name))


def expected_f32(torch, name, t):
    if name == "uint16":
        return t.numpy().astype(np.float32) / np.float32(65535)
    return t.float().numpy() if name != "float32" else t.numpy()


@pytest.mark.parametrize("name", ["uint16", "float16", "bfloat16", "float32"])
@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_import_other_dtypes(kc, torch, name, layout, channels):
    h, w = 37, 53
    rng = np.random.default_rng(len(name) * 100 + len(layout) * 10 + channels)
    if layout == "hwc":
        big = source_values(torch, name, (h + 3, w + 5, channels), rng)
        view = big[1:1 + h, 2:2 + w, :]  # padded rows, offset start
        want = [expected_f32(torch, name, view[:, :, c].contiguous()) for c in range(channels)]
    else:
        big = source_values(torch, name, (2 * channels + 1, h + 2, w + 7), rng)
        view = big[1::2][:channels, 1:1 + h, 3:3 + w]  # gaps between the planes and at the rows' ends
        want = [expected_f32(torch, name, view[c].contiguous()) for c in range(channels)]
    dev = big.cuda()
    dview = dev[1:1 + h, 2:2 + w, :] if layout == "hwc" else dev[1::2][:channels, 1:1 + h, 3:3 + w]
    got = kc.SlotImage.from_torch(dview, layout=layout).planes()
    want = rgba_rule(want, h, w)
    if name == "float32":  # the bits as they are
        for c in range(4):
            assert np.array_equal(got[c].view(np.uint32), want[c].view(np.uint32)), c
    else:
        assert_planes(got, want, what="%s %s" % (name, layout))


# ---- 3. U8 export = kc_image_to_u8 = the oracle's to_u8
@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("shape", [(67, 129), (5, 3)])
def test_u8_export_is_to_u8(kc, orc, torch, srgb, shape):
    h, w = shape
    planes = edge_planes(h, w)
    img = kc.SlotImage.from_planes(planes)
    want = img.to_u8(srgb)
    assert np.array_equal(want, orc.to_u8(orc.Image(planes), srgb))
    got = img.to_torch(torch.uint8, srgb=srgb).cpu().numpy()
    assert np.array_equal(got, want)
    for c in (1, 3):
        assert np.array_equal(img.to_torch(torch.uint8, channels=c, srgb=srgb).cpu().numpy(), want[:, :, :c])
    chw = img.to_torch(torch.uint8, layout="chw", srgb=srgb).cpu().numpy()
    assert np.array_equal(chw, want.transpose(2, 0, 1))


# ---- 4. F16 / BF16 / F32 / U16 export
def u16_formula(v):
    x = np.where(v < 0, np.float32(0), v).astype(np.float32)
    x = np.where(x > 1, np.float32(1), x).astype(np.float32)  # NaN passes both
    x = (x * np.float32(65535)).astype(np.float32)
    x = np.where(~(x <= 65535), np.float32(65535), x)
    return x.astype(np.uint16)


@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_other_dtype_exports(kc, torch, layout):
    h, w = 41, 70
    planes = edge_planes(h, w)
    planes[0].reshape(-1)[100:104] = [65504.0, 65520.0, 1e-8, 3.0e38]  # f16 overflow / rounding, bf16 range
    img = kc.SlotImage.from_planes(planes)
    ref = torch.from_numpy(np.stack(planes, 2 if layout == "hwc" else 0))
    for dt in (torch.float16, torch.bfloat16):
        got = img.to_torch(dt, layout=layout).cpu()
        want = ref.to(dt)
        gn, wn = torch.isnan(got), torch.isnan(want)
        assert torch.equal(gn, wn), dt
        gb = got.view(torch.int16).numpy()
        wb = want.view(torch.int16).numpy()
        assert np.array_equal(gb[~gn.numpy()], wb[~wn.numpy()]), dt
    got = img.to_torch(torch.float32, layout=layout).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.numpy().view(np.uint32))
    got = img.to_torch(torch.uint16, layout=layout).cpu().numpy()
    assert np.array_equal(got, u16_formula(ref.numpy()))


# ---- 5. Gray, constant and unmaterialised images
def test_export_gray_constant_and_lazy(kc, orc, torch):
    h, w = 33, 47
    a, b = synthetic_rgba(SEED_A, h, w), synthetic_rgba(SEED_B, h, w)
    g = kc.SlotImage.from_planes([with_edge_cases(a[0])])
    assert np.array_equal(g.to_torch(torch.uint8).cpu().numpy(), g.to_u8())
    got = g.to_torch(torch.float32, layout="chw").cpu().numpy()
    gp = g.planes()[0]
    assert_planes(list(got), [gp, gp, gp, np.ones((h, w), np.float32)], what="gray as (v, v, v, 1)")
    n0 = launches(kc)
    k = kc.SlotImage.from_value(kc.Size(w, h), 0.25, True)
    got = k.to_torch(torch.float32, layout="chw").cpu().numpy()
    assert launches(kc) - n0 == 1  # constants are not materialised first
    assert_planes(list(got), [np.full((h, w), v, np.float32) for v in (0.25, 0.25, 0.25, 1.0)], what="from_value")
    ia, ib = kc.SlotImage.from_planes(a), kc.SlotImage.from_planes(b)
    m = kc.mix_process(ia, ib, kc.MixType.Multiply)  # a pending fused chain
    got = m.to_torch(torch.float32, layout="chw").cpu().numpy()
    want = [orc.mix_plane("Multiply", a[c], b[c]) for c in range(3)] + [np.ones((h, w), np.float32)]
    assert_planes(list(got), want, what="lazy Mix")
    assert np.array_equal(m.to_torch(torch.uint8).cpu().numpy(), m.to_u8())


def test_live_graph_buffer_torch(kc, torch):
    h, w = 40, 24
    a, b = synthetic_rgba(SEED_A, h, w), synthetic_rgba(SEED_B, h, w)
    tp = kc.TextureProcessor.new()
    lg = tp.new_live_graph()
    na = lg.add_node(kc.Node.new(kc.NodeType.Embed(0)))
    nb = lg.add_node(kc.Node.new(kc.NodeType.Embed(1)))
    lg.embed_slot_data_with_id(kc.SlotData(0, 0, kc.SlotImage.from_planes(a)), 0)
    lg.embed_slot_data_with_id(kc.SlotData(0, 0, kc.SlotImage.from_planes(b)), 1)
    mix = lg.add_node(kc.Node.new(kc.NodeType.Mix(kc.MixType.Add)))
    lg.connect(na, mix, 0, 0)
    lg.connect(nb, mix, 0, 1)
    lg.await_clean(mix)
    for srgb in (False, True):
        got = lg.buffer_torch(mix, 0, torch.uint8, srgb=srgb).cpu().numpy()
        assert np.array_equal(got, lg.buffer_rgba(mix, 0, srgb))
    f = lg.buffer_torch(mix, 0).cpu().numpy()
    assert_planes([f[:, :, c] for c in range(4)], lg.slot_data(mix, 0).image.planes(), what="buffer_torch f32")


# ---- 6. strided output: nothing outside the described elements changes
@pytest.mark.parametrize("dtype_name", ["uint8", "float16", "float32"])
def test_export_into_strided_slice(kc, torch, dtype_name):
    dt = getattr(torch, dtype_name)
    h, w = 29, 45
    img = kc.SlotImage.from_planes(edge_planes(h, w))
    full = img.to_torch(dt, channels=3).cpu()
    big = torch.full((h + 4, w + 6, 3), 7, dtype=dt, device="cuda")
    before = big.cpu()
    img.to_torch(out=big[2:2 + h, 3:3 + w, :])
    after = big.cpu()
    expect = before.clone()
    expect[2:2 + h, 3:3 + w, :] = full
    iv = {torch.uint8: torch.uint8, torch.float16: torch.int16, torch.float32: torch.int32}[dt]  # compare bits, NaNs included
    assert torch.equal(after.view(iv), expect.view(iv))
    # planar: every other plane of a larger tensor, an inner window of each
    big = torch.full((7, h + 3, w + 9), 5, dtype=dt, device="cuda")
    before = big.cpu()
    img.to_torch(layout="chw", out=big[0:7:2, 1:1 + h, 4:4 + w])
    after = big.cpu()
    expect = before.clone()
    expect[0:7:2, 1:1 + h, 4:4 + w] = img.to_torch(dt, layout="chw").cpu()
    assert torch.equal(after.view(iv), expect.view(iv))


# ---- 7. ordering against torch's stream, no synchronisation
@pytest.mark.parametrize("which", ["side stream", "default stream"])
def test_stream_ordering_without_sync(kc, orc, torch, which):
    h, w = 1024, 1024
    rng = np.random.default_rng(77)
    px = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    host = torch.from_numpy(px).pin_memory()
    s = torch.cuda.Stream() if which == "side stream" else torch.cuda.default_stream()
    with torch.cuda.stream(s):
        t = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
        torch.cuda._sleep(20_000_000)  # the producer is late: the library's stream must wait for it
        t.copy_(host, non_blocking=True)
        img = kc.SlotImage.from_torch(t)
        del t
        junk = [torch.full((h, w, 4), 255, dtype=torch.uint8, device="cuda") for _ in range(3)]  # may reuse t's memory
        b = kc.SlotImage.from_planes(synthetic_rgba(SEED_B, h, w))
        m = kc.mix_process(img, b, kc.MixType.Multiply)
        out = m.to_torch(torch.float32, layout="chw")
        doubled = out * 2.0  # a torch op on the same stream sees the converted data
        got = doubled.cpu().numpy()
    del junk
    dec = orc.deconstruct_u8(px)
    assert_planes(img.planes(), dec, what="import after the source was freed")
    bp = synthetic_rgba(SEED_B, h, w)
    want = [orc.mix_plane("Multiply", dec[c], bp[c]) * np.float32(2) for c in range(3)] + [np.full((h, w), 2.0, np.float32)]
    assert_planes(list(got), want, what="export then torch op")


# ---- 8. refusals: validation only for foreign memory; data-moving entries with arithmetic-invalid descriptors
def test_refusals(kc, torch):
    from kanter_core_amd import _lib
    L = _lib.load()
    host = np.zeros((64, 64, 4), np.uint8)
    d = _lib.kc_device_image(host.ctypes.data, 64, 64, 4, 0, 0, 256, 0)
    ext = C.c_size_t()
    assert L.kc_device_image_validate(C.byref(d), C.byref(ext)) == KC_ERR_INVALID_ARG
    assert ext.value == 64 * 256
    assert L.kc_last_error()
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), 4 << 20) == 0
    try:
        ok = _lib.kc_device_image(p.value, 256, 4096, 4, 0, 0, 1024, 0)  # exactly the allocation
        assert L.kc_device_image_validate(C.byref(ok), C.byref(ext)) == 0, L.kc_last_error()
        assert ext.value == 4 << 20
        past = _lib.kc_device_image(p.value, 256, 4097, 4, 0, 0, 1024, 0)  # one row past its end
        assert L.kc_device_image_validate(C.byref(past), C.byref(ext)) == KC_ERR_INVALID_ARG
        assert b"allocation" in L.kc_last_error()
    finally:
        hip.hipFree(p)
    t = torch.zeros((8, 8, 4), dtype=torch.float16, device="cuda")
    img = kc.SlotImage.from_planes(synthetic_rgba(SEED_A, 8, 8))
    n0 = launches(kc)
    d = kc.device_image_desc(t)
    assert L.kc_image_to_device(img._h, C.byref(d), kc.DEVICE_SRGB, None) == KC_ERR_UNSUPPORTED
    bad = kc.device_image_desc(t)
    bad.channels = 5
    out = C.c_void_p()
    assert L.kc_image_from_device(C.byref(bad), 0, None, C.byref(out)) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_device(img._h, C.byref(bad), 0, None) == KC_ERR_INVALID_ARG
    assert launches(kc) == n0
    with pytest.raises(ValueError):
        kc.SlotImage.from_torch(torch.zeros((8, 8, 4), dtype=torch.uint8))  # a CPU tensor


# ---- 9. a 4096^2 RGBA round trip on the device = the host path
def test_round_trip_4096_matches_host_path(kc, torch):
    n = 4096
    rng = np.random.default_rng(4096)
    px = rng.integers(0, 256, size=(n, n, 4), dtype=np.uint8)
    px2 = rng.integers(0, 256, size=(n, n, 4), dtype=np.uint8)
    ib = kc.SlotImage.from_u8(px2)
    t = torch.from_numpy(px).cuda()
    dev = kc.mix_process(kc.SlotImage.from_torch(t), ib, kc.MixType.Multiply).to_torch(torch.uint8, srgb=True)
    want = kc.mix_process(kc.SlotImage.from_u8(px), ib, kc.MixType.Multiply).to_u8(True)
    assert np.array_equal(dev.cpu().numpy(), want)
