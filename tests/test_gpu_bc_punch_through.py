"""BC1 with punch-through alpha on the device (KC_BC_PUNCH_THROUGH, csrc/bc1a.hip): the blocks are bc1a_ref.encode of the RGBA8
bytes kc_image_to_u8 writes, byte for byte -- all three block classes, edge-case floats, edge blocks, the grid-stride loop,
constant alpha on both sides of the threshold, wrapped planes with padding -- through every entry point that takes the flag:
the host and device forms, the error measure, the chains and DDS files, a live graph; and refusals launch nothing."""
import ctypes as C

import numpy as np
import pytest

import bc1a_ref as R
import bc_ref
from util import MIXED, SEED_A, SEED_B, synthetic_rgba, with_edge_cases, wrapped_image

pytestmark = pytest.mark.gpu

KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 102, 104
REFS = [1, 128, 255]
SHAPES = [(1, 1), (4, 4), (3, 5), (13, 17), (129, 257)]


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


def planes(kc, h, w, ref, seed=SEED_A):
    """Edge-case colour planes and bc1a_ref.class_alpha's alpha for the byte `ref`"""
    p = [with_edge_cases(q * 1.2 - 0.1, shift=c) for c, q in enumerate(synthetic_rgba(seed, h, w)[:3])]
    return p + [R.class_alpha(h, w, kc.alpha_ref_threshold(ref), seed)]


_images = {}


def image(kc, h, w, ref):
    """One resident image per (shape, byte), shared by the tests and never changed"""
    if (h, w, ref) not in _images:
        _images[h, w, ref] = kc.SlotImage.from_planes(planes(kc, h, w, ref)).materialize()
    return _images[h, w, ref]


def check(img, ref, srgb, got):
    px = img.to_u8(srgb)
    want = R.encode(px, ref)
    assert got.shape == want.shape and got.dtype == np.uint8, (got.shape, want.shape)
    bad = np.argwhere((got != want).any(-1))
    assert bad.size == 0, "B=%d srgb=%s: %d blocks differ, first %s: %s vs %s" % (
        ref, srgb, len(bad), bad[0], got[tuple(bad[0])].tobytes().hex(), want[tuple(bad[0])].tobytes().hex())
    return px


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("ref", REFS)
def test_bytes_equal_the_reference(kc, ref, srgb, shape):
    h, w = shape
    img = image(kc, h, w, ref)
    px = check(img, ref, srgb, img.to_bc(1, srgb, punch_through=ref))
    if h * w > 100:  # from 4 x 5 blocks on, every class is there: empty, mixed and full blocks, edge blocks included
        assert min(R.class_counts(px, ref)) > 0, R.class_counts(px, ref)


@pytest.mark.parametrize("option,value", [("tune_cap", 2), ("cache_budget_mb", 0)])
def test_grid_stride_loop(kc, option, value):
    """Capped at two workgroups, 512 threads, the 2145 blocks of 129 x 257 take five rounds, the last partly out of range (the
    sRGB forms: a thread's first block before the loop, the others in it); cache_budget_mb = 0: the same in the nontemporal
    instantiations"""
    img = image(kc, 129, 257, 128)
    saved = {o: kc.get_option(o) for o in ("tune_cap", option)}
    try:
        kc.set_option("tune_cap", 2)
        kc.set_option(option, value)
        got = [img.to_bc(1, srgb, punch_through=128) for srgb in (False, True)]
        err = img.bc_error(1, True, punch_through=128)
    finally:
        for o, v in saved.items():
            kc.set_option(o, v)
    for srgb, g in zip((False, True), got):
        check(img, 128, srgb, g)
    sse, mx = R.error_sums(img.to_u8(True), got[1], 128)
    assert np.array_equal(err.sse, sse.astype(np.uint64)) and np.array_equal(err.max_abs, mx.astype(np.uint32))


def test_constant_alpha_and_the_counters(kc):
    h, w, ref = 30, 42, 128
    bx, by = (w + 3) // 4, (h + 3) // 4
    rgb = planes(kc, h, w, ref)[:3]
    r_b = kc.alpha_ref_threshold(ref)

    def with_alpha(v):
        one = lambda p: kc.SlotImage.from_planes([p])
        return kc.combine_rgba_process([one(rgb[0]), one(rgb[1]), one(rgb[2]), kc.value_process(float(v))])  # alpha stays a constant plane

    opaque = with_alpha(1.0)
    assert np.array_equal(opaque.to_bc(1, punch_through=ref), opaque.to_bc(1))
    assert np.array_equal(with_alpha(r_b).to_bc(1, True, punch_through=ref), opaque.to_bc(1, True))  # r_B is at the byte
    for v in (0.0, np.nextafter(r_b, np.float32(0))):  # and the float below it is not
        assert (with_alpha(v).to_bc(1, punch_through=ref) == R.EMPTY).all(), v
    resident = kc.SlotImage.from_planes(rgb + [R.class_alpha(h, w, r_b)]).materialize()
    for img, n_planes in ((resident, 4), (opaque, 3), (kc.SlotImage.from_value(kc.Size(w, h), 0.5, True), 0)):
        st0 = kc.stats()
        img.to_bc(1, punch_through=ref)
        st1 = kc.stats()
        assert st1["kernel_launches"] - st0["kernel_launches"] == 1
        assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == w * h * 4 * n_planes + bx * by * 8, n_planes
        img.bc_error(1, punch_through=ref)
        st2 = kc.stats()
        assert st2["kernel_launches"] - st1["kernel_launches"] == 3  # the encode, then the comparison's two
        assert st2["algorithmic_bytes"] - st1["algorithmic_bytes"] == 2 * (w * h * 4 * n_planes + bx * by * 8), n_planes


@pytest.mark.parametrize("w", [9, 10, 11, 12])
def test_wrapped_planes_with_padding(kc, torch, w):
    h, ref = 19, 128
    wi = wrapped_image(kc, torch, planes(kc, h, w, ref, SEED_B), MIXED, float("nan"))
    for srgb in (False, True):
        px = check(wi.image, ref, srgb, wi.image.to_bc(1, srgb, punch_through=ref))
        err = wi.image.bc_error(1, srgb, punch_through=ref)
        sse, mx = R.error_sums(px, R.encode(px, ref), ref)
        assert np.array_equal(err.sse, sse.astype(np.uint64))
    wi.assert_untouched()


@pytest.mark.parametrize("srgb", [False, True])
def test_device_form_equals_host_form_and_keeps_padding(kc, torch, srgb):
    h, w, ref = 13, 17, 128
    img = image(kc, h, w, ref)
    host = img.to_bc(1, srgb, punch_through=ref)
    assert np.array_equal(img.to_bc_torch(1, srgb, punch_through=ref).cpu().numpy(), host)
    by, bx, bb = host.shape
    big = torch.full((by + 3, bx + 5, bb), 0xa5, dtype=torch.uint8, device="cuda")
    img.to_bc_torch(1, srgb, out=big[1:1 + by, 2:2 + bx, :], punch_through=ref)
    expect = np.full(tuple(big.shape), 0xa5, np.uint8)
    expect[1:1 + by, 2:2 + bx, :] = host
    assert np.array_equal(big.cpu().numpy(), expect)


@pytest.mark.parametrize("ref", REFS)
def test_round_trip_keeps_the_alpha_test(kc, ref):
    h, w = 129, 257
    img = image(kc, h, w, ref)
    dec = kc.SlotImage.from_bc(img.to_bc(1, punch_through=ref), w, h, 1)
    alpha = dec.planes()[3]
    assert np.array_equal(alpha == 1.0, img.to_u8()[..., 3] >= ref) and set(np.unique(alpha)) <= {0.0, 1.0}
    assert dec.alpha_coverage(1) == img.alpha_coverage(ref)


@pytest.mark.parametrize("srgb", [False, True])
def test_the_error_measure(kc, torch, srgb):
    h, w, ref = 129, 257, 128
    img = image(kc, h, w, ref)
    px = img.to_u8(srgb)
    blk = R.encode(px, ref)
    err = img.bc_error(1, srgb, punch_through=ref)
    sse, mx = R.error_sums(px, blk, ref)
    assert err.format == 1 and err.channel_mask == 0xF and err.pixels == w * h and err.undecoded_blocks == 0
    assert err.flags == kc.bc_punch_through_ref(ref) | (kc.BC_SRGB if srgb else 0)
    assert np.array_equal(err.sse, sse.astype(np.uint64)) and np.array_equal(err.max_abs, mx.astype(np.uint32))
    assert err.sse[3] == 0 and sse[:3].sum() > 0
    # blocks cut at another byte: covered pixels that decode transparent (64) and the reverse (200)
    for other in (64, 200):
        foreign = R.encode(px, other)
        got = img.bc_error(1, srgb, blocks=torch.from_numpy(foreign).cuda(), punch_through=ref)
        sse, mx = R.error_sums(px, foreign, ref)
        assert sse[3] > 0 and mx[3] == 255
        assert np.array_equal(got.sse, sse.astype(np.uint64)) and np.array_equal(got.max_abs, mx.astype(np.uint32)), other
    # without the flag the measure is what it was: alpha masked out, every pixel counted
    plain = img.bc_error(1, srgb, blocks=torch.from_numpy(blk).cuda())
    assert plain.channel_mask == 0x7 and plain.sse[3] == 0 and plain.sse[:3].sum() > err.sse[:3].sum()


def cutout(kc, w, h, ref):
    return kc.SlotImage.from_planes(planes(kc, h, w, ref, SEED_B)).materialize()


@pytest.mark.parametrize("size", [(37, 21), (64, 64)])
@pytest.mark.parametrize("kw", [dict(coverage=128, punch_through=True), dict(punch_through=128),
                                dict(alpha_weighted=True, punch_through=128), dict(coverage=128, alpha_weighted=True, punch_through=128)],
                         ids=["coverage", "plain", "alpha_weighted", "both"])
def test_chains_and_dds(kc, tmp_path, size, kw):
    w, h = size
    ref, srgb = 128, True
    img = cutout(kc, w, h, ref)
    chain_kw = {k: v for k, v in kw.items() if k != "punch_through"}
    levels = img.mips(**chain_kw)
    want = [R.encode(lv.to_u8(srgb), ref) for lv in levels]
    got = img.to_bc_mips(1, srgb, **kw)
    assert len(got) == len(want)
    for k, (g, wnt) in enumerate(zip(got, want)):
        assert np.array_equal(g, wnt), (k, kw)
    flat = np.concatenate([g.reshape(-1) for g in got])
    assert np.array_equal(np.concatenate([g.reshape(-1) for g in img.to_bc_mips(1, srgb, per_level=True, **kw)]), flat)
    t, offs = img.to_bc_mips_torch(1, srgb, **kw)
    assert np.array_equal(t.cpu().numpy(), flat)
    assert np.array_equal(np.concatenate([g.reshape(-1) for g in kc.levels_to_bc_mips(levels, 1, srgb, punch_through=ref)]), flat)
    # the files: an ordinary BC1 file whose levels decode to the reference's pixels
    a, b, c = (str(tmp_path / n) for n in ("a.dds", "b.dds", "c.dds"))
    img.write_dds(a, 1, srgb, **kw)
    kc.write_dds_levels(b, levels, 1, srgb, punch_through=ref)
    assert open(a, "rb").read() == open(b, "rb").read() == kc.dds_header(w, h, 1, srgb) + flat.tobytes()
    for k, lv in enumerate(levels):
        s = lv.size()
        assert np.array_equal(kc.SlotImage.read_dds(a, k).to_u8(), R.decode(want[k], s.height, s.width)), k
    img.write_dds(c, 1, srgb, mips=False, **kw)  # the chain flags have no effect without mips: the image itself, cut at the byte
    assert open(c, "rb").read() == kc.dds_header(w, h, 1, srgb, levels=1) + R.encode(img.to_u8(srgb), ref).tobytes()


def test_through_a_live_graph(kc, torch):
    w, h, ref = 37, 21, 128
    img = cutout(kc, w, h, ref)
    tp = kc.TextureProcessor.new()
    lg = tp.new_live_graph()
    lg.embed_slot_data_with_id(kc.SlotData(0, 0, img), 0)
    n = lg.add_node(kc.Node.new(kc.NodeType.Embed(0)))
    lg.await_clean(n)
    assert np.array_equal(lg.buffer_bc_torch(n, 0, 1, True, punch_through=ref).cpu().numpy(), img.to_bc(1, True, punch_through=ref))
    t, offs = lg.buffer_bc_mips_torch(n, 0, 1, coverage=ref, punch_through=True)
    assert np.array_equal(t.cpu().numpy(), np.concatenate([g.reshape(-1) for g in img.to_bc_mips(1, coverage=ref, punch_through=True)]))
    a, b = lg.buffer_bc_error(n, 0, 1, punch_through=ref), img.bc_error(1, punch_through=ref)
    assert np.array_equal(a.sse, b.sse) and a.channel_mask == 0xF
    torch.cuda.synchronize()


def test_pending_mix_chain_is_forced(kc):
    h, w, ref = 45, 67, 128
    m = kc.mix_process(kc.SlotImage.from_planes(planes(kc, h, w, ref, SEED_A)), kc.SlotImage.from_planes(planes(kc, h, w, ref, SEED_B)),
                       kc.MixType.Multiply)
    got = m.to_bc(1, True, punch_through=ref)  # the pending chain runs first
    check(m, ref, True, got)


def test_refusals_launch_nothing_and_write_nothing(kc, torch):
    from kanter_core_amd import _lib
    L = _lib.load()
    ref = 128
    pt = kc.bc_punch_through_ref(ref)
    img = image(kc, 13, 17, ref)
    gray = kc.SlotImage.from_planes([planes(kc, 13, 17, ref)[0]]).materialize()
    kc.sync()
    by, bx = 4, 5
    buf = np.full(by * bx * 8 * 2, 0xa5, np.uint8)
    t = torch.full((by, bx, 8), 0xa5, dtype=torch.uint8, device="cuda")
    t16 = torch.full((by, bx, 16), 0xa5, dtype=torch.uint8, device="cuda")
    err = _lib.kc_bc_error()
    ok = _lib.kc_bc_image(t.data_ptr(), 17, 13, 1, bx * 8)
    torch.cuda.synchronize()
    n0 = launches(kc)
    # a Gray image
    assert L.kc_image_to_bc(gray._h, 1, pt, buf.ctypes.data, buf.nbytes) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_device(gray._h, C.byref(ok), pt, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_bc_error(gray._h, 1, pt, C.byref(err)) == KC_ERR_INVALID_ARG
    assert L.kc_image_bc_compare(gray._h, C.byref(ok), pt, C.byref(err)) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_mips(gray._h, 1, pt, buf.ctypes.data, buf.nbytes) == KC_ERR_INVALID_ARG
    assert L.kc_image_levels_to_bc_mips((C.c_void_p * 1)(gray._h.value), 1, 1, pt, buf.ctypes.data, buf.nbytes) == KC_ERR_INVALID_ARG
    # the illegal words
    d3 = _lib.kc_bc_image(t16.data_ptr(), 17, 13, 3, bx * 16)
    for fmt, flags, d in [(3, pt, d3), (1, kc.BC_PUNCH_THROUGH, ok), (1, ref << 24, ok), (1, pt | kc.MIP_NORMALS, ok), (1, pt | 8, ok)]:
        assert L.kc_image_to_bc(img._h, fmt, flags, buf.ctypes.data, buf.nbytes) == KC_ERR_UNSUPPORTED, (fmt, flags)
        assert L.kc_image_to_bc_device(img._h, C.byref(d), flags, None) == KC_ERR_UNSUPPORTED, (fmt, flags)
        assert L.kc_image_to_bc_mips(img._h, fmt, flags, buf.ctypes.data, buf.nbytes) == KC_ERR_UNSUPPORTED, (fmt, flags)
        assert L.kc_image_bc_error(img._h, fmt, flags, C.byref(err)) == KC_ERR_UNSUPPORTED, (fmt, flags)
    with pytest.raises(ValueError):
        img.to_bc_mips(1, coverage=128, punch_through=127)
    # a short buffer, and a descriptor of another size
    assert L.kc_image_to_bc(img._h, 1, pt, buf.ctypes.data, by * bx * 8 - 1) == KC_ERR_INVALID_ARG
    other = _lib.kc_bc_image(t.data_ptr(), 16, 13, 1, bx * 8)
    assert L.kc_image_to_bc_device(img._h, C.byref(other), pt, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_bc_compare(img._h, C.byref(other), pt, C.byref(err)) == KC_ERR_INVALID_ARG
    assert launches(kc) == n0
    torch.cuda.synchronize()
    assert (buf == 0xa5).all() and (t.cpu().numpy() == 0xa5).all() and (t16.cpu().numpy() == 0xa5).all()
    assert L.kc_image_to_bc_device(img._h, C.byref(ok), pt, None) == 0
    assert launches(kc) == n0 + 1
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), img.to_bc(1, punch_through=ref))
