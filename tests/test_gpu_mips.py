"""Mip chains on the device (kc_image_build_mips and its exporters, csrc/mip.*): every level equals tests/mip_ref.py bit for
bit on the f32 words (a NaN where the reference has one), in the fused form and under KC_MIP_PER_LEVEL alike -- at the sizes
where each part of the kernels can go wrong: one full tile, two tiles, partial tiles with odd levels, a second pyramid launch,
levels after one extent has reached 1, no pyramid launch at all, and enough tiles for every XCD.  Gray and RGBA, constant and
aliased planes, a pending Mix chain, a wrapped tensor with a tight pitch, IEEE special values; launch and byte counts; the BC
chain in host, device, live-graph and DDS form against bc_ref of every reference level."""
import ctypes as C
import os

import numpy as np
import pytest

import bc_ref
import mip_ref
from util import SEED_A, SEED_B, assert_planes, bit_equal, synthetic_rgba

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 102, 104
MIP_PER_LEVEL = 2
SHAPES = [(64, 64), (128, 64), (130, 70), (256, 256), (320, 192), (1, 1), (1, 5), (5, 1), (3, 3), (2, 2), (1024, 512)]  # (w, h)
FLT_MAX = np.finfo(np.float32).max
SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 5.877e-39, 1.1754942e-38, FLT_MAX, -FLT_MAX, 3e38],
                    np.float32)


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    return kc


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def random_planes(w, h, n, seed=SEED_A):
    return synthetic_rgba(seed, h, w)[:n]  # [0, 1)


def special_plane(w, h, seed):
    """Random data with special values scattered over a tenth of the texels and filling whole aligned 2 x 2 quads and 4 x 4
    blocks (so that they survive, unmixed, into levels 1 and 2)."""
    rng = np.random.default_rng([seed, w, h])
    p = rng.random((h, w), dtype=np.float32)
    hit = rng.random((h, w)) < 0.1
    p[hit] = SPECIALS[rng.integers(0, len(SPECIALS), size=int(hit.sum()))]
    for i in range(min(64, (h // 2) * (w // 2))):
        y, x = 2 * int(rng.integers(0, h // 2)), 2 * int(rng.integers(0, w // 2))
        p[y:y + 2, x:x + 2] = SPECIALS[i % len(SPECIALS)]
    for i in range(min(24, (h // 4) * (w // 4))):
        y, x = 4 * int(rng.integers(0, h // 4)), 4 * int(rng.integers(0, w // 4))
        p[y:y + 4, x:x + 4] = SPECIALS[(5 * i + 1) % len(SPECIALS)]
    return p


def special_planes(w, h, n):
    return [special_plane(w, h, 7 + c) for c in range(n)]


_REF = {}


def ref_chain(key, plane):
    """mip_ref.chain of a plane, computed once per key and shared (read-only) between the tests."""
    if key not in _REF:
        levels = mip_ref.chain(plane)
        for l in levels:
            l.setflags(write=False)
        _REF[key] = levels
    return _REF[key]


def check_levels(levels, refs, what):
    """levels: SlotImages; refs: per channel, the reference chain."""
    assert len(levels) == len(refs[0]), what
    for k, img in enumerate(levels):
        h, w = refs[0][k].shape
        assert tuple(img.size()) == (w, h), (what, k)
        assert_planes(img.planes(), [r[k] for r in refs], what="%s level %d" % (what, k))


def check_image(kc, planes, key):
    img = kc.SlotImage.from_planes(planes)
    refs = [ref_chain((key, c), p) for c, p in enumerate(planes)]
    fused, per_level = img.mips(), img.mips(per_level=True)
    check_levels(fused, refs, "%s fused" % (key,))
    check_levels(per_level, refs, "%s per level" % (key,))
    return img, fused


# ------------------------------------------------------------------ the bits
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("n", [1, 4], ids=["gray", "rgba"])
@pytest.mark.parametrize("data", ["random", "special"])
def test_levels_equal_the_reference(kc, shape, n, data):
    w, h = shape
    planes = random_planes(w, h, n) if data == "random" else special_planes(w, h, n)
    img, levels = check_image(kc, planes, (data, w, h))
    assert levels[0]._h.value == img._h.value  # level 0 is the image itself
    assert len(levels) == kc.mip_level_count(w, h) == mip_ref.level_count(w, h)
    assert levels[1:] == [] or all(l.is_rgba() == (n == 4) for l in levels)


def const_fold(c, k):
    c = np.float32(c)
    with np.errstate(all="ignore"):
        for _ in range(k):
            c = ((c + c) + (c + c)) * np.float32(0.25)
    return c


def plane_const(L, img, ch):
    """(is_const, value, handle) of channel ch"""
    p, is_c, v = C.c_void_p(), C.c_int(), C.c_float()
    assert L.kc_image_plane(img._h, ch, C.byref(p)) == 0
    assert L.kc_plane_is_const(p, C.byref(is_c), C.byref(v)) == 0
    L.kc_plane_release(p)
    return bool(is_c.value), np.float32(v.value), p.value


@pytest.mark.parametrize("alpha", [0.6, 3e38, -3e38, 1e-45, 4.2e-45, float("inf"), -0.0])
def test_constant_alpha_stays_constant(kc, alpha):
    from kanter_core_amd import _lib
    L = _lib.load()
    w, h = 130, 70
    p = random_planes(w, h, 3, SEED_B)
    img = kc.combine_rgba_process([kc.SlotImage.from_planes([p[0]]), kc.SlotImage.from_planes([p[1]]),
                                   kc.SlotImage.from_planes([p[2]]), kc.SlotImage.from_value(kc.Size(w, h), alpha, False)])
    st0 = kc.stats()
    levels = img.mips()
    st1 = kc.stats()
    refs = [ref_chain(("const", c), p[c]) for c in range(3)]
    texels = sum(r.size for r in refs[0])
    assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == 3 * 4 * texels  # the constant costs nothing
    for k, lv in enumerate(levels):
        is_c, v, _ = plane_const(L, lv, 3)
        want = const_fold(alpha, k)
        assert is_c, k
        assert bit_equal(np.array([v]), np.array([want])), (k, v, want)
        got = lv.planes()
        assert_planes(got[:3], [r[k] for r in refs], what="level %d" % k)
        assert bit_equal(got[3], np.full(refs[0][k].shape, want, np.float32)), k
    # an image of constants launches nothing
    n0 = kc.stats()["kernel_launches"]
    consts = kc.SlotImage.from_value(kc.Size(37, 21), 0.25, True).mips()
    assert kc.stats()["kernel_launches"] == n0
    assert [tuple(c.size()) for c in consts] == [mip_ref.level_size(37, 21, k) for k in range(6)]
    # from_value's alpha is 1
    assert all(plane_const(L, c, ch)[:2] == (True, np.float32(1.0 if ch == 3 else 0.25)) for c in consts for ch in range(4))


def test_aliased_planes_are_reduced_once(kc):
    from kanter_core_amd import _lib
    L = _lib.load()
    w, h = 64, 64
    p = random_planes(w, h, 1, SEED_B)[0]
    gray = kc.SlotImage.from_planes([p]).materialize()
    rgba = gray.as_type(True)  # [p, p, p, ones]
    st0 = kc.stats()
    levels = rgba.mips()
    st1 = kc.stats()
    ref = ref_chain(("alias", 0), p)
    assert st1["kernel_launches"] - st0["kernel_launches"] == 1
    assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == 4 * sum(r.size for r in ref)  # one plane
    for k, lv in enumerate(levels):
        handles = [plane_const(L, lv, ch)[2] for ch in range(3)]
        assert handles[0] == handles[1] == handles[2], k
        assert plane_const(L, lv, 3)[:2] == (True, np.float32(1.0)), k
        assert_planes(lv.planes(), [ref[k]] * 3 + [np.ones(ref[k].shape, np.float32)], what="level %d" % k)


def test_pending_mix_chain_is_forced(kc):
    w, h = 130, 70
    a, b = special_planes(w, h, 4), random_planes(w, h, 4, SEED_B)
    m = kc.mix_process(kc.SlotImage.from_planes(a), kc.SlotImage.from_planes(b), kc.MixType.Multiply)
    levels = m.mips()  # the pending chain runs first
    check_levels(levels, [mip_ref.chain(p) for p in m.planes()], "mix")
    check_levels(m.mips(per_level=True), [mip_ref.chain(p) for p in m.planes()], "mix per level")


@pytest.mark.parametrize("h", [37, 64])
def test_wrapped_tensor_with_a_tight_pitch(kc, torch, h):
    from kanter_core_amd import _lib
    L = _lib.load()
    w = 100  # 400 bytes per row, no padding: the second tile's columns 100 .. 127 do not exist
    p = special_plane(w, h, 3)
    t = torch.from_numpy(p).cuda().contiguous()
    torch.cuda.synchronize()
    plane, img = C.c_void_p(), C.c_void_p()
    assert L.kc_plane_wrap(t.data_ptr(), w, h, 4 * w, C.byref(plane)) == 0
    assert L.kc_image_gray(plane, C.byref(img)) == 0
    L.kc_plane_release(plane)
    src = kc.SlotImage(img.value)
    ref = [mip_ref.chain(p)]
    check_levels(src.mips(), ref, "wrapped")
    check_levels(src.mips(per_level=True), ref, "wrapped per level")
    kc.sync()
    del src
    assert np.array_equal(t.cpu().numpy().view(np.uint32), p.view(np.uint32))  # the source is only read


# ------------------------------------------------------------------ handles, counts
def test_level_zero_is_the_input_and_references_balance(kc):
    from kanter_core_amd import _lib
    L = _lib.load()
    w, h = 130, 70
    img = kc.SlotImage.from_planes(random_planes(w, h, 4)).materialize()
    kc.sync()
    in_use = kc.stats()["bytes_in_use"]
    n = kc.mip_level_count(w, h)
    arr, count = (C.c_void_p * n)(), C.c_uint32()
    # too small an array: the count is written, nothing is launched or allocated
    n0 = kc.stats()["kernel_launches"]
    assert L.kc_image_build_mips(img._h, 0, arr, n - 1, C.byref(count)) == KC_ERR_INVALID_ARG
    assert count.value == n and kc.stats()["kernel_launches"] == n0 and kc.stats()["bytes_in_use"] == in_use
    assert L.kc_image_build_mips(img._h, 4, arr, n, C.byref(count)) == KC_ERR_UNSUPPORTED
    assert L.kc_image_build_mips(img._h, 0, arr, n, C.byref(count)) == 0
    assert count.value == n and arr[0] == img._h.value
    assert kc.stats()["bytes_in_use"] > in_use
    for k in range(n):
        assert L.kc_image_release(arr[k]) == 0
    assert kc.stats()["bytes_in_use"] == in_use
    assert tuple(img.size()) == (w, h)  # the image is still alive: it held its own reference


def chain_texels(w, h):
    return sum(a * b for a, b in (mip_ref.level_size(w, h, k) for k in range(mip_ref.level_count(w, h))))


@pytest.mark.parametrize("w,h,n,launches,pyramid", [(64, 64, 4, 1, 1), (256, 256, 1, 2, 2), (128, 64, 1, 2, 1), (130, 70, 4, 2, 1),
                                                    (320, 192, 1, 3, 2), (1, 5, 1, 2, 0), (3, 3, 4, 1, 1), (1, 1, 1, 0, 0),
                                                    (1024, 512, 4, 3, 2)])
def test_launches_and_algorithmic_bytes(kc, w, h, n, launches, pyramid):
    img = kc.SlotImage.from_planes(random_planes(w, h, n)).materialize()
    for per_level in (False, True):
        st0, p0, l0 = kc.stats(), kc.stats_counter("mip_pyramid"), kc.stats_counter("mip_level")
        img.mips(per_level=per_level)
        st1, p1, l1 = kc.stats(), kc.stats_counter("mip_pyramid"), kc.stats_counter("mip_level")
        want = mip_ref.level_count(w, h) - 1 if per_level else launches
        assert st1["kernel_launches"] - st0["kernel_launches"] == want
        assert (p1 - p0, l1 - l0) == ((0, want) if per_level else (pyramid, launches - pyramid))
        # 4 w h per plane read plus 4 sum W_k H_k per plane written
        assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == (4 * n * chain_texels(w, h) if w * h > 1 else 0)


# ------------------------------------------------------------------ the BC chain
def bc_reference(kc, planes, fmt, srgb):
    """bc_ref.encode of to_u8 of each mip_ref level (the reference level goes through the device's quantiser)"""
    chains = [mip_ref.chain(p) for p in planes]
    return [bc_ref.encode(kc.SlotImage.from_planes([c[k] for c in chains]).to_u8(srgb), fmt) for k in range(len(chains[0]))]


@pytest.fixture(scope="module")
def bc_images(kc):
    out = {}
    for w, h in ((130, 70), (64, 64)):
        rgba, gray = special_planes(w, h, 4), special_planes(w, h, 1)
        out[(w, h, 4)] = (kc.SlotImage.from_planes(rgba), rgba)
        out[(w, h, 1)] = (kc.SlotImage.from_planes(gray), gray)
    return out


@pytest.mark.parametrize("shape", [(130, 70), (64, 64)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fmt,srgb,n", [(1, False, 4), (1, True, 4), (3, False, 4), (4, False, 1), (5, False, 4)])
def test_bc_chain_equals_bc_ref_of_every_level(kc, bc_images, shape, fmt, srgb, n):
    w, h = shape
    img, planes = bc_images[(w, h, n)]
    want = bc_reference(kc, planes, fmt, srgb)
    for per_level in (False, True):
        got = img.to_bc_mips(fmt, srgb, per_level=per_level)
        assert len(got) == len(want)
        for k, (g, r) in enumerate(zip(got, want)):
            assert g.shape == r.shape, (k, g.shape, r.shape)
            assert np.array_equal(g, r), "BC%d srgb=%s level %d differs" % (fmt, srgb, k)
        assert got[1].base is got[0].base  # views of one buffer
    assert np.array_equal(got[0], img.to_bc(fmt, srgb))


def test_device_form_keeps_the_bytes_past_the_chain(kc, torch, bc_images):
    img, _ = bc_images[(130, 70, 4)]
    for fmt, srgb in ((3, True), (1, False)):
        host = np.concatenate([l.reshape(-1) for l in img.to_bc_mips(fmt, srgb)])
        offs, total = kc.bc_mip_layout(130, 70, fmt)
        assert host.size == total
        t, got_offs = img.to_bc_mips_torch(fmt, srgb)
        assert got_offs == offs and t.numel() == total and np.array_equal(t.cpu().numpy(), host)
        big = torch.full((total + 4096,), 0xa5, dtype=torch.uint8, device="cuda")
        out, _ = img.to_bc_mips_torch(fmt, srgb, out=big)
        assert out is big
        got = big.cpu().numpy()
        assert np.array_equal(got[:total], host)
        assert (got[total:] == 0xa5).all()


def test_refusals_launch_nothing(kc, torch, bc_images):
    from kanter_core_amd import _lib
    L = _lib.load()
    img, _ = bc_images[(130, 70, 4)]
    img.materialize()
    _, total = kc.bc_mip_layout(130, 70, 3)
    t = torch.zeros((total,), dtype=torch.uint8, device="cuda")
    host = np.zeros(total, np.uint8)
    n0 = kc.stats()["kernel_launches"]
    assert L.kc_image_to_bc_mips(img._h, 3, 0, host.ctypes.data, total - 1) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_mips_device(img._h, 3, 0, t.data_ptr(), total - 1, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_mips_device(img._h, 3, 0, host.ctypes.data, total, None) == KC_ERR_INVALID_ARG  # a host pointer
    assert L.kc_image_to_bc_mips_device(img._h, 4, 1, t.data_ptr(), total, None) == KC_ERR_UNSUPPORTED
    assert L.kc_image_to_bc_mips_device(img._h, 3, 8, t.data_ptr(), total, None) == KC_ERR_UNSUPPORTED
    assert kc.stats()["kernel_launches"] == n0
    assert not host.any()
    torch.cuda.synchronize()


def test_write_dds(kc, bc_images, tmp_path):
    img, _ = bc_images[(130, 70, 4)]
    chain = b"".join(l.tobytes() for l in img.to_bc_mips(3))
    _, total = kc.bc_mip_layout(130, 70, 3)
    img.write_dds(tmp_path / "chain.dds", 3)
    data = (tmp_path / "chain.dds").read_bytes()
    assert len(data) == 148 + total
    assert data == kc.dds_header(130, 70, 3) + chain
    img.write_dds(tmp_path / "top.dds", "bc1", srgb=True, mips=False)
    assert (tmp_path / "top.dds").read_bytes() == kc.dds_header(130, 70, 1, srgb=True, levels=1) + img.to_bc(1, True).tobytes()


def test_live_graph_slot_as_bc_chain(kc, torch):
    tp = kc.TextureProcessor.new()
    lg = tp.new_live_graph()
    src = lg.add_node(kc.Node.new(kc.NodeType.Image(os.path.join(INPUTS, "heart_110.png"))))
    sep = lg.add_node(kc.Node.new(kc.NodeType.SeparateRgba))
    lg.connect(src, sep, 0, 0)
    lg.await_clean(sep)
    image = lg.slot_data(sep, 1).image
    for fmt, srgb in ((4, False), (1, True)):
        want = np.concatenate([l.reshape(-1) for l in image.to_bc_mips(fmt, srgb)])
        got, offs = lg.buffer_bc_mips_torch(sep, 1, fmt, srgb)
        assert offs == kc.bc_mip_layout(*image.size(), fmt)[0]
        assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(kc.TexProError):
        lg.buffer_bc_mips_torch(sep, 9, 4)  # no such slot
    torch.cuda.synchronize()
