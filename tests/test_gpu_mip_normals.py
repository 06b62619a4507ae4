"""Normal-map mip chains on the device (KC_MIP_NORMALS, csrc/mip_normals.hip): R, G and B of every level equal
tests/mip_normals_ref.py bit for bit on the f32 words, alpha equals tests/mip_ref.py, in the fused form and under
KC_MIP_PER_LEVEL alike -- at the sizes where each part of the kernels can go wrong (one full tile with the barrier path, partial
tiles with odd levels, a second pyramid launch, levels after one extent has reached 1, no pyramid launch at all, enough tiles for
every XCD), on HeightToNormal results, on vectors that are not unit vectors and on IEEE special values and blocks that reach the
fallback at levels 1, 2 and 3.  Constant and aliased planes, a pending Mix chain, wrapped tensors with a tight pitch; launch and
byte counts; the BC chain in host, device, live-graph and DDS form; the refusals; and the plain rule, which does not move."""
import ctypes as C
import os

import numpy as np
import pytest

import bc_ref
import mip_normals_ref
import mip_ref
from util import SEED_A, SEED_B, assert_planes, bit_equal, synthetic_rgba, wrapped_image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 102, 104
BC_SRGB, MIP_PER_LEVEL, MIP_NORMALS = 1, 2, 32
F = np.float32
SHAPES = [(64, 64), (130, 70), (256, 256), (320, 192), (1, 5), (5, 1), (3, 3), (1, 1), (1024, 512)]  # (w, h)
FLT_MAX = np.finfo(F).max
SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, 3e38, -3e38, FLT_MAX, 0.5, 0.5 + 2.0 ** -24, 0.5 - 2.0 ** -24,
                     0.5 + 2.0 ** -20, 0.5 - 2.0 ** -20], F)
FLAT = (0.5, 0.5, 1.0)  # the fallback texel: the vector (0, 0, 1)


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    return kc


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def L():
    from kanter_core_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ data
def random_planes(w, h, seed=SEED_A):
    return synthetic_rgba(seed, h, w)  # [0, 1): R, G, B are not unit vectors


CELL = 8  # the blocks below sit at the origins of distinct 8 x 8 cells
BLOCK_KINDS = [(1, "cancel"), (2, "cancel"), (3, "cancel"), (1, "half"), (2, "half"), (1, "max"), (2, "max")]


def fallback_blocks(w, h, seed):
    """[(level, x, y, kind)]: aligned blocks of 2^level texels a side -- texel (x, y) of `level` -- that reach the fallback:
    "cancel" = the left half +x, the right half -x in all rows: unit vectors at every level above, their zero sum at `level`, so
    the fallback is taken at levels 1, 2 and 3; "half" = the value 0.5 in the three channels (the zero vector) and "max" =
    FLT_MAX in one channel (its box overflows): the fallback at level 1 in every quad of the block."""
    rng = np.random.default_rng([seed, w, h, 99])
    cells = [(cx, cy) for cy in range((h + CELL - 1) // CELL) for cx in range((w + CELL - 1) // CELL)]
    out = []
    for i, j in enumerate(rng.permutation(len(cells))[:2 * len(BLOCK_KINDS)]):
        level, kind = BLOCK_KINDS[i % len(BLOCK_KINDS)]
        s, (cx, cy) = 1 << level, cells[j]
        if cx * CELL + s <= w and cy * CELL + s <= h:
            out.append((level, cx * CELL // s, cy * CELL // s, kind))
    return out


def special_planes(w, h, seed=7):
    """Four planes of random data with a tenth of the texels from SPECIALS, and fallback_blocks written over R, G, B."""
    planes = []
    for c in range(4):
        rng = np.random.default_rng([seed + c, w, h])
        p = rng.random((h, w), dtype=F)
        hit = rng.random((h, w)) < 0.1
        p[hit] = SPECIALS[rng.integers(0, len(SPECIALS), size=int(hit.sum()))]
        planes.append(p)
    for level, x, y, kind in fallback_blocks(w, h, seed):
        s = 1 << level
        ys, xs = slice(y * s, (y + 1) * s), slice(x * s, (x + 1) * s)
        if kind == "max":
            planes[(x + y) % 3][ys, xs] = FLT_MAX
            continue
        for c in range(3):
            planes[c][ys, xs] = 0.5
        if kind == "cancel":
            planes[0][ys, x * s:x * s + s // 2] = 1.0
            planes[0][ys, x * s + s // 2:(x + 1) * s] = 0.0
    return planes


def height_plane(w, h):
    return np.random.default_rng([5, w, h]).random((h, w), dtype=F)


_REF = {}


def ref_chains(key, planes):
    """[R, G, B (, A)] reference chains of the planes: mip_normals_ref for the first three, mip_ref for alpha; computed once per
    key and shared, read-only."""
    if key not in _REF:
        chains = mip_normals_ref.chain(*planes[:3]) + [mip_ref.chain(p) for p in planes[3:]]
        for ch in chains:
            for l in ch:
                l.setflags(write=False)
        _REF[key] = chains
    return _REF[key]


def check_levels(levels, refs, what):
    """levels: SlotImages; refs: per channel, the reference chain."""
    assert len(levels) == len(refs[0]), what
    for k, img in enumerate(levels):
        h, w = refs[0][k].shape
        assert tuple(img.size()) == (w, h), (what, k)
        got = img.planes()
        assert_planes(got, [r[k] for r in refs], what="%s level %d" % (what, k))
        if k >= 1:
            assert not any(np.isnan(p).any() for p in got[:3]), (what, k)


def check_image(img, refs, what):
    fused, per_level = img.mips(normals=True), img.mips(per_level=True, normals=True)
    check_levels(fused, refs, "%s fused" % (what,))
    check_levels(per_level, refs, "%s per level" % (what,))
    return fused


def plane_const(L, img, ch):
    """(is_const, value, handle) of channel ch"""
    p, is_c, v = C.c_void_p(), C.c_int(), C.c_float()
    assert L.kc_image_plane(img._h, ch, C.byref(p)) == 0
    assert L.kc_plane_is_const(p, C.byref(is_c), C.byref(v)) == 0
    L.kc_plane_release(p)
    return bool(is_c.value), F(v.value), p.value


def const_fold(c, k=1):
    c = F(c)
    with np.errstate(all="ignore"):
        for _ in range(k):
            c = ((c + c) + (c + c)) * F(0.25)
    return c


def const_image(kc, size, values):
    """An RGBA image of four constant planes"""
    return kc.combine_rgba_process([kc.SlotImage.from_value(size, v, False) for v in values])


def chain_texels(w, h, first=0):
    return sum(a * b for a, b in (mip_ref.level_size(w, h, k) for k in range(first, mip_ref.level_count(w, h))))


def counters(kc):
    return [kc.stats_counter(n) for n in ("mip_normals_pyramid", "mip_normals_level", "mip_pyramid", "mip_level")]


# ------------------------------------------------------------------ the bits
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_height_to_normal_chain_equals_the_reference(kc, L, shape):
    w, h = shape
    img = kc.height_to_normal_process(kc.SlotImage.from_planes([height_plane(w, h)]))
    planes = img.planes()
    refs = ref_chains(("h2n", w, h), planes)
    levels = check_image(img, refs, ("h2n", w, h))
    assert levels[0]._h.value == img._h.value  # level 0 is the image itself
    assert len(levels) == kc.mip_level_count(w, h)
    assert all(l.is_rgba() for l in levels)
    assert all(plane_const(L, l, 3)[:2] == (True, F(1.0)) for l in levels)  # the constant alpha stays a constant
    if w >= 64 and h >= 64:  # what the flag is for: the plain chain's vectors get shorter, these do not
        d = np.stack([refs[c][3] for c in range(3)]).astype(np.float64) * 2.0 - 1.0
        assert np.abs(np.sqrt((d * d).sum(axis=0)) - 1.0).max() <= 1e-6
        # without the keyword the same image gives the plain reference
        check_levels(img.mips(), [mip_ref.chain(p) for p in planes], ("h2n plain", w, h))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("data", ["random", "special"])
def test_levels_equal_the_reference(kc, shape, data):
    """Four resident planes: R, G, B by the normals rule, alpha (with NaN and infinities in "special") by the plain one."""
    w, h = shape
    planes = random_planes(w, h) if data == "random" else special_planes(w, h)
    refs = ref_chains((data, w, h), planes)
    check_image(kc.SlotImage.from_planes(planes), refs, (data, w, h))
    if data == "special" and w >= 8 and h >= 8:
        assert any(np.isnan(l).any() for l in refs[3][1:])  # alpha keeps its NaN where the reference has one


def test_the_special_planes_reach_the_fallback_at_three_levels():
    """The data of the test above, in the reference: a "cancel" block's texel is the fallback at its level and the four texels
    above it are not (the fallback is taken at levels 1, 2 and 3, not inherited); "half" and "max" blocks are the fallback in
    every quad of level 1."""
    w, h = 64, 64
    refs = ref_chains(("special", w, h), special_planes(w, h))
    blocks = fallback_blocks(w, h, 7)
    assert {(l, k) for l, _, _, k in blocks} == set(BLOCK_KINDS)
    for level, x, y, kind in blocks:
        if kind == "cancel":
            assert tuple(refs[c][level][y, x] for c in range(3)) == FLAT, (level, x, y, kind)
            above = np.stack([refs[c][level - 1][2 * y:2 * y + 2, 2 * x:2 * x + 2] for c in range(3)], axis=-1).reshape(-1, 3)
            assert not any(tuple(t) == FLAT for t in above), (level, x, y, kind)
        else:
            s = 1 << (level - 1)
            for c in range(3):
                assert (refs[c][1][y * s:(y + 1) * s, x * s:(x + 1) * s] == F(FLAT[c])).all(), (level, x, y, kind, c)


# ------------------------------------------------------------------ planes
def test_one_resident_plane_and_two_constants(kc, L):
    w, h = 130, 70
    r = random_planes(w, h, SEED_B)[0]
    size = kc.Size(w, h)
    img = kc.combine_rgba_process([kc.SlotImage.from_planes([r])] + [kc.SlotImage.from_value(size, v, False) for v in (0.5, 1.0, 0.25)])
    refs = ref_chains(("r-const", w, h), [r, np.full((h, w), 0.5, F), np.full((h, w), 1.0, F), np.full((h, w), 0.25, F)])
    for per_level in (False, True):
        st0 = kc.stats()
        levels = img.mips(per_level=per_level, normals=True)
        st1 = kc.stats()
        check_levels(levels, refs, "r-const per_level=%s" % per_level)
        # one plane read, three written
        assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == 4 * w * h + 12 * chain_texels(w, h, 1)
        for k, lv in enumerate(levels[1:], 1):
            handles = [plane_const(L, lv, ch) for ch in range(3)]
            assert not any(hd[0] for hd in handles), k  # three resident planes
            assert len({hd[2] for hd in handles}) == 3, k
            assert plane_const(L, lv, 3)[:2] == (True, const_fold(0.25, k)), k


@pytest.mark.parametrize("rgb", [(0.8, 0.3, 0.9), (0.5, 0.5, 0.5), (3e38, 0.5, 0.5), (1e-45, 0.5 + 2.0 ** -24, 0.5), (0.5, 0.5, 1.0),
                                 (float("nan"), 0.2, 0.7), (0.25, float("-inf"), 0.5)])
def test_three_constants_are_folded_on_the_host(kc, L, rgb):
    w, h = 37, 21
    img = const_image(kc, kc.Size(w, h), list(rgb) + [0.6])
    n0, c0 = kc.stats()["kernel_launches"], counters(kc)
    levels = img.mips(normals=True)
    assert kc.stats()["kernel_launches"] == n0 and counters(kc) == c0
    assert [tuple(l.size()) for l in levels] == [mip_ref.level_size(w, h, k) for k in range(mip_ref.level_count(w, h))]
    want = [F(v) for v in rgb]
    for k, lv in enumerate(levels):
        if k >= 1:
            want = [x.reshape(()).astype(F) for x in mip_normals_ref.normal_texel(*[const_fold(v) for v in want])]
        for ch in range(3):
            is_c, v, _ = plane_const(L, lv, ch)
            assert is_c and bit_equal(np.array([v]), np.array([want[ch]])), (k, ch, v, want[ch])
        assert plane_const(L, lv, 3)[:2] == (True, const_fold(0.6, k)), k


def test_aliased_planes_are_read_once_and_written_three_times(kc, L):
    w, h = 64, 64
    p = random_planes(w, h, SEED_B)[0]
    rgba = kc.SlotImage.from_planes([p]).materialize().as_type(True)  # [p, p, p, ones]
    refs = ref_chains(("alias", w, h), [p, p, p, np.ones((h, w), F)])
    for per_level in (False, True):
        st0 = kc.stats()
        levels = rgba.mips(per_level=per_level, normals=True)
        st1 = kc.stats()
        assert st1["kernel_launches"] - st0["kernel_launches"] == (6 if per_level else 1)
        assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == 4 * w * h + 12 * chain_texels(w, h, 1)
        check_levels(levels, refs, "alias per_level=%s" % per_level)
        for k, lv in enumerate(levels[1:], 1):
            assert len({plane_const(L, lv, ch)[2] for ch in range(3)}) == 3, k
            assert plane_const(L, lv, 3)[:2] == (True, F(1.0)), k


def test_pending_mix_chain_is_forced(kc):
    w, h = 130, 70
    a, b = special_planes(w, h, 21), random_planes(w, h, SEED_B)
    m = kc.mix_process(kc.SlotImage.from_planes(a), kc.SlotImage.from_planes(b), kc.MixType.Multiply)
    levels = m.mips(normals=True)  # the pending chain runs first
    planes = m.planes()
    refs = mip_normals_ref.chain(*planes[:3]) + [mip_ref.chain(planes[3])]
    check_levels(levels, refs, "mix")
    check_levels(m.mips(per_level=True, normals=True), refs, "mix per level")


@pytest.mark.parametrize("h", [37, 64])
def test_wrapped_tensors_with_a_tight_pitch(kc, torch, h):
    w = 100  # 400 bytes per row, no padding: the second tile's columns 100 .. 127 do not exist
    planes = special_planes(w, h, 3)[:3] + [np.ones((h, w), F)]
    wi = wrapped_image(kc, torch, planes, ["tight", "tight", "tight", ("const", 1.0)], guard=np.nan)
    assert all(t.shape[1] * 4 == 400 for t, _ in wi.parents) and len(wi.parents) == 3
    refs = ref_chains(("wrapped", w, h), planes)
    check_image(wi.image, refs, ("wrapped", w, h))
    wi.assert_untouched()  # the sources are only read


# ------------------------------------------------------------------ handles, counts
@pytest.mark.parametrize("w,h,launches,pyramid", [(64, 64, 1, 1), (256, 256, 2, 2), (130, 70, 2, 1), (1, 5, 2, 0)])
@pytest.mark.parametrize("alpha", ["constant", "resident"])
def test_launches_counters_and_algorithmic_bytes(kc, w, h, launches, pyramid, alpha):
    p = random_planes(w, h)
    if alpha == "constant":
        size = kc.Size(w, h)
        img = kc.combine_rgba_process([kc.SlotImage.from_planes([p[c]]).materialize() for c in range(3)] + [kc.SlotImage.from_value(size, 0.5, False)])
    else:
        img = kc.SlotImage.from_planes(p).materialize()
    groups = 1 if alpha == "constant" else 2  # a resident alpha takes the plain kernels' launches beside the coupled ones
    for per_level in (False, True):
        st0, c0 = kc.stats(), counters(kc)
        img.mips(per_level=per_level, normals=True)
        st1, c1 = kc.stats(), counters(kc)
        want = mip_ref.level_count(w, h) - 1 if per_level else launches
        pyr, lev = (0, want) if per_level else (pyramid, launches - pyramid)
        assert st1["kernel_launches"] - st0["kernel_launches"] == groups * want
        assert [b - a for a, b in zip(c0, c1)] == [pyr, lev] + ([0, 0] if alpha == "constant" else [pyr, lev])
        # 4 w h per distinct resident plane of R, G, B read plus 12 sum W_k H_k written, plus alpha's by the plain rule
        assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == (
            12 * w * h + 12 * chain_texels(w, h, 1) + (4 * chain_texels(w, h) if alpha == "resident" else 0))
        # the same image without the flag takes as many launches for its three (four) planes, all on the plain counters
        st0, c0 = kc.stats(), counters(kc)
        img.mips(per_level=per_level)
        st1, c1 = kc.stats(), counters(kc)
        assert st1["kernel_launches"] - st0["kernel_launches"] == want
        assert [b - a for a, b in zip(c0, c1)] == [0, 0, pyr, lev]  # "mip_normals_*" do not move


def test_references_balance_and_refusals_launch_nothing(kc, L, torch):
    w, h = 130, 70
    img = kc.SlotImage.from_planes(random_planes(w, h)).materialize()
    gray = kc.SlotImage.from_planes(random_planes(w, h)[:1]).materialize()
    kc.sync()
    n = kc.mip_level_count(w, h)
    _, total = kc.bc_mip_layout(w, h, 3)
    t = torch.zeros((total,), dtype=torch.uint8, device="cuda")
    host = np.zeros(total, np.uint8)
    arr, count = (C.c_void_p * n)(), C.c_uint32()
    in_use, n0 = kc.stats()["bytes_in_use"], kc.stats()["kernel_launches"]
    # a Gray image: the count is written, nothing is launched or allocated
    assert L.kc_image_build_mips(gray._h, MIP_NORMALS, arr, n, C.byref(count)) == KC_ERR_INVALID_ARG
    assert count.value == n
    count.value = 0
    assert L.kc_image_build_mips(gray._h, MIP_NORMALS | MIP_PER_LEVEL, arr, n, C.byref(count)) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_mips(gray._h, 4, MIP_NORMALS, host.ctypes.data, total) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_mips_device(gray._h, 4, MIP_NORMALS, t.data_ptr(), total, None) == KC_ERR_INVALID_ARG
    # too small an array
    assert L.kc_image_build_mips(img._h, MIP_NORMALS, arr, n - 1, C.byref(count)) == KC_ERR_INVALID_ARG and count.value == n
    # a vector is not a colour; 4 and 8 stay refused
    for flags in (MIP_NORMALS | BC_SRGB, MIP_NORMALS | 4, MIP_NORMALS | 8, 4, 8):
        assert L.kc_image_build_mips(img._h, flags, arr, n, C.byref(count)) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_to_bc_mips(img._h, 3, flags, host.ctypes.data, total) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_to_bc_mips_device(img._h, 3, flags, t.data_ptr(), total, None) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_write_dds(img._h, b"/nonexistent/x.dds", 3, flags, 1) == KC_ERR_UNSUPPORTED, flags
    assert L.kc_image_to_bc_mips(img._h, 5, MIP_NORMALS | BC_SRGB, host.ctypes.data, total) == KC_ERR_UNSUPPORTED
    assert kc.stats()["kernel_launches"] == n0 and kc.stats()["bytes_in_use"] == in_use
    assert not host.any()
    with pytest.raises(kc.TexProError):
        img.to_bc_mips(3, srgb=True, normals=True)
    with pytest.raises(kc.TexProError):
        gray.mips(normals=True)
    assert kc.stats()["kernel_launches"] == n0
    # the levels hold their planes until they are released
    assert L.kc_image_build_mips(img._h, MIP_NORMALS, arr, n, C.byref(count)) == 0
    assert count.value == n and arr[0] == img._h.value
    assert kc.stats()["bytes_in_use"] > in_use
    for k in range(n):
        assert L.kc_image_release(arr[k]) == 0
    assert kc.stats()["bytes_in_use"] == in_use
    assert tuple(img.size()) == (w, h)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ export
def bc_reference(kc, refs, fmt):
    """bc_ref.encode of to_u8 of each reference level (the reference level goes through the device's quantiser)"""
    return [bc_ref.encode(kc.SlotImage.from_planes([c[k] for c in refs]).to_u8(False), fmt) for k in range(len(refs[0]))]


@pytest.fixture(scope="module")
def normal_map(kc):
    """A HeightToNormal result of 130 x 70, its reference chains and their BC5 and BC3 encodings"""
    w, h = 130, 70
    img = kc.height_to_normal_process(kc.SlotImage.from_planes([height_plane(w, h)]))
    refs = ref_chains(("h2n", w, h), img.planes())
    return img, refs, {fmt: bc_reference(kc, refs, fmt) for fmt in (5, 3)}


@pytest.mark.parametrize("fmt", [5, 3])
def test_bc_chain_equals_bc_ref_of_every_reference_level(kc, torch, normal_map, fmt):
    img, _, want = normal_map
    for per_level in (False, True):
        got = img.to_bc_mips(fmt, per_level=per_level, normals=True)
        assert len(got) == len(want[fmt])
        for k, (g, r) in enumerate(zip(got, want[fmt])):
            assert g.shape == r.shape, (k, g.shape, r.shape)
            assert np.array_equal(g, r), "BC%d level %d differs" % (fmt, k)
    host = np.concatenate([l.reshape(-1) for l in got])
    assert not np.array_equal(host, np.concatenate([l.reshape(-1) for l in img.to_bc_mips(fmt)]))  # the plain chain differs
    offs, total = kc.bc_mip_layout(130, 70, fmt)
    t, got_offs = img.to_bc_mips_torch(fmt, normals=True)
    assert got_offs == offs and t.numel() == total and np.array_equal(t.cpu().numpy(), host)
    big = torch.full((total + 4096,), 0xa5, dtype=torch.uint8, device="cuda")
    out, _ = img.to_bc_mips_torch(fmt, out=big, per_level=True, normals=True)
    assert out is big
    dev = big.cpu().numpy()
    assert np.array_equal(dev[:total], host)
    assert (dev[total:] == 0xa5).all()  # bytes past the chain are untouched


def test_write_dds(kc, normal_map, tmp_path):
    img, _, want = normal_map
    chain = b"".join(l.tobytes() for l in want[5])
    img.write_dds(tmp_path / "normals.dds", "bc5", normals=True)
    assert (tmp_path / "normals.dds").read_bytes() == kc.dds_header(130, 70, 5) + chain
    img.write_dds(tmp_path / "top.dds", "bc5", mips=False, normals=True)  # accepted, and without effect
    assert (tmp_path / "top.dds").read_bytes() == kc.dds_header(130, 70, 5, levels=1) + want[5][0].tobytes()


def test_live_graph_height_to_normal_as_bc5_chain(kc, torch):
    tp = kc.TextureProcessor.new()
    lg = tp.new_live_graph()
    src = lg.add_node(kc.Node.new(kc.NodeType.Image(os.path.join(INPUTS, "clouds.png"))))
    sep = lg.add_node(kc.Node.new(kc.NodeType.SeparateRgba))
    h2n = lg.add_node(kc.Node.new(kc.NodeType.HeightToNormal))
    lg.connect(src, sep, 0, 0)
    lg.connect(sep, h2n, 0, 0)
    lg.await_clean(h2n)
    image = lg.slot_data(h2n, 0).image
    refs = ref_chains("clouds", image.planes())
    want = np.concatenate([l.reshape(-1) for l in bc_reference(kc, refs, 5)])
    got, offs = lg.buffer_bc_mips_torch(h2n, 0, 5, normals=True)
    assert offs == kc.bc_mip_layout(*image.size(), 5)[0]
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(lg.buffer_bc_mips_torch(h2n, 0, 5, per_level=True, normals=True)[0].cpu().numpy(), want)
    assert not np.array_equal(lg.buffer_bc_mips_torch(h2n, 0, 5)[0].cpu().numpy(), want)  # the plain chain is another one
    with pytest.raises(kc.TexProError):
        lg.buffer_bc_mips_torch(h2n, 0, 3, srgb=True, normals=True)
    torch.cuda.synchronize()
