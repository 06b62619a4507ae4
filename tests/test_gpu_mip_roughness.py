"""Roughness mip chains on the device (kc_image_build_roughness_mips, csrc/mip_roughness.hip): every level of the named channel
equals tests/mip_roughness_ref.py bit for bit on the f32 words, the other channels equal tests/mip_ref.py, in the fused form and
under KC_MIP_PER_LEVEL alike -- at the sizes where each part of the kernels can go wrong (one full tile with the barrier path,
partial tiles with odd levels, a second pyramid launch that reads the state planes, levels after one extent has reached 1, no
pyramid launch at all, enough tiles for every XCD), on HeightToNormal results, on vectors that are not unit vectors, on IEEE
special values in all four planes and on blocks whose normals cancel at levels 1, 2 and 3.  Gray and RGBA images, the image as
its own normal map, constant and aliased planes, a pending Mix chain, wrapped tensors with a tight pitch; launch and byte counts;
the exporters of a chain the caller holds; the refusals."""
import ctypes as C

import numpy as np
import pytest

import mip_ref
import mip_roughness_ref as ref
from util import SEED_A, SEED_B, assert_planes, bit_equal, synthetic_rgba, wrapped_image

pytestmark = pytest.mark.gpu

KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 102, 104
MIP_PER_LEVEL = 2
BC4, BC7 = 4, 98
F = np.float32
SHAPES = [(64, 64), (130, 70), (256, 256), (320, 192), (1, 5), (5, 1), (3, 3), (1, 1), (1024, 512)]  # (w, h)
FLT_MAX = np.finfo(F).max
SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, 3e38, -3e38, FLT_MAX, 0.5, 0.5 + 2.0 ** -24, 0.5 - 2.0 ** -24,
                     1.0, 1.25, -0.25], F)
COUNTERS = ("mip_roughness_pyramid", "mip_roughness_level", "mip_pyramid", "mip_level")


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
def height_plane(w, h):
    return np.random.default_rng([5, w, h]).random((h, w), dtype=F)


def rough_plane(w, h, seed=11):
    return np.random.default_rng([seed, w, h]).random((h, w), dtype=F)


CELL = 8  # the cancel blocks sit at the origins of distinct 8 x 8 cells


def cancel_blocks(w, h, seed):
    """[(level, x, y)]: aligned blocks of 2^level texels a side -- texel (x, y) of `level` -- whose left half is +x and whose
    right half is -x in all rows: unit vectors at every level above, their zero sum at `level`, where the texel is exactly 1."""
    rng = np.random.default_rng([seed, w, h, 99])
    cells = [(cx, cy) for cy in range((h + CELL - 1) // CELL) for cx in range((w + CELL - 1) // CELL)]
    out = []
    for i, j in enumerate(rng.permutation(len(cells))[:6]):
        level = 1 + i % 3
        s, (cx, cy) = 1 << level, cells[j]
        if cx * CELL + s <= w and cy * CELL + s <= h:
            out.append((level, cx * CELL // s, cy * CELL // s))
    return out


def special_planes(w, h, seed=7):
    """Four planes of random data with a tenth of the texels from SPECIALS, and cancel_blocks written over R, G, B (alpha, the
    roughness, is finite there: 0.25)."""
    planes = []
    for c in range(4):
        rng = np.random.default_rng([seed + c, w, h])
        p = rng.random((h, w), dtype=F)
        hit = rng.random((h, w)) < 0.1
        p[hit] = SPECIALS[rng.integers(0, len(SPECIALS), size=int(hit.sum()))]
        planes.append(p)
    for level, x, y in cancel_blocks(w, h, seed):
        s = 1 << level
        ys = slice(y * s, (y + 1) * s)
        planes[1][ys, x * s:(x + 1) * s] = 0.5
        planes[2][ys, x * s:(x + 1) * s] = 0.5
        planes[0][ys, x * s:x * s + s // 2] = 1.0
        planes[0][ys, x * s + s // 2:(x + 1) * s] = 0.0
        planes[3][ys, x * s:(x + 1) * s] = 0.25
    return planes


_REF = {}


def cached(key, make):
    """A reference chain (or a list of them), computed once per key and shared, read-only."""
    if key not in _REF:
        got = make()
        for lv in (got if isinstance(got[0], np.ndarray) else [l for ch in got for l in ch]):
            lv.setflags(write=False)
        _REF[key] = got
    return _REF[key]


def floor_log2(v):
    return v.bit_length() - 1


def walk(w, h, per_level):
    """(launches, pyramid launches, the levels whose four boxes go through state planes) of the chain's level walk."""
    n, k, launches, pyramids, state = mip_ref.level_count(w, h), 0, 0, 0, []
    while k + 1 < n:
        small = min(mip_ref.level_size(w, h, k))
        fused = 0 if per_level or small < 2 else min(6, floor_log2(small))
        k += fused or 1
        launches += 1
        pyramids += 1 if fused else 0
        if k + 1 < n:
            state.append(k)
    return launches, pyramids, state


def texels(w, h, levels):
    return sum(a * b for a, b in (mip_ref.level_size(w, h, k) for k in levels))


def chain_texels(w, h, first=0):
    return texels(w, h, range(first, mip_ref.level_count(w, h)))


def roughness_bytes(w, h, per_level, distinct):
    """kc_stats_algorithmic_bytes of the coupled launches: `distinct` resident planes read, one plane per level written, the state
    planes written and read."""
    return 4 * w * h * distinct + 4 * chain_texels(w, h, 1) + 32 * texels(w, h, walk(w, h, per_level)[2])


def counters(kc):
    return [kc.stats_counter(n) for n in COUNTERS]


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


def check_levels(levels, refs, what):
    """levels: SlotImages; refs: per channel, the reference chain."""
    assert len(levels) == len(refs[0]), what
    for k, img in enumerate(levels):
        h, w = refs[0][k].shape
        assert tuple(img.size()) == (w, h), (what, k)
        assert_planes(img.planes(), [r[k] for r in refs], what="%s level %d" % (what, k))


def check_image(img, normals, channel, power, refs, what):
    fused = img.roughness_mips(normals, channel, power)
    check_levels(fused, refs, "%s fused" % (what,))
    check_levels(img.roughness_mips(normals, channel, power, per_level=True), refs, "%s per level" % (what,))
    assert fused[0]._h.value == img._h.value  # level 0 is the image itself
    return fused


# ------------------------------------------------------------------ the bits
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_gray_roughness_beside_a_height_to_normal_result(kc, L, shape):
    w, h = shape
    normals = kc.height_to_normal_process(kc.SlotImage.from_planes([height_plane(w, h)]))
    rho = rough_plane(w, h)
    img = kc.SlotImage.from_planes([rho]).materialize()
    X, Y, Z, _ = normals.planes()
    want = cached(("h2n", w, h), lambda: ref.chain(rho, X, Y, Z, 1.0))
    n0, c0 = kc.stats()["kernel_launches"], counters(kc)
    levels = check_image(img, normals, 0, 1.0, [want], ("h2n", w, h))
    assert len(levels) == kc.mip_level_count(w, h) and not any(l.is_rgba() for l in levels)
    if (w, h) == (1, 1):
        assert kc.stats()["kernel_launches"] == n0 and counters(kc) == c0  # nothing launched
    if w >= 64 and h >= 64:  # what the chain is for: rougher than the plain one, which the same image still gives
        plain = mip_ref.chain(rho)
        assert float(want[3].mean()) > float(plain[3].mean()) + 1e-3
        check_levels(img.mips(), [plain], ("h2n plain", w, h))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("power", [2.0 ** -10, 65536.0])
def test_channel_one_of_an_rgba_image_beside_vectors_that_are_not_unit(kc, shape, power):
    """An ORM texture: roughness in G; R, B and A follow the plain rule."""
    w, h = shape
    orm, nrm = synthetic_rgba(SEED_A, h, w), synthetic_rgba(SEED_B, h, w)
    want = cached(("orm", w, h, power), lambda: [ref.chain(orm[1], nrm[0], nrm[1], nrm[2], power) if c == 1 else mip_ref.chain(orm[c]) for c in range(4)])
    check_image(kc.SlotImage.from_planes(orm), kc.SlotImage.from_planes(nrm), 1, power, want, ("orm", w, h, power))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_image_as_its_own_normal_map_with_special_values(kc, shape):
    """Roughness in the normal map's alpha; a tenth of the texels of all four planes are special values."""
    w, h = shape
    p = special_planes(w, h)
    want = cached(("special", w, h), lambda: [mip_ref.chain(p[c]) for c in range(3)] + [ref.chain(p[3], p[0], p[1], p[2], 1.0)])
    img = kc.SlotImage.from_planes(p)
    check_image(img, img, 3, 1.0, want, ("special", w, h))
    if w >= 8 and h >= 8:
        assert any(np.isnan(l).any() for l in want[3][1:])  # the roughness keeps its NaN where the plain box has one


def test_the_special_planes_cancel_at_three_levels():
    """The data of the test above, in the reference: a cancel block's texel is exactly 1 at its level, and is not at the level
    above (the normals cancel at levels 1, 2 and 3: it is not inherited)."""
    w, h = 64, 64
    p = special_planes(w, h)
    want = cached(("special", w, h), lambda: [mip_ref.chain(p[c]) for c in range(3)] + [ref.chain(p[3], p[0], p[1], p[2], 1.0)])[3]
    blocks = cancel_blocks(w, h, 7)
    assert {l for l, _, _ in blocks} == {1, 2, 3}
    for level, x, y in blocks:
        assert want[level][y, x] == F(1.0), (level, x, y)
        if level > 1:
            assert (want[level - 1][2 * y:2 * y + 2, 2 * x:2 * x + 2] == F(0.25)).all(), (level, x, y)


# ------------------------------------------------------------------ planes
def test_a_constant_roughness_beside_resident_normals(kc, L):
    w, h = 130, 70
    normals = kc.height_to_normal_process(kc.SlotImage.from_planes([height_plane(w, h)]))
    X, Y, Z, _ = normals.planes()
    img = kc.SlotImage.from_value(kc.Size(w, h), 0.3, False)
    want = cached(("const-rho", w, h), lambda: ref.chain(np.full((h, w), 0.3, F), X, Y, Z, 1.0))
    for per_level in (False, True):
        st0 = kc.stats()
        levels = img.roughness_mips(normals, per_level=per_level)
        st1 = kc.stats()
        check_levels(levels, [want], "const rho per_level=%s" % per_level)
        assert not any(plane_const(L, lv, 0)[0] for lv in levels[1:])  # a new resident plane at every level
        assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == roughness_bytes(w, h, per_level, 3)


@pytest.mark.parametrize("rgb", [(0.8, 0.3, 0.9), (0.5, 0.5, 0.5), (float("nan"), 0.2, 0.7)])
def test_constant_normals_are_the_plain_chain_and_launch_nothing_new(kc, L, rgb):
    w, h = 130, 70
    normals = kc.combine_rgba_process([kc.SlotImage.from_value(kc.Size(w, h), v, False) for v in list(rgb) + [1.0]])
    p = synthetic_rgba(SEED_B, h, w)
    img = kc.SlotImage.from_planes(p).materialize()
    want = cached(("plain", w, h), lambda: [mip_ref.chain(c) for c in p])
    for per_level in (False, True):
        c0, st0 = counters(kc), kc.stats()
        levels = img.roughness_mips(normals, 2, 4.0, per_level=per_level)
        c1, st1 = counters(kc), kc.stats()
        launches = walk(w, h, per_level)
        assert [b - a for a, b in zip(c0, c1)] == [0, 0, launches[1], launches[0] - launches[1]]
        assert st1["kernel_launches"] - st0["kernel_launches"] == launches[0]
        check_levels(levels, want, "constant normals per_level=%s" % per_level)
    # a constant roughness too: every level a folded constant, nothing launched at all
    gray = kc.SlotImage.from_value(kc.Size(w, h), 0.3, False)
    n0 = kc.stats()["kernel_launches"]
    levels = gray.roughness_mips(normals)
    assert kc.stats()["kernel_launches"] == n0
    assert [plane_const(L, lv, 0)[:2] for lv in levels] == [(True, const_fold(0.3, k)) for k in range(len(levels))]


def test_an_aliased_image_gets_a_plane_of_its_own_for_the_named_channel(kc, L):
    w, h = 64, 64
    p = rough_plane(w, h, 3)
    rgba = kc.SlotImage.from_planes([p]).materialize().as_type(True)  # [p, p, p, ones]
    normals = kc.height_to_normal_process(kc.SlotImage.from_planes([height_plane(w, h)]))
    X, Y, Z, _ = normals.planes()
    plain = mip_ref.chain(p)
    want = cached(("alias", w, h), lambda: [plain, ref.chain(p, X, Y, Z, 1.0), plain, mip_ref.chain(np.ones((h, w), F))])
    for per_level in (False, True):
        st0 = kc.stats()
        levels = rgba.roughness_mips(normals, 1, per_level=per_level)
        st1 = kc.stats()
        check_levels(levels, want, "alias per_level=%s" % per_level)
        assert st1["kernel_launches"] - st0["kernel_launches"] == 2 * (6 if per_level else 1)  # the coupled walk and the plain one of p
        # X, Y, Z and p read by the coupled launches; p once more, and its chain written, by the plain ones
        assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == roughness_bytes(w, h, per_level, 4) + 4 * chain_texels(w, h)
        for k, lv in enumerate(levels[1:], 1):
            handles = [plane_const(L, lv, ch)[2] for ch in range(3)]
            assert handles[0] == handles[2] != handles[1], k  # R and B still alias; G is its own plane
            assert plane_const(L, lv, 3)[:2] == (True, F(1.0)), k


@pytest.mark.parametrize("pending", ["image", "normals"])
def test_pending_mix_chains_are_forced(kc, pending):
    w, h = 130, 70
    a, b = synthetic_rgba(SEED_A, h, w), synthetic_rgba(SEED_B, h, w)
    mixed = kc.mix_process(kc.SlotImage.from_planes(a), kc.SlotImage.from_planes(b), kc.MixType.Multiply)
    other = kc.SlotImage.from_planes(special_planes(w, h, 21))
    img, normals = (mixed, other) if pending == "image" else (other, mixed)
    levels = img.roughness_mips(normals, 0, 2.0)  # the pending chain runs first
    p, n = img.planes(), normals.planes()
    want = [ref.chain(p[0], n[0], n[1], n[2], 2.0)] + [mip_ref.chain(c) for c in p[1:]]
    check_levels(levels, want, "mix %s" % pending)
    check_levels(img.roughness_mips(normals, 0, 2.0, per_level=True), want, "mix %s per level" % pending)


@pytest.mark.parametrize("h", [37, 64])
def test_wrapped_tensors_with_a_tight_pitch(kc, torch, h):
    w = 100  # 400 bytes per row, no padding: the second tile's columns 100 .. 127 do not exist
    n = special_planes(w, h, 3)[:3] + [np.ones((h, w), F)]
    rho = rough_plane(w, h, 5)
    wn = wrapped_image(kc, torch, n, ["tight", "tight", "tight", ("const", 1.0)], guard=np.nan)
    wr = wrapped_image(kc, torch, [rho], "tight", guard=np.nan)
    assert all(t.shape[1] * 4 == 400 for t, _ in wn.parents + wr.parents)
    want = cached(("wrapped", w, h), lambda: ref.chain(rho, n[0], n[1], n[2], 1.0))
    check_image(wr.image, wn.image, 0, 1.0, [want], ("wrapped", w, h))
    wn.assert_untouched()  # the sources are only read
    wr.assert_untouched()


# ------------------------------------------------------------------ counts
@pytest.mark.parametrize("w,h,launches,pyramid", [(64, 64, 1, 1), (256, 256, 2, 2), (130, 70, 2, 1), (1, 5, 2, 0), (1024, 512, 3, 2)])
@pytest.mark.parametrize("kind", ["gray", "rgba"])
def test_launches_counters_and_algorithmic_bytes(kc, w, h, launches, pyramid, kind):
    normals = kc.SlotImage.from_planes(synthetic_rgba(SEED_B, h, w)).materialize()
    p = synthetic_rgba(SEED_A, h, w)
    img = kc.SlotImage.from_planes(p[:1] if kind == "gray" else p).materialize()
    others = 0 if kind == "gray" else 3  # resident channels beside the named one: the plain kernels' launches
    for per_level in (False, True):
        assert walk(w, h, False)[:2] == (launches, pyramid)
        want = mip_ref.level_count(w, h) - 1 if per_level else launches
        pyr, lev = (0, want) if per_level else (pyramid, launches - pyramid)
        st0, c0 = kc.stats(), counters(kc)
        img.roughness_mips(normals, 0, per_level=per_level)
        st1, c1 = kc.stats(), counters(kc)
        assert st1["kernel_launches"] - st0["kernel_launches"] == want * (2 if others else 1)
        assert [b - a for a, b in zip(c0, c1)] == [pyr, lev] + ([pyr, lev] if others else [0, 0])
        assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == roughness_bytes(w, h, per_level, 4) + 4 * chain_texels(w, h) * others
        # the plain chain of the same image: as many launches, none of them on the new counters
        st0, c0 = kc.stats(), counters(kc)
        img.mips(per_level=per_level)
        st1, c1 = kc.stats(), counters(kc)
        assert st1["kernel_launches"] - st0["kernel_launches"] == want
        assert [b - a for a, b in zip(c0, c1)] == [0, 0, pyr, lev]


# ------------------------------------------------------------------ a chain the caller holds
@pytest.mark.parametrize("fmt", [BC4, BC7])
@pytest.mark.parametrize("kind", ["gray", "rgba"])
def test_levels_of_a_plain_chain_encode_as_to_bc_mips_does(kc, fmt, kind):
    w, h = 130, 70
    p = synthetic_rgba(SEED_A, h, w)
    img = kc.SlotImage.from_planes(p[:1] if kind == "gray" else p).materialize()
    srgb = fmt == BC7
    want = img.to_bc_mips(fmt, srgb=srgb)
    levels = img.mips()
    got = kc.levels_to_bc_mips(levels, fmt, srgb=srgb)
    assert len(got) == len(want) == len(levels)
    for k, (g, r) in enumerate(zip(got, want)):
        assert g.shape == r.shape and np.array_equal(g, r), "level %d differs" % k
    first = kc.levels_to_bc_mips(levels[:3], fmt, srgb=srgb)  # the first levels alone
    assert len(first) == 3 and all(np.array_equal(g, r) for g, r in zip(first, want))


def test_write_dds_levels_of_a_roughness_chain(kc, tmp_path):
    w, h = 130, 70
    normals = kc.height_to_normal_process(kc.SlotImage.from_planes([height_plane(w, h)]))
    levels = kc.SlotImage.from_planes([rough_plane(w, h)]).roughness_mips(normals)
    blocks = kc.levels_to_bc_mips(levels, "bc4")
    assert [b.shape for b in blocks] == [b.shape for b in levels[0].to_bc_mips("bc4")]
    for k, lv in enumerate(levels):
        assert np.array_equal(blocks[k], lv.to_bc("bc4")), k  # the encoder of to_bc on the level as it stands
    assert not np.array_equal(blocks[3], levels[0].to_bc_mips("bc4")[3])  # the plain chain is another one
    path = tmp_path / "roughness.dds"
    kc.write_dds_levels(path, levels, "bc4")
    assert path.read_bytes() == kc.dds_header(w, h, BC4) + b"".join(b.tobytes() for b in blocks)
    for k, b in enumerate(blocks):
        lw, lh = mip_ref.level_size(w, h, k)
        got, info = kc.SlotImage.read_dds(path, level=k, return_info=True)
        assert tuple(got.size()) == (lw, lh) and info.levels == len(levels)
        assert_planes(got.planes(), kc.SlotImage.from_bc(b, lw, lh, "bc4").planes(), what="level %d" % k)
    kc.write_dds_levels(tmp_path / "top.dds", levels[:2], "bc4")
    assert (tmp_path / "top.dds").read_bytes() == kc.dds_header(w, h, BC4, levels=2) + blocks[0].tobytes() + blocks[1].tobytes()


# ------------------------------------------------------------------ refusals
def test_references_balance_and_refusals_launch_nothing(kc, L, tmp_path):
    w, h = 130, 70
    p = synthetic_rgba(SEED_A, h, w)
    img = kc.SlotImage.from_planes(p).materialize()
    gray = kc.SlotImage.from_planes(p[:1]).materialize()
    other = kc.SlotImage.from_planes(synthetic_rgba(SEED_A, h, w + 1)).materialize()
    kc.sync()
    n = kc.mip_level_count(w, h)
    arr, count = (C.c_void_p * n)(), C.c_uint32()
    build = L.kc_image_build_roughness_mips
    one = C.c_float(1.0)
    in_use, n0 = kc.stats()["bytes_in_use"], kc.stats()["kernel_launches"]

    def refused(*args):
        count.value = 0
        assert build(*args, arr, n, C.byref(count)) == KC_ERR_INVALID_ARG, args
        assert count.value == n  # the count is written
    refused(img._h, 0, gray._h, one, 0)              # the normal map must be RGBA
    refused(gray._h, 0, gray._h, one, MIP_PER_LEVEL)
    refused(img._h, 0, other._h, one, 0)             # no implicit resize
    refused(gray._h, 1, img._h, one, 0)              # a Gray image has channel 0 alone
    refused(img._h, 4, img._h, one, 0)
    assert build(img._h, 0, img._h, one, 0, arr, n - 1, C.byref(count)) == KC_ERR_INVALID_ARG and count.value == n
    count.value = 0
    for flags in (1, 4, 8, 32, 64, 64 | 128 << 24):  # KC_MIP_PER_LEVEL only
        assert build(img._h, 0, img._h, one, flags, arr, n, C.byref(count)) == KC_ERR_UNSUPPORTED, flags
    for power in (0.0, -1.0, float("nan"), float("inf"), 65537.0):
        assert build(img._h, 0, img._h, C.c_float(power), 0, arr, n, C.byref(count)) == KC_ERR_INVALID_ARG, power
    assert count.value == 0  # those are refused before the image is looked at
    with pytest.raises(kc.TexProError):
        img.roughness_mips(gray)
    with pytest.raises(kc.TexProError):
        img.roughness_mips(img, power=0.0)
    # the exporters of a chain the caller holds
    levels = img.mips()
    glevels = gray.mips()
    kc.sync()
    held, n1 = kc.stats()["bytes_in_use"], kc.stats()["kernel_launches"]
    _, total = kc.bc_mip_layout(w, h, BC4)
    host = np.zeros(total, np.uint8)
    to_bc, dds = L.kc_image_levels_to_bc_mips, L.kc_image_levels_write_dds
    path = str(tmp_path / "never.dds").encode()

    def handles(images):
        return (C.c_void_p * len(images))(*[i._h.value if i is not None else None for i in images])
    # levels out of order, a level left out, another kind, a NULL level, more levels than the chain has
    for bad in ([levels[1], levels[0]], [levels[0], levels[2]], [levels[0], glevels[1]], [levels[0], None], levels + [levels[-1]]):
        assert to_bc(handles(bad), len(bad), BC4, 0, host.ctypes.data, total) == KC_ERR_INVALID_ARG
        assert dds(handles(bad), len(bad), path, BC4, 0) == KC_ERR_INVALID_ARG
    del bad
    assert to_bc(handles(levels), n, BC4, 0, host.ctypes.data, total - 1) == KC_ERR_INVALID_ARG
    assert to_bc(handles(levels), n, BC4, 1, host.ctypes.data, total) == KC_ERR_UNSUPPORTED  # sRGB is not for BC4
    assert to_bc(handles(levels), n, BC4, MIP_PER_LEVEL, host.ctypes.data, total) == KC_ERR_UNSUPPORTED
    assert kc.stats()["kernel_launches"] == n1 and kc.stats()["bytes_in_use"] == held
    assert not host.any() and not (tmp_path / "never.dds").exists()
    with pytest.raises(ValueError):
        kc.levels_to_bc_mips([], BC4)
    del levels, glevels
    assert kc.stats()["kernel_launches"] == n1 and n1 - n0 == 2 * walk(w, h, False)[0]  # the two plain chains above, nothing else
    # the levels hold their planes until they are released
    assert kc.stats()["bytes_in_use"] == in_use
    assert build(img._h, 2, img._h, one, 0, arr, n, C.byref(count)) == 0
    assert count.value == n and arr[0] == img._h.value
    assert kc.stats()["bytes_in_use"] > in_use
    for k in range(n):
        assert L.kc_image_release(arr[k]) == 0
    assert kc.stats()["bytes_in_use"] == in_use  # the state planes went back to the pool with the call
    assert tuple(img.size()) == (w, h)
