"""Alpha-test coverage in mip chains on the device (KC_MIP_COVERAGE, csrc/mip_coverage.hip): alpha of every level of
mips(coverage=B) equals tests/mip_coverage_ref.py bit for bit on the f32 words, R, G and B equal the plain chain, and
mip_coverage_info -- targets, plain counts, the selected key and the scale -- equals the reference, which tells a selection error
from a scaling error.  Sizes at which each path can go wrong (one workgroup per level, rows that end inside a quad, levels after
one extent has reached 1, a 1 x 1 image, levels that span many workgroups), masks with heavy ties, IEEE special values, the floor
of the scale; constant, aliased and caller-owned alpha planes; the property the flag is there for; KC_MIP_PER_LEVEL and
KC_MIP_NORMALS beside it; the BC chain in host, device, live-graph and DDS form; launches, bytes, the pool; the refusals."""
import ctypes as C

import numpy as np
import pytest

import mip_coverage_ref as R
import mip_normals_ref
import mip_ref
from util import SEED_A, SEED_B, assert_planes, bit_equal, synthetic_rgba, wrapped_image

pytestmark = pytest.mark.gpu

KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 102, 104
BC_SRGB, MIP_PER_LEVEL, MIP_NORMALS, MIP_COVERAGE, BC7 = 1, 2, 32, 64, 98
F = np.float32
SHAPES = [(64, 64), (130, 70), (256, 256), (320, 192), (1, 5), (5, 1), (3, 3), (1, 1), (1024, 512)]  # (w, h)
REFS = [1, 85, 128, 255]
KINDS = ["noise", "dots", "lines", "zeros", "ones", "range", "special", "tiny"]
SEEDED = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, 1e-40, 2.0 ** -17, 2.0 ** -16, 1.0, 2.0], F)
COVERAGE_LAUNCHES = 7  # three counts, three picks, one scale: whatever the level count


def cov(b):
    return MIP_COVERAGE | b << 24


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
def lines_mask(w, h):
    a = np.zeros((h, w), F)
    a[::7, :] = 1.0
    a[:, ::5] = 1.0
    return a


def dots_mask(w, h, share=0.3):
    return (np.random.default_rng([17, w, h]).random((h, w)) < share).astype(F)


def alpha_plane(kind, w, h):
    rng = np.random.default_rng([23, w, h, KINDS.index(kind)])
    if kind == "noise":
        return rng.random((h, w), dtype=F)
    if kind == "dots":
        return dots_mask(w, h)
    if kind == "lines":
        return lines_mask(w, h)
    if kind == "zeros":
        return np.zeros((h, w), F)
    if kind == "ones":
        return np.ones((h, w), F)
    if kind == "range":
        return rng.random((h, w), dtype=F) * F(3.0) - F(1.0)  # [-1, 2)
    if kind == "tiny":
        # under the floor of ve, except the last two rows and columns: where a level drops them (an odd extent above it) the
        # target stays above zero while every value of the level lies under the floor
        p = rng.random((h, w), dtype=F) * F(1e-5)
        p[-2:, :] = 1.0
        p[:, -2:] = 1.0
        return p
    p = rng.random((h, w), dtype=F)  # "special"
    hit = rng.random((h, w)) < 0.1
    p[hit] = SEEDED[rng.integers(0, len(SEEDED), size=int(hit.sum()))]
    p.reshape(-1)[:len(SEEDED)] = SEEDED[:p.size]
    return p


_REF = {}


def ref_chain(key, alpha, ref):
    """(levels, info) of mip_coverage_ref.chain, computed once per key and shared, read-only."""
    k = (key, ref)
    if k not in _REF:
        levels, info = R.chain(alpha, ref)
        for l in levels:
            l.setflags(write=False)
        _REF[k] = (levels, info)
    return _REF[k]


def plain_chains(key, planes):
    k = (key, "plain")
    if k not in _REF:
        _REF[k] = [mip_ref.chain(p) for p in planes]
    return _REF[k]


def check_info(got, want, what):
    assert len(got) == len(want), what
    for k, (g, r) in enumerate(zip(got, want)):
        assert (g.texels, g.target, g.plain_covered) == (r.texels, r.target, r.plain_covered), (what, k, g, r)  # the selection's inputs
        assert g.v.view(np.uint32) == r.v.view(np.uint32), (what, k, "the selected key", g, r)
        assert g.scale.view(np.uint32) == r.scale.view(np.uint32), (what, k, "the scale", g, r)


def check_levels(levels, rgb_refs, alpha_ref, what):
    """levels: SlotImages; rgb_refs: the reference chains of R, G, B; alpha_ref: the stored alpha levels."""
    assert len(levels) == len(alpha_ref), what
    for k, img in enumerate(levels):
        h, w = alpha_ref[k].shape
        assert tuple(img.size()) == (w, h), (what, k)
        assert_planes(img.planes(), [r[k] for r in rgb_refs] + [alpha_ref[k]], what="%s level %d" % (what, k))


def rgba_with(alpha, seed=SEED_A):
    h, w = alpha.shape
    return synthetic_rgba(seed, h, w)[:3] + [alpha]


def plane_handle(L, img, ch):
    p, is_c, v = C.c_void_p(), C.c_int(), C.c_float()
    assert L.kc_image_plane(img._h, ch, C.byref(p)) == 0
    assert L.kc_plane_is_const(p, C.byref(is_c), C.byref(v)) == 0
    L.kc_plane_release(p)
    return bool(is_c.value), F(v.value), p.value


def chain_texels(w, h, first=0):
    return sum(a * b for a, b in (mip_ref.level_size(w, h, k) for k in range(first, mip_ref.level_count(w, h))))


# ------------------------------------------------------------------ the bits
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_levels_and_info_equal_the_reference(kc, shape, kind):
    w, h = shape
    planes = rgba_with(alpha_plane(kind, w, h))
    img = kc.SlotImage.from_planes(planes)
    rgb = plain_chains(("rgb", w, h), planes[:3])
    scaled = 0
    for ref in REFS:
        want, info = ref_chain((kind, w, h), planes[3], ref)
        levels = img.mips(coverage=ref)
        assert levels[0]._h.value == img._h.value  # level 0 is the image itself
        check_info(img.mip_coverage_info(ref), info, (kind, w, h, ref))
        check_levels(levels, rgb, want, (kind, w, h, ref))
        scaled += sum(i.scale != F(1.0) for i in info)
        if kind in ("zeros", "ones"):  # a fully empty or fully opaque texture never changes
            assert all(i.scale == F(1.0) for i in info)
            check_levels(levels, rgb, mip_ref.chain(planes[3]), (kind, w, h, ref, "plain"))
    if kind in ("noise", "dots", "lines", "range", "special") and w >= 64 and h >= 64:
        assert scaled > 0  # the case reaches the select and the scale


def test_the_special_plane_keeps_its_nan_and_its_zeros(kc):
    w, h = 130, 70
    a = alpha_plane("special", w, h)
    want, info = ref_chain(("special", w, h), a, 128)
    assert any(np.isnan(l).any() for l in want[1:]) and any(i.scale != F(1.0) for i in info)
    tiny, tinfo = ref_chain(("tiny", w, h), alpha_plane("tiny", w, h), 128)
    big = [i for i in tinfo[1:] if i.scale != F(1.0) and i.v < R.FLOOR]
    assert big and all(np.isfinite(i.scale) and i.scale == R.threshold(128) / R.FLOOR for i in big)  # the floor of ve


# ------------------------------------------------------------------ planes
def test_a_constant_alpha_launches_nothing_and_stays_constant(kc, L):
    w, h = 130, 70
    p = synthetic_rgba(SEED_B, h, w)
    for value in (0.6, 0.3, float("nan")):
        img = kc.combine_rgba_process([kc.SlotImage.from_planes([p[c]]).materialize() for c in range(3)]
                                      + [kc.SlotImage.from_value(kc.Size(w, h), value, False)])
        st0 = kc.stats()
        plain = img.mips()
        st1 = kc.stats()
        levels = img.mips(coverage=128)
        st2 = kc.stats()
        assert st2["kernel_launches"] - st1["kernel_launches"] == st1["kernel_launches"] - st0["kernel_launches"]
        assert st2["algorithmic_bytes"] - st1["algorithmic_bytes"] == st1["algorithmic_bytes"] - st0["algorithmic_bytes"]
        c = F(value)
        n0 = w * h
        c0 = n0 if R.quant_u8(c) >= 128 else 0
        info = img.mip_coverage_info(128)
        assert kc.stats()["kernel_launches"] == st2["kernel_launches"]  # answered on the host
        for k, (lv, pl) in enumerate(zip(levels, plain)):
            if k:
                with np.errstate(all="ignore"):
                    c = ((c + c) + (c + c)) * F(0.25)
            is_c, v, _ = plane_handle(L, lv, 3)
            assert is_c and bit_equal(np.array([v]), np.array([c])), (value, k)
            assert_planes(lv.planes()[:3], pl.planes()[:3], what="constant alpha level %d" % k)
            n_k = lv.size().width * lv.size().height
            want = R.Level(n_k, c0 if k == 0 else R.target(n0, n_k, c0), n_k if R.quant_u8(c) >= 128 else 0, F(0.0), F(1.0))
            check_info([info[k]], [want], ("constant", value, k))


def test_alpha_that_aliases_red_gets_planes_of_its_own(kc, L):
    w, h = 130, 70
    a = dots_mask(w, h)
    p = synthetic_rgba(SEED_B, h, w)
    shared = kc.SlotImage.from_planes([a]).materialize()
    img = kc.combine_rgba_process([shared, kc.SlotImage.from_planes([p[1]]).materialize(), kc.SlotImage.from_planes([p[2]]).materialize(), shared])
    assert plane_handle(L, img, 0)[2] == plane_handle(L, img, 3)[2]
    want, info = ref_chain(("dots", w, h), a, 128)
    assert any(i.scale != F(1.0) for i in info)
    rgb = [mip_ref.chain(x) for x in (a, p[1], p[2])]
    for per_level in (False, True):
        levels = img.mips(per_level=per_level, coverage=128)
        check_levels(levels, rgb, want, "alias per_level=%s" % per_level)  # R's levels stay plain, alpha's differ
        for k, lv in enumerate(levels[1:], 1):
            assert plane_handle(L, lv, 0)[2] != plane_handle(L, lv, 3)[2], k
    check_info(img.mip_coverage_info(128), info, "alias")


@pytest.mark.parametrize("layout", ["tight", "pad48", "offset"])
def test_a_caller_owned_alpha_with_poisoned_padding(kc, torch, layout):
    w, h = 101, 37  # rows end inside a quad: the three floats behind them and the padding are NaN, which would count as covered
    planes = rgba_with(alpha_plane("noise", w, h) * F(0.4))
    wi = wrapped_image(kc, torch, planes, ["tight", "tight", "tight", layout], guard=np.nan)
    rgb = [mip_ref.chain(p) for p in planes[:3]]
    for ref in (85, 1):
        want, info = ref_chain(("wrapped", w, h), planes[3], ref)
        check_info(wi.image.mip_coverage_info(ref), info, (layout, ref))
        check_levels(wi.image.mips(coverage=ref), rgb, want, (layout, ref))
    wi.assert_untouched()


# ------------------------------------------------------------------ what the flag is for
@pytest.mark.parametrize("mask", ["lines", "dots"])
def test_coverage_is_kept_where_the_plain_chain_loses_it(kc, mask):
    w = h = 256
    a = lines_mask(w, h) if mask == "lines" else dots_mask(w, h)
    img = kc.SlotImage.from_planes(rgba_with(a))
    plain, kept = img.mips(), img.mips(coverage=128)
    info = img.mip_coverage_info(128)
    c0 = img.alpha_coverage(128)
    assert c0 == R.covered(a, 128) == info[0].target
    share = [lv.alpha_coverage(128) / (lv.size().width * lv.size().height) for lv in plain]
    print("%s: plain coverage %s" % (mask, ["%.3f" % s for s in share]))
    assert share[2] < 0.5 * share[0]
    plain_alpha = mip_ref.chain(a)
    for k in range(1, len(kept)):
        i = info[k]
        ck = kept[k].alpha_coverage(128)
        if i.scale == F(1.0):
            assert ck == i.plain_covered, k
            continue
        assert i.v >= R.FLOOR
        upper = int((R.key(plain_alpha[k]).astype(np.float64) >= float(i.v) * (1.0 - 2.0 ** -20)).sum())
        print("%s level %d: target %d covered %d upper %d" % (mask, k, i.target, ck, upper))
        assert i.target <= ck <= upper, (k, i, ck, upper)


def test_per_level_and_normals_give_the_same_alpha(kc):
    w, h = 130, 70
    planes = rgba_with(alpha_plane("noise", w, h))
    img = kc.SlotImage.from_planes(planes)
    want, info = ref_chain(("noise", w, h), planes[3], 85)
    rgb = plain_chains(("rgb", w, h), planes[:3])
    check_levels(img.mips(per_level=True, coverage=85), rgb, want, "per level")
    normals = mip_normals_ref.chain(*planes[:3])
    check_levels(img.mips(normals=True, coverage=85), normals, want, "normals")
    check_levels(img.mips(per_level=True, normals=True, coverage=85), normals, want, "normals per level")
    check_levels(img.mips(), rgb, mip_ref.chain(planes[3]), "the plain chain does not move")


# ------------------------------------------------------------------ export
@pytest.fixture(scope="module")
def cutout(kc):
    w, h = 130, 70
    return kc.SlotImage.from_planes(rgba_with(dots_mask(w, h) * alpha_plane("noise", w, h))).materialize()


@pytest.mark.parametrize("fmt", [3, BC7])
def test_bc_chain_equals_to_bc_of_every_level(kc, torch, cutout, fmt, tmp_path):
    w, h = cutout.size()
    ref = 128
    want = [lv.to_bc(fmt) for lv in cutout.mips(coverage=ref)]
    got = cutout.to_bc_mips(fmt, coverage=ref)
    assert len(got) == len(want)
    for k, (g, r) in enumerate(zip(got, want)):
        assert g.shape == r.shape and np.array_equal(g, r), (fmt, k)
    host = np.concatenate([l.reshape(-1) for l in want])
    assert not np.array_equal(host, np.concatenate([l.reshape(-1) for l in cutout.to_bc_mips(fmt)]))  # the plain chain differs
    offs, total = kc.bc_mip_layout(w, h, fmt)
    t, got_offs = cutout.to_bc_mips_torch(fmt, coverage=ref)
    assert got_offs == offs and t.numel() == total and np.array_equal(t.cpu().numpy(), host)
    t, _ = cutout.to_bc_mips_torch(fmt, per_level=True, coverage=ref)
    assert np.array_equal(t.cpu().numpy(), host)
    # the live-graph form
    tp = kc.TextureProcessor.new()
    lg = tp.new_live_graph()
    lg.embed_slot_data_with_id(kc.SlotData(0, 0, cutout), 0)
    n = lg.add_node(kc.Node.new(kc.NodeType.Embed(0)))
    lg.await_clean(n)
    t, got_offs = lg.buffer_bc_mips_torch(n, 0, fmt, coverage=ref)
    assert got_offs == offs and np.array_equal(t.cpu().numpy(), host)
    # the file, read back level by level
    path = tmp_path / "cutout.dds"
    cutout.write_dds(path, fmt, coverage=ref)
    assert path.read_bytes() == kc.dds_header(w, h, fmt) + host.tobytes()
    for k, lv in enumerate(cutout.mips(coverage=ref)):
        back = kc.SlotImage.read_dds(path, level=k)
        assert np.array_equal(back.to_u8(False), kc.SlotImage.from_bc(want[k], *lv.size(), fmt).to_u8(False)), (fmt, k)
    top = tmp_path / "top.dds"
    cutout.write_dds(top, fmt, mips=False, coverage=ref)  # accepted, and without effect
    assert top.read_bytes() == kc.dds_header(w, h, fmt, levels=1) + want[0].tobytes()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ launches, bytes, the pool, refusals
@pytest.mark.parametrize("shape", [(64, 64), (1024, 512)], ids=lambda s: "%dx%d" % s)
def test_launches_and_algorithmic_bytes(kc, shape):
    w, h = shape
    img = kc.SlotImage.from_planes(rgba_with(dots_mask(w, h))).materialize()
    below = chain_texels(w, h, 1)
    for per_level in (False, True):
        st0, c0 = kc.stats(), kc.stats_counter("mip_coverage")
        img.mips(per_level=per_level)
        st1 = kc.stats()
        img.mips(per_level=per_level, coverage=128)
        st2, c2 = kc.stats(), kc.stats_counter("mip_coverage")
        plain_launches = st1["kernel_launches"] - st0["kernel_launches"]
        assert st2["kernel_launches"] - st1["kernel_launches"] == plain_launches + COVERAGE_LAUNCHES
        assert c2 - c0 == COVERAGE_LAUNCHES
        # level 0's alpha once, every further level once per pass and once for the scale, and written once
        assert (st2["algorithmic_bytes"] - st1["algorithmic_bytes"]) - (st1["algorithmic_bytes"] - st0["algorithmic_bytes"]) == 4 * w * h + 20 * below
    gray = kc.SlotImage.from_planes([dots_mask(w, h)]).materialize()
    st0 = kc.stats()
    gray.mips()
    st1 = kc.stats()
    img.mip_coverage_info(128)  # alpha's plain chain and the select, no scale
    st2 = kc.stats()
    assert st2["kernel_launches"] - st1["kernel_launches"] == st1["kernel_launches"] - st0["kernel_launches"] + COVERAGE_LAUNCHES - 1
    assert st2["algorithmic_bytes"] - st1["algorithmic_bytes"] == 4 * chain_texels(w, h) + 4 * w * h + 12 * below


def test_a_1x1_image_launches_nothing(kc):
    img = kc.SlotImage.from_planes([np.full((1, 1), v, F) for v in (0.1, 0.2, 0.3, 0.7)]).materialize()
    n0 = kc.stats()["kernel_launches"]
    levels = img.mips(coverage=128)
    assert len(levels) == 1 and kc.stats()["kernel_launches"] == n0
    check_info(img.mip_coverage_info(128), [R.Level(1, 1, 1, F(0.0), F(1.0))], "1x1")


def test_the_pool_balances_and_refusals_launch_nothing(kc, L, torch):
    w, h = 130, 70
    img = kc.SlotImage.from_planes(rgba_with(alpha_plane("noise", w, h))).materialize()
    gray = kc.SlotImage.from_planes([alpha_plane("noise", w, h)]).materialize()
    kc.sync()
    from kanter_core_amd import _lib
    n = kc.mip_level_count(w, h)
    _, total = kc.bc_mip_layout(w, h, 3)
    t = torch.zeros((total,), dtype=torch.uint8, device="cuda")
    host = np.zeros(total, np.uint8)
    arr, count = (C.c_void_p * n)(), C.c_uint32()
    recs = (_lib.kc_mip_coverage_level * n)()
    in_use, n0 = kc.stats()["bytes_in_use"], kc.stats()["kernel_launches"]
    # a Gray image: the count is written, nothing is launched or allocated
    assert L.kc_image_build_mips(gray._h, cov(128), arr, n, C.byref(count)) == KC_ERR_INVALID_ARG and count.value == n
    count.value = 0
    assert L.kc_image_mip_coverage_info(gray._h, cov(128), recs, n, C.byref(count)) == KC_ERR_INVALID_ARG and count.value == n
    assert L.kc_image_to_bc_mips(gray._h, 4, cov(128), host.ctypes.data, total) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_mips_device(gray._h, 4, cov(128), t.data_ptr(), total, None) == KC_ERR_INVALID_ARG
    # too small an array
    assert L.kc_image_build_mips(img._h, cov(128), arr, n - 1, C.byref(count)) == KC_ERR_INVALID_ARG and count.value == n
    assert L.kc_image_mip_coverage_info(img._h, cov(128), recs, n - 1, C.byref(count)) == KC_ERR_INVALID_ARG and count.value == n
    # the bad flag words
    for flags in (MIP_COVERAGE, 128 << 24, cov(128) | 4, cov(128) | 8, cov(128) | 16, cov(128) | MIP_NORMALS | BC_SRGB):
        assert L.kc_image_build_mips(img._h, flags, arr, n, C.byref(count)) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_to_bc_mips(img._h, 3, flags, host.ctypes.data, total) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_to_bc_mips_device(img._h, 3, flags, t.data_ptr(), total, None) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_write_dds(img._h, b"/nonexistent/x.dds", 3, flags, 1) == KC_ERR_UNSUPPORTED, flags
        assert L.kc_image_mip_coverage_info(img._h, flags, recs, n, C.byref(count)) == KC_ERR_UNSUPPORTED, flags
    assert kc.stats()["kernel_launches"] == n0 and kc.stats()["bytes_in_use"] == in_use
    assert not host.any()
    with pytest.raises(kc.TexProError):
        gray.mips(coverage=128)
    with pytest.raises(ValueError):
        img.mips(coverage=0)
    assert kc.stats()["kernel_launches"] == n0
    # the scratch goes back to the pool with the call; the levels hold their planes until they are released
    img.mip_coverage_info(128)
    assert kc.stats()["bytes_in_use"] == in_use
    assert L.kc_image_build_mips(img._h, cov(128), arr, n, C.byref(count)) == 0
    assert count.value == n and arr[0] == img._h.value
    held = kc.stats()["bytes_in_use"]
    assert held > in_use
    for k in range(n):
        assert L.kc_image_release(arr[k]) == 0
    assert kc.stats()["bytes_in_use"] == in_use
    # the plain alpha nothing aliases is scratch: a chain with the flag holds no more than the plain chain
    assert L.kc_image_build_mips(img._h, 0, arr, n, C.byref(count)) == 0
    assert kc.stats()["bytes_in_use"] == held
    for k in range(n):
        assert L.kc_image_release(arr[k]) == 0
    assert kc.stats()["bytes_in_use"] == in_use
    torch.cuda.synchronize()
