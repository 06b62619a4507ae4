"""Alpha-weighted mip chains on the device (KC_MIP_ALPHA_WEIGHT, csrc/mip_alpha.hip): R, G and B of every level, level 0 included,
equal tests/mip_alpha_ref.py bit for bit on the f32 words, and alpha equals tests/mip_ref.py (tests/mip_coverage_ref.py when the
two flags combine), in the fused form and under KC_MIP_PER_LEVEL alike -- at the sizes where each part of the kernels can go
wrong (one full tile with the barrier path; partial tiles, odd levels and a dropped last column and row; a second pyramid launch
that reads the state planes, under a push whose ancestor walk crosses that boundary; levels after one extent has reached 1; no
pyramid launch at all; enough tiles for every XCD), under masks that are binary, fractional, a single texel, empty, full, and
full of IEEE special values.  Constant and aliased planes, a pending Mix chain, wrapped tensors with a tight pitch; launch and
byte counts; the exporters; the refusals."""
import ctypes as C

import numpy as np
import pytest

import mip_alpha_ref as ref
import mip_coverage_ref
import mip_ref
from test_gpu_mip_roughness import SPECIALS
from util import SEED_A, SEED_B, assert_planes, bit_equal, synthetic_rgba, wrapped_image

pytestmark = pytest.mark.gpu

KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 102, 104
MIP_PER_LEVEL, MIP_NORMALS, MIP_ALPHA_WEIGHT = 2, 32, 128
BC3, BC7 = 3, 98
F = np.float32
SHAPES = [(64, 64), (130, 70), (256, 256), (320, 192), (1, 5), (5, 1), (3, 3), (2, 2), (1, 1), (1024, 512)]  # (w, h)
ALPHAS = ["binary", "fractional", "lone", "transparent", "ones", "specials"]
COUNTERS = ("mip_alpha_pull_pyramid", "mip_alpha_pull_level", "mip_alpha_push", "mip_pyramid", "mip_level")


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
def colours(w, h, seed=3):
    """R, G, B in [-0.25, 1.25): nothing in the rule clamps a colour."""
    return [np.random.default_rng([seed, c, w, h]).random((h, w), dtype=F) * F(1.5) - F(0.25) for c in range(3)]


def lone(w, h, x, y):
    a = np.zeros((h, w), F)
    a[max(y, 0), max(x, 0)] = 1.0
    return a


def planes_of(kind, w, h):
    """R, G, B and the alpha of the named kind."""
    rng = np.random.default_rng([17, w, h])
    p = colours(w, h)
    if kind == "binary":  # 30 % opaque
        a = np.where(rng.random((h, w)) < 0.3, F(1.0), F(0.0)).astype(F)
    elif kind == "fractional":  # half the texels 0, the rest anywhere in [0, 1.2): some weights clamp
        a = np.where(rng.random((h, w)) < 0.5, rng.random((h, w), dtype=F) * F(1.2), F(0.0)).astype(F)
    elif kind == "lone":  # one opaque texel near the far corner: every other texel walks up to its first known ancestor
        a = lone(w, h, w - 2, h - 2)
    elif kind == "corner":  # 130 x 70: column 64 and row 34 of level 1 are dropped, so nothing above level 1 knows it
        a = lone(w, h, w - 1, h - 1)
    elif kind == "transparent":
        a = np.zeros((h, w), F)
    elif kind == "ones":
        a = np.ones((h, w), F)
    elif kind == "specials":  # a tenth of the texels of all four planes
        a = rng.random((h, w), dtype=F)
        a[rng.random((h, w)) < 0.3] = 0.0
        for q in p + [a]:
            hit = rng.random((h, w)) < 0.1
            q[hit] = SPECIALS[rng.integers(0, len(SPECIALS), size=int(hit.sum()))]
    else:
        raise ValueError(kind)
    return p + [a]


_REF = {}


def cached(key, make):
    """Reference chains (per channel, a list of levels), computed once per key and shared, read-only."""
    if key not in _REF:
        got = make()
        for ch in got:
            for lv in ch:
                lv.setflags(write=False)
        _REF[key] = got
    return _REF[key]


def want_of(p, coverage=None):
    """The four reference chains of the planes p under the flag (alpha: the plain rule, or coverage's)."""
    alpha = mip_ref.chain(p[3]) if coverage is None else mip_coverage_ref.chain(p[3], coverage)[0]
    return ref.chain(*p) + [alpha]


def floor_log2(v):
    return v.bit_length() - 1


def walk(w, h, per_level):
    """(launches, pyramid launches, the levels whose P go through state planes) of the chain's level walk."""
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


def alpha_bytes(w, h, per_level, distinct, alpha_resident=True):
    """kc_stats_algorithmic_bytes of the pull and the push: `distinct` resident planes read, level 0's colour written, three
    colours and the weight of every level written, the state planes written and read beside the weight read, and the push's reads."""
    below = chain_texels(w, h, 1)
    return (4 * w * h * distinct + 12 * w * h + 16 * below + 28 * texels(w, h, walk(w, h, per_level)[2])
            + (4 * w * h if alpha_resident else 0) + 4 * below)


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


def gray(kc, plane):
    return kc.SlotImage.from_planes([plane]).materialize()


def check_levels(levels, refs, what):
    """levels: SlotImages; refs: per channel, the reference chain."""
    assert len(levels) == len(refs[0]), what
    for k, img in enumerate(levels):
        h, w = refs[0][k].shape
        assert tuple(img.size()) == (w, h), (what, k)
        assert_planes(img.planes(), [r[k] for r in refs], what="%s level %d" % (what, k))


def check_image(img, refs, what, coverage=None):
    fused = img.mips(alpha_weighted=True, coverage=coverage)
    check_levels(fused, refs, "%s fused" % (what,))
    check_levels(img.mips(per_level=True, alpha_weighted=True, coverage=coverage), refs, "%s per level" % (what,))
    return fused


# ------------------------------------------------------------------ the bits
@pytest.mark.parametrize("kind", ALPHAS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_level_equals_the_reference(kc, L, shape, kind):
    w, h = shape
    p = planes_of(kind, w, h)
    want = cached((kind, w, h), lambda: want_of(p))
    img = kc.SlotImage.from_planes(p).materialize()
    levels = check_image(img, want, (kind, w, h))
    assert len(levels) == kc.mip_level_count(w, h) and all(l.is_rgba() for l in levels)
    # level 0 is an image of its own: new colour planes beside the image's alpha, and the image keeps its planes as they were
    assert levels[0]._h.value != img._h.value
    mine, first = [plane_const(L, img, ch)[2] for ch in range(4)], [plane_const(L, levels[0], ch)[2] for ch in range(4)]
    assert first[3] == mine[3] and not set(first[:3]) & set(mine)
    assert_planes(img.planes(), p, what="the image afterwards")
    if kind == "ones":
        for c in range(3):
            assert all(bit_equal(a, b) for a, b in zip(want[c], mip_ref.chain(p[c])))  # the plain chain
    if kind == "transparent":
        assert not any(lv.any() for c in range(3) for lv in want[c])


@pytest.mark.parametrize("shape", [(256, 256), (1024, 512)], ids=lambda s: "%dx%d" % s)
def test_the_lone_texel_leaves_unknown_texels_above_the_second_launch(shape):
    """A condition on the input of the test above: at level 7, behind the state planes, texels are still unknown, so the push of
    a level-0 texel walks past the launch boundary: the far corner finds its first known ancestor at the last level."""
    w, h = shape
    p = planes_of("lone", w, h)
    _, known = ref.pull(*p)
    assert walk(w, h, False)[2][0] == 6
    assert known[7].any() and not known[7].all() and known[0].sum() == 1
    want = cached(("lone", w, h), lambda: want_of(p))
    assert not any(known[k][0, 0] for k in range(len(known) - 1)) and known[-1][0, 0]
    assert want[0][0][0, 0] == want[0][-1][0, 0] != 0.0 and want[0][0][h - 2, w - 2] == p[0][h - 2, w - 2]


def test_a_texel_in_a_dropped_column_and_row(kc):
    w, h = 130, 70
    p = planes_of("corner", w, h)
    want = cached(("corner", w, h), lambda: want_of(p))
    _, known = ref.pull(*p)
    assert known[1][34, 64] and not any(k.any() for k in known[2:])
    check_image(kc.SlotImage.from_planes(p), want, "corner")


@pytest.mark.parametrize("shape", [(130, 70), (256, 256)], ids=lambda s: "%dx%d" % s)
def test_combined_with_coverage(kc, shape):
    w, h = shape
    p = planes_of("fractional", w, h)
    want = cached(("fractional+coverage", w, h), lambda: want_of(p, 128))
    assert not all(bit_equal(a, b) for a, b in zip(want[3], mip_ref.chain(p[3])))  # coverage does rescale this alpha
    check_image(kc.SlotImage.from_planes(p), want, ("coverage", w, h), coverage=128)


# ------------------------------------------------------------------ planes
def mixed_image(kc, p, const):
    """An RGBA image of the planes p; channel ch is the constant plane const[ch] where that is not None."""
    w, h = p[0].shape[1], p[0].shape[0]
    parts = [kc.SlotImage.from_value(kc.Size(w, h), const[ch], False) if const[ch] is not None else gray(kc, p[ch]) for ch in range(4)]
    return kc.combine_rgba_process(parts)  # the planes themselves: a constant stays a constant


@pytest.mark.parametrize("alpha", [1.0, 1.5, 0.0, -2.0, float("nan"), 0.5])
def test_a_constant_alpha(kc, L, alpha):
    w, h = 130, 70
    p = colours(w, h) + [np.full((h, w), alpha, F)]
    img = mixed_image(kc, p, [None, None, None, alpha])
    assert plane_const(L, img, 3)[0] and not plane_const(L, img, 0)[0]
    weight = float(ref.weight(alpha))
    want = cached(("const alpha", repr(alpha)), lambda: want_of(p))
    for per_level in (False, True):
        launches, pyramids, _ = walk(w, h, per_level)
        c0, st0 = counters(kc), kc.stats()
        levels = img.mips(per_level=per_level, alpha_weighted=True)
        c1, st1 = counters(kc), kc.stats()
        delta = [b - a for a, b in zip(c0, c1)]
        check_levels(levels, want, "alpha %r per_level=%s" % (alpha, per_level))
        assert [plane_const(L, lv, 3)[:2] for lv in levels] == [(True, const_fold(alpha, k)) for k in range(len(levels))] or alpha != alpha
        if weight == 1.0:  # the plain chain of the image: levels[0] is the image, the colours go down the plain kernels
            assert levels[0]._h.value == img._h.value
            assert delta == [0, 0, 0, pyramids, launches - pyramids]
        elif weight == 0.0:  # constant-zero colour at every level, nothing launched
            assert delta == [0, 0, 0, 0, 0] and st1["kernel_launches"] == st0["kernel_launches"]
            assert all(plane_const(L, lv, ch)[:2] == (True, F(0.0)) for lv in levels for ch in range(3))
        else:  # through the kernels; the push has nothing to read at level 0
            assert delta == [pyramids, launches - pyramids, 1, 0, 0]
            assert st1["kernel_launches"] - st0["kernel_launches"] == launches + 1
            assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == alpha_bytes(w, h, per_level, 3, alpha_resident=False)


@pytest.mark.parametrize("alpha", [0.5, 1e-45, 1.0, 0.0])
def test_four_constants_are_folded_on_the_host(kc, L, alpha):
    w, h = 130, 70
    rgb = (0.8, 3e38, -0.25)
    img = kc.combine_rgba_process([kc.SlotImage.from_value(kc.Size(w, h), v, False) for v in rgb + (alpha,)])
    want = want_of([np.full((h, w), v, F) for v in rgb + (alpha,)])
    n0 = kc.stats()["kernel_launches"]
    levels = img.mips(alpha_weighted=True)
    assert kc.stats()["kernel_launches"] == n0
    assert all(plane_const(L, lv, ch)[0] for lv in levels for ch in range(4))
    check_levels(levels, want, "four constants, alpha %r" % alpha)


def test_a_constant_colour_channel_and_aliased_colour_channels(kc, L):
    w, h = 130, 70
    p = planes_of("binary", w, h)
    # G is a constant: a value in the first launch's arguments, and a plane of its own at every level, level 0 included
    q = [p[0], np.full((h, w), 0.3, F), p[2], p[3]]
    img = mixed_image(kc, q, [None, 0.3, None, None])
    assert plane_const(L, img, 1)[:2] == (True, F(0.3))
    want = want_of(q)
    for per_level in (False, True):
        st0 = kc.stats()
        levels = img.mips(per_level=per_level, alpha_weighted=True)
        st1 = kc.stats()
        check_levels(levels, want, "constant G per_level=%s" % per_level)
        assert not any(plane_const(L, lv, 1)[0] for lv in levels)
        assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == alpha_bytes(w, h, per_level, 3) + 4 * chain_texels(w, h)
    # R, G, B alias one plane (as_type's planes) beside a resident alpha: read once each, three planes written
    g = gray(kc, p[0])
    rgba = g.as_type(True)
    handles = [plane_const(L, rgba, ch)[2] for ch in range(3)]
    assert handles[0] == handles[1] == handles[2]
    parts = [g, g, g, gray(kc, p[3])]
    img = kc.combine_rgba_process(parts).materialize()
    handles = [plane_const(L, img, ch)[2] for ch in range(3)]
    assert handles[0] == handles[1] == handles[2]
    want = want_of([p[0], p[0], p[0], p[3]])
    for per_level in (False, True):
        st0 = kc.stats()
        levels = img.mips(per_level=per_level, alpha_weighted=True)
        st1 = kc.stats()
        check_levels(levels, want, "aliased per_level=%s" % per_level)
        assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == alpha_bytes(w, h, per_level, 2) + 4 * chain_texels(w, h)
        for lv in levels:
            assert len({plane_const(L, lv, ch)[2] for ch in range(3)}) == 3


def test_a_pending_mix_chain_is_forced(kc):
    """Mix writes an alpha of ones, so the colours are three pending Gray chains beside a resident alpha."""
    w, h = 130, 70
    a, b = synthetic_rgba(SEED_A, h, w), synthetic_rgba(SEED_B, h, w)
    alpha = np.where(b[3] < 0.5, F(0.0), b[3]).astype(F)
    parts = [kc.mix_process(kc.SlotImage.from_planes([a[c]]), kc.SlotImage.from_planes([b[c]]), kc.MixType.Multiply) for c in range(3)]
    mixed = kc.combine_rgba_process(parts + [gray(kc, alpha)])
    levels = mixed.mips(alpha_weighted=True)  # the pending chains run first
    p = mixed.planes()
    assert (p[3] == 0).any() and (p[3] > 0).any() and not bit_equal(p[0], a[0])
    want = want_of(p)
    check_levels(levels, want, "mix")
    check_levels(mixed.mips(per_level=True, alpha_weighted=True), want, "mix per level")
    # an RGBA Mix result itself: its alpha is a constant 1, and the chain is the plain one
    rgba = kc.mix_process(kc.SlotImage.from_planes(a), kc.SlotImage.from_planes(b), kc.MixType.Multiply)
    levels = rgba.mips(alpha_weighted=True)
    check_levels(levels, [mip_ref.chain(c) for c in rgba.planes()], "mix rgba")
    assert levels[0]._h.value == rgba._h.value


@pytest.mark.parametrize("h", [37, 64])
def test_wrapped_tensors_with_a_tight_pitch(kc, torch, h):
    w = 100  # 400 bytes per row, no padding: the second tile's columns 100 .. 127 do not exist
    p = planes_of("specials", w, h)
    wi = wrapped_image(kc, torch, p, "tight", guard=np.nan)
    assert all(t.shape[1] * 4 == 400 for t, _ in wi.parents)
    want = cached(("specials", w, h), lambda: want_of(p))
    check_image(wi.image, want, ("wrapped", w, h))
    wi.assert_untouched()  # the sources are only read


# ------------------------------------------------------------------ counts
@pytest.mark.parametrize("w,h,launches,pyramid", [(64, 64, 1, 1), (256, 256, 2, 2), (130, 70, 2, 1), (1024, 512, 3, 2)])
def test_launches_counters_and_algorithmic_bytes(kc, w, h, launches, pyramid):
    img = kc.SlotImage.from_planes(planes_of("binary", w, h)).materialize()
    for per_level in (False, True):
        assert walk(w, h, False)[:2] == (launches, pyramid)
        want = mip_ref.level_count(w, h) - 1 if per_level else launches
        pyr, lev = (0, want) if per_level else (pyramid, launches - pyramid)
        st0, c0 = kc.stats(), counters(kc)
        img.mips(per_level=per_level, alpha_weighted=True)
        st1, c1 = kc.stats(), counters(kc)
        # the pull takes the launches of the plain chain of one plane, the push one more; alpha keeps its plain launches
        assert [b - a for a, b in zip(c0, c1)] == [pyr, lev, 1, pyr, lev]
        assert st1["kernel_launches"] - st0["kernel_launches"] == 2 * want + 1
        assert st1["algorithmic_bytes"] - st0["algorithmic_bytes"] == alpha_bytes(w, h, per_level, 4) + 4 * chain_texels(w, h)
        # the plain chain of the same image: none of it on the new counters
        c0 = counters(kc)
        img.mips(per_level=per_level)
        assert [b - a for a, b in zip(c0, counters(kc))] == [0, 0, 0, pyr, lev]


def test_a_one_by_one_image_takes_a_copy_and_the_push(kc):
    img = kc.SlotImage.from_planes(planes_of("ones", 1, 1)).materialize()
    st0, c0 = kc.stats(), counters(kc)
    levels = img.mips(alpha_weighted=True)
    st1, c1 = kc.stats(), counters(kc)
    assert len(levels) == 1 and [b - a for a, b in zip(c0, c1)] == [0, 1, 1, 0, 0]
    assert st1["kernel_launches"] - st0["kernel_launches"] == 2


# ------------------------------------------------------------------ the exporters
@pytest.mark.parametrize("fmt", [BC3, BC7])
def test_the_exporters_encode_the_chain_mips_builds(kc, fmt, tmp_path):
    w, h = 130, 70
    p = planes_of("fractional", w, h)
    img = kc.SlotImage.from_planes([np.clip(c, 0.0, 1.0) for c in p]).materialize()
    srgb = fmt == BC7
    want = kc.levels_to_bc_mips(img.mips(alpha_weighted=True), fmt, srgb=srgb)
    got = img.to_bc_mips(fmt, srgb=srgb, alpha_weighted=True)
    assert len(got) == len(want) == kc.mip_level_count(w, h)
    for k, (g, r) in enumerate(zip(got, want)):
        assert g.shape == r.shape and np.array_equal(g, r), "level %d differs" % k
    plain = img.to_bc_mips(fmt, srgb=srgb)
    assert not np.array_equal(plain[0], got[0]) and not np.array_equal(plain[2], got[2])  # level 0 is filled too
    both = img.to_bc_mips(fmt, srgb=srgb, alpha_weighted=True, coverage=128, per_level=True)
    for k, r in enumerate(kc.levels_to_bc_mips(img.mips(alpha_weighted=True, coverage=128), fmt, srgb=srgb)):
        assert np.array_equal(both[k], r), "level %d differs with coverage" % k
    path = tmp_path / "cutout.dds"
    img.write_dds(path, fmt, srgb=srgb, alpha_weighted=True)
    assert path.read_bytes() == kc.dds_header(w, h, fmt, srgb=srgb) + b"".join(b.tobytes() for b in want)
    img.write_dds(path, fmt, srgb=srgb, mips=False, alpha_weighted=True)  # no effect without mips
    assert path.read_bytes() == kc.dds_header(w, h, fmt, srgb=srgb, levels=1) + img.to_bc(fmt, srgb=srgb).tobytes()
    dev, offs = img.to_bc_mips_torch(fmt, srgb=srgb, alpha_weighted=True)
    assert dev.cpu().numpy().tobytes() == b"".join(b.tobytes() for b in want)


# ------------------------------------------------------------------ refusals
def test_gray_images_and_normals_are_refused_with_nothing_launched_or_allocated(kc, L, tmp_path):
    w, h = 130, 70
    p = planes_of("binary", w, h)
    img = kc.SlotImage.from_planes(p).materialize()
    g = gray(kc, p[0])
    kc.sync()
    n = kc.mip_level_count(w, h)
    arr, count = (C.c_void_p * n)(), C.c_uint32(0)
    _, total = kc.bc_mip_layout(w, h, BC3)
    host = np.zeros(total, np.uint8)
    in_use, n0 = kc.stats()["bytes_in_use"], kc.stats()["kernel_launches"]
    assert L.kc_image_build_mips(g._h, MIP_ALPHA_WEIGHT, arr, n, C.byref(count)) == KC_ERR_INVALID_ARG and count.value == n
    assert L.kc_image_build_mips(g._h, MIP_ALPHA_WEIGHT | MIP_PER_LEVEL, arr, n, C.byref(count)) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_mips(g._h, BC3, MIP_ALPHA_WEIGHT, host.ctypes.data, total) == KC_ERR_INVALID_ARG
    assert L.kc_image_write_dds(g._h, str(tmp_path / "never.dds").encode(), BC3, MIP_ALPHA_WEIGHT, 1) == KC_ERR_INVALID_ARG
    count.value = 0
    for image in (img, g):
        assert L.kc_image_build_mips(image._h, MIP_ALPHA_WEIGHT | MIP_NORMALS, arr, n, C.byref(count)) == KC_ERR_UNSUPPORTED
        assert L.kc_image_to_bc_mips(image._h, BC3, MIP_ALPHA_WEIGHT | MIP_NORMALS, host.ctypes.data, total) == KC_ERR_UNSUPPORTED
    assert count.value == 0  # refused before the image is looked at
    assert L.kc_image_build_mips(img._h, MIP_ALPHA_WEIGHT, arr, n - 1, C.byref(count)) == KC_ERR_INVALID_ARG and count.value == n
    with pytest.raises(kc.TexProError):
        g.mips(alpha_weighted=True)
    with pytest.raises(kc.TexProError):
        img.mips(alpha_weighted=True, normals=True)
    assert kc.stats()["kernel_launches"] == n0 and kc.stats()["bytes_in_use"] == in_use
    assert not host.any() and not (tmp_path / "never.dds").exists()
    # the levels hold their planes until they are released; the scratch went back to the pool with the call
    assert L.kc_image_build_mips(img._h, MIP_ALPHA_WEIGHT, arr, n, C.byref(count)) == 0 and count.value == n
    assert kc.stats()["bytes_in_use"] > in_use
    for k in range(n):
        assert L.kc_image_release(arr[k]) == 0
    assert kc.stats()["bytes_in_use"] == in_use
