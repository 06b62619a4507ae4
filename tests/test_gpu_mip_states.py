"""The product of the channel states, through every mip family: each of the 52 patterns of constant and aliased channels
(tests/mip_states.py) -- the classes of one image in different memory layouts: a pool plane, caller-owned planes of three pitches
in NaN-guarded tensors, a pending Mix chain -- goes through mips() under the six flag sets and through roughness_mips(), fused and
per level, at the two smallest shapes that reach every level walk, and every level equals the numpy references bit for bit.  With
it: the source is only read; constants stay folded constants, aliased channels keep sharing a plane and channels under a rule of
their own get planes of their own; launches, counters and (where a family's module has the formula) algorithmic bytes of a second
call; the pool balances; the exporters encode the chain mips() builds.  The families' own modules test one or two hand-made
patterns each, all in one layout; the conditions on this module's inputs are test_mip_states_host.py's.

The sweep has found no defect so far; a pattern that does is pinned in a test_patterns_that_found_defects case here, with its
cause, as test_gpu_fuzz_graphs pins seeds.

Run time on an MI355X: 17 s for the module (66 tests, about 3 800 mips() and 2 200 roughness_mips() calls), of which 12 s are
the first test's set-up (library start-up); no test takes longer than 0.2 s."""
import ctypes as C

import numpy as np
import pytest

import bc1a_ref
import bc_ref
import mip_alpha_ref
import mip_states as ms
from test_gpu_mip_alpha import alpha_bytes, chain_texels, check_levels, const_fold, plane_const, walk
from test_gpu_mip_roughness import roughness_bytes
from util import bit_equal, wrapped_image

pytestmark = pytest.mark.gpu

F = np.float32
BC1, BC3, BC5, BC7 = 1, 3, 5, 98
COVERAGE_LAUNCHES = 7  # three counts, three picks, one scale
COUNTERS = ("mip_pyramid", "mip_level", "mip_normals_pyramid", "mip_normals_level", "mip_alpha_pull_pyramid", "mip_alpha_pull_level",
            "mip_alpha_push", "mip_coverage", "mip_roughness_pyramid", "mip_roughness_level")
SHAPE_IDS = ["%dx%d" % s for s in ms.SHAPES]
FLAG_IDS = [ms.flag_id(f) for f in ms.FLAG_SETS]
OWN_PLANES, ALIAS_R_CONST_G = ms.pattern_index((0, 1, 2, 3)), ms.pattern_index((0, None, 0, 1))


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


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


# ------------------------------------------------------------------ helpers
def release(L, levels):
    """gives the levels back now, whatever still names them"""
    for lv in levels:
        assert L.kc_image_release(lv._h) == 0
        lv._h = C.c_void_p(None)


def channels(L, img):
    """[(is_const, value, handle)] of the image's channels"""
    return [plane_const(L, img, ch) for ch in range(4 if img.is_rgba() else 1)]


def distinct(infos):
    """the distinct resident planes among (is_const, value, handle) entries"""
    return len({hnd for is_c, _, hnd in infos if not is_c})


def counted(kc, call):
    c0, s0 = [kc.stats_counter(n) for n in COUNTERS], kc.stats()
    got = call()
    c1, s1 = [kc.stats_counter(n) for n in COUNTERS], kc.stats()
    delta = {n: b - a for n, a, b in zip(COUNTERS, c0, c1)}
    return got, delta, s1["kernel_launches"] - s0["kernel_launches"], s1["algorithmic_bytes"] - s0["algorithmic_bytes"]


def check_source(L, built, what):
    """The image as it stands after the first call is the state: constants where the pattern has them, one plane per class
    unless forcing a pending class made more, and every resident class at the pitch the host conditions assume."""
    st = built.state
    info = channels(L, built.image)
    for ch, (is_c, v, hnd) in enumerate(info):
        assert is_c == (not st.resident(ch)), (what, ch)
        if is_c:
            assert bit_equal(np.array([v]), np.array([st.values[ch]])), (what, ch)
            continue
        p, ptr, pitch = C.c_void_p(), C.c_void_p(), C.c_size_t()
        assert L.kc_image_plane(built.image._h, ch, C.byref(p)) == 0
        assert L.kc_plane_device_ptr(p, C.byref(ptr), C.byref(pitch)) == 0
        L.kc_plane_release(p)
        kind = st.kinds[st.pattern[ch]]
        assert pitch.value == 4 * ms.pitch_of(kind, st.w), (what, ch, kind, pitch.value)
        if kind != "pending":
            assert all(hnd == info[e][2] for e in range(4) if st.pattern[e] == st.pattern[ch]), (what, ch)
    return info


def through_alpha_kernels(flags, info):
    """(the call builds level 0 anew, the pull and push run) for KC_MIP_ALPHA_WEIGHT on an image of this level-0 state"""
    if not flags.get("alpha_weighted"):
        return False, False
    a_const, a = info[3][0], info[3][1]
    weight = float(mip_alpha_ref.weight(a)) if a_const else None
    own_level0 = not (a_const and weight == 1.0)
    fold = all(i[0] for i in info)
    return own_level0, own_level0 and not (a_const and weight == 0.0) and not fold


def expected_mips_cost(flags, info, w, h, per_level):
    """-> (counter deltas, launches, algorithmic bytes or None) of mips(**flags) on a forced image of this level-0 state, as
    image_build_mips and image_build_alpha_mips enqueue them."""
    n, pyr, _ = walk(w, h, per_level)
    lev = n - pyr
    want = dict.fromkeys(COUNTERS, 0)
    resident = [not i[0] for i in info]
    own_level0, kernels = through_alpha_kernels(flags, info)
    nbytes = None
    if n == 0:  # a 1 x 1 image has no level to make: the alpha rule's level 0 alone, by one one-level launch and the push
        if kernels:
            want.update(mip_alpha_pull_level=1, mip_alpha_push=1)
        return want, sum(want.values()), None
    if own_level0:
        plain = resident[3]
        if kernels:
            want.update(mip_alpha_pull_pyramid=pyr, mip_alpha_pull_level=lev, mip_alpha_push=1)
        if not flags.get("coverage"):
            nbytes = (alpha_bytes(w, h, per_level, distinct(info), alpha_resident=resident[3]) if kernels else 0) + (4 * chain_texels(w, h) if plain else 0)
    else:
        normals = bool(flags.get("normals"))
        plain = any(resident[3 if normals else 0:])
        if normals and any(resident[:3]):
            want.update(mip_normals_pyramid=pyr, mip_normals_level=lev)
    if plain:
        want.update(mip_pyramid=pyr, mip_level=lev)
    if flags.get("coverage") and resident[3]:
        want["mip_coverage"] = COVERAGE_LAUNCHES
    return want, sum(want.values()), nbytes


def check_structure(kc, L, img, info, levels, flags, what):
    """The planes of the levels: folded constants stay constants, aliases of the plain rule keep sharing, a rule of its own gives
    planes of its own; `info`: the image's channels after the first call."""
    own_level0, kernels = through_alpha_kernels(flags, info)
    resident = [not i[0] for i in info]
    own = set()  # the channels under a rule of their own that gives them resident planes
    if flags.get("normals") and any(resident[:3]) or kernels:
        own |= {0, 1, 2}
    if flags.get("coverage") and resident[3]:
        own.add(3)
    first = channels(L, levels[0])
    if own_level0:  # an image of its own: new colour planes beside the image's alpha
        assert levels[0]._h.value != img._h.value, what
        assert first[3][2] == info[3][2] and not {i[2] for i in first[:3]} & {i[2] for i in info}, what
        if kernels:
            assert distinct(first[:3]) == 3, what
        else:  # weight 0, or four constants: folded on the host
            assert all(i[0] for i in first[:3]), what
    else:
        assert levels[0]._h.value == img._h.value, what
    flat = [i[1] for i in info[:3]]  # KC_MIP_NORMALS on three constants
    for k, lv in enumerate(levels[1:], 1):
        got = channels(L, lv)
        if flags.get("normals") and not any(resident[:3]):
            flat = list(kc.mip_normal_texel([const_fold(v) for v in flat]))
        for ch in range(4):
            is_c, v, hnd = got[ch]
            if ch in own:
                assert not is_c and all(hnd != got[e][2] for e in range(4) if e != ch), (what, k, ch)
            elif ch < 3 and own_level0:  # constant colour of the alpha rule, held to the reference by value
                assert is_c, (what, k, ch)
            elif ch < 3 and flags.get("normals"):
                assert is_c and bit_equal(np.array([v]), np.array([flat[ch]])), (what, k, ch, v, flat[ch])
            elif not resident[ch]:  # the plain rule: a folded constant
                assert is_c and bit_equal(np.array([v]), np.array([const_fold(info[ch][1], k)])), (what, k, ch, v)
            else:  # the plain rule: one plane per plane of level 0
                assert not is_c, (what, k, ch)
                for e in range(4):
                    if e != ch and e not in own and resident[e]:
                        assert (hnd == got[e][2]) == (info[ch][2] == info[e][2]), (what, k, ch, e)


# ------------------------------------------------------------------ mips(): every pattern under every flag set
@pytest.mark.parametrize("per_level", [False, True], ids=["fused", "per_level"])
@pytest.mark.parametrize("flags", ms.FLAG_SETS, ids=FLAG_IDS)
@pytest.mark.parametrize("shape", ms.SHAPES, ids=SHAPE_IDS)
def test_every_pattern_under_the_flag_set(kc, torch, L, shape, flags, per_level):
    w, h = shape
    for st in ms.states(w, h, flags):
        what = "%r %s per_level=%s" % (st, ms.flag_id(flags), per_level)
        want = ms.reference(st.planes, flags, st.keys)
        built = ms.build(kc, torch, st)
        img = built.image
        in_use = kc.stats()["bytes_in_use"]
        levels = img.mips(per_level=per_level, **flags)  # forces a pending class
        assert len(levels) == kc.mip_level_count(w, h) and all(lv.is_rgba() for lv in levels), what
        check_levels(levels, want, what)
        info = check_source(L, built, what)
        check_structure(kc, L, img, info, levels, flags, what)
        release(L, levels)
        forced = kc.stats()["bytes_in_use"]
        assert forced == in_use or "pending" in st.kinds, what
        # the second call: nothing is left to force
        levels, delta, launches, nbytes = counted(kc, lambda: img.mips(per_level=per_level, **flags))
        cost = expected_mips_cost(flags, info, w, h, per_level)
        assert (delta, launches) == cost[:2], what
        assert cost[2] is None or nbytes == cost[2], (what, nbytes, cost[2])
        check_levels(levels, want, what + ", second call")
        release(L, levels)
        built.assert_untouched(what)
        assert kc.stats()["bytes_in_use"] == forced, what


# ------------------------------------------------------------------ roughness_mips()
def expected_roughness_cost(img_info, channel, normal_info, w, h, per_level):
    n, pyr, _ = walk(w, h, per_level)
    want = dict.fromkeys(COUNTERS, 0)
    others = [i for ch, i in enumerate(img_info) if ch != channel]
    if all(i[0] for i in normal_info[:3]):  # flat normals: the plain chain of the image
        if distinct(img_info):
            want.update(mip_pyramid=pyr, mip_level=n - pyr)
        return want, sum(want.values()), None
    want.update(mip_roughness_pyramid=pyr, mip_roughness_level=n - pyr)
    if distinct(others):
        want.update(mip_pyramid=pyr, mip_level=n - pyr)
    nbytes = roughness_bytes(w, h, per_level, distinct(list(normal_info[:3]) + [img_info[channel]])) + 4 * chain_texels(w, h) * distinct(others)
    return want, sum(want.values()), nbytes


def run_roughness(kc, L, img, normals, channel, power, per_level, want, what, pending):
    """One image beside one normal map: the bits, the named channel's planes, the cost of a second call, the pool."""
    w, h = img.size()
    in_use = kc.stats()["bytes_in_use"]
    levels = img.roughness_mips(normals, channel, power, per_level=per_level)
    check_levels(levels, want, what)
    assert levels[0]._h.value == img._h.value, what
    img_info, normal_info = channels(L, img), channels(L, normals)
    flat = all(i[0] for i in normal_info[:3])
    for k, lv in enumerate(levels[1:], 1):
        got = channels(L, lv)
        if not flat:  # a plane of its own, whatever the channel is at level 0
            assert not got[channel][0] and all(got[channel][2] != g[2] for ch, g in enumerate(got) if ch != channel), (what, k)
        elif img_info[channel][0]:
            assert got[channel][0] and bit_equal(np.array([got[channel][1]]), np.array([const_fold(img_info[channel][1], k)])), (what, k)
    release(L, levels)
    forced = kc.stats()["bytes_in_use"]
    assert forced == in_use or pending, what
    levels, delta, launches, nbytes = counted(kc, lambda: img.roughness_mips(normals, channel, power, per_level=per_level))
    cost = expected_roughness_cost(img_info, channel, normal_info, w, h, per_level)
    assert (delta, launches) == cost[:2], what
    assert cost[2] is None or nbytes == cost[2], (what, nbytes, cost[2])
    check_levels(levels, want, what + ", second call")
    release(L, levels)
    assert kc.stats()["bytes_in_use"] == forced, what


def own_normal_map(kc, torch, L, st, channel, power, per_level):
    what = "%r as its own normal map, channel %d power %r per_level=%s" % (st, channel, power, per_level)
    want = ms.reference(st.planes, dict(roughness=(channel, st.planes[:3], power), roughness_keys=st.keys[:3]), st.keys)
    built = ms.build(kc, torch, st)
    run_roughness(kc, L, built.image, built.image, channel, power, per_level, want, what, "pending" in st.kinds)
    info = check_source(L, built, what)
    built.assert_untouched(what)
    return info


@pytest.mark.parametrize("channel", range(4))
@pytest.mark.parametrize("per_level", [False, True], ids=["fused", "per_level"])
@pytest.mark.parametrize("shape", ms.SHAPES, ids=SHAPE_IDS)
def test_roughness_of_every_pattern_as_its_own_normal_map(kc, torch, L, shape, per_level, channel):
    """Among them: R, G and B all constant (the plain chain, nothing new launched), the named channel a constant, and the named
    channel an alias of X, Y or Z."""
    for st in ms.states(*shape):
        own_normal_map(kc, torch, L, st, channel, 1.0, per_level)


@pytest.mark.parametrize("power", [2.0 ** -10, 65536.0])
@pytest.mark.parametrize("shape", ms.SHAPES, ids=SHAPE_IDS)
def test_roughness_at_the_ends_of_the_power_range(kc, torch, L, shape, power):
    for index in (OWN_PLANES, ALIAS_R_CONST_G):
        for per_level in (False, True):
            for channel in range(4):
                own_normal_map(kc, torch, L, ms.State(index, *shape), channel, power, per_level)


IMAGES = ["gray pool", "gray offset", "gray constant", "rgba aliased"]


@pytest.mark.parametrize("kind", IMAGES)
@pytest.mark.parametrize("per_level", [False, True], ids=["fused", "per_level"])
@pytest.mark.parametrize("shape", ms.SHAPES, ids=SHAPE_IDS)
def test_roughness_beside_a_separate_normal_map(kc, torch, L, shape, per_level, kind):
    """The normal map: every R, G, B pattern with a resident, a constant alpha, the kinds rotated by two against the images'."""
    w, h = shape
    maps = [i for i, p in enumerate(ms.patterns()) if p[3] is None and any(j is not None for j in p[:3])]
    assert len(maps) == 14
    rho, rho_key = ms.base_plane(w, h, 3), ("class", 3, False)
    for i in maps:
        nst = ms.State(i, w, h, rotate=2)
        nmap = ms.build(kc, torch, nst)
        channel, pending, check = 0, "pending" in nst.kinds, None
        if kind == "gray pool":
            img, planes, keys = kc.SlotImage.from_planes([rho]).materialize(), [rho], [rho_key]
        elif kind == "gray offset":
            wi = wrapped_image(kc, torch, [rho], "offset", guard=np.nan)
            img, planes, keys, check = wi.image, [rho], [rho_key], wi.assert_untouched
        elif kind == "gray constant":
            v = ms.CONSTANTS[3]
            img, planes, keys = kc.SlotImage.from_value(kc.Size(w, h), v, False), [ms.const_plane(w, h, v)], [("const", repr(F(v)))]
        else:  # channel 1 aliases channel 0
            ist = ms.State(ms.pattern_index((0, 0, 1, 2)), w, h)
            ibuilt = ms.build(kc, torch, ist)
            img, planes, keys, channel, check = ibuilt.image, ist.planes, ist.keys, 1, lambda: ibuilt.assert_untouched(kind)
            pending = pending or "pending" in ist.kinds
        what = "%s beside %r per_level=%s" % (kind, nst, per_level)
        want = ms.reference(planes, dict(roughness=(channel, nst.planes[:3], 1.0), roughness_keys=nst.keys[:3]), keys)
        run_roughness(kc, L, img, nmap.image, channel, 1.0, per_level, want, what, pending)
        check_source(L, nmap, what)
        nmap.assert_untouched(what)
        if check:
            check()
        if kind == "rgba aliased":
            got = channels(L, img)
            assert got[0][2] == got[1][2], what  # the image keeps its alias


# ------------------------------------------------------------------ the exporters
EXPORT = {"plain": (BC7, None), "normals=True": (BC5, None), "coverage=128+normals=True": (BC3, None), "coverage=128": (BC1, True),
          "alpha_weighted=True": (BC3, None), "alpha_weighted=True+coverage=128": (BC1, True)}


@pytest.mark.parametrize("flags", ms.FLAG_SETS, ids=FLAG_IDS)
def test_the_exporters_encode_the_chain_mips_builds(kc, torch, orc, flags, tmp_path):
    w, h = ms.SHAPES[0]
    fmt, punch = EXPORT[ms.flag_id(flags)]
    ref = flags.get("coverage") if punch else None
    for st in ms.states(w, h):
        what = "%r %s BC%d" % (st, ms.flag_id(flags), fmt)
        built = ms.build(kc, torch, st)
        img = built.image
        got = img.to_bc_mips(fmt, punch_through=punch, **flags)  # forces a pending class
        want = kc.levels_to_bc_mips(img.mips(**flags), fmt, punch_through=ref)
        assert len(got) == len(want) == kc.mip_level_count(w, h), what
        for k, (g, r) in enumerate(zip(got, want)):
            assert g.shape == r.shape and np.array_equal(g, r), "%s: level %d differs" % (what, k)
        if st.index % 7 == 0:
            path = tmp_path / ("pattern%d.dds" % st.index)
            img.write_dds(path, fmt, punch_through=punch, **flags)
            assert path.read_bytes() == kc.dds_header(w, h, fmt) + b"".join(b.tobytes() for b in want), what
            if fmt != BC7:  # one link to numpy: the encoders' references on the reference levels
                chains = ms.reference(st.planes, flags, st.keys)
                for k, g in enumerate(got):
                    px = orc.to_u8(orc.Image([c[k] for c in chains]), False)
                    blocks = bc1a_ref.encode(px, ref) if punch else bc_ref.encode(px, fmt)
                    assert g.shape == blocks.shape and np.array_equal(g, blocks), "%s: level %d differs from the reference's blocks" % (what, k)
        built.assert_untouched(what)
