"""Conditions on the inputs of the mip-state sweep (tests/mip_states.py, test_gpu_mip_states.py), established from the numpy
references alone, so that the device tests cannot pass emptily: the patterns are the 52 there are, the kind rotation gives every
channel every kind and every image two pitches, and at both shapes every rule really differs from the plain rule on the pixels the
device test uses (pending classes included).  No device; 2 s, nearly all of it the references of the last test but one."""
import math

import numpy as np
import pytest

import mip_alpha_ref
import mip_ref
import mip_states as ms
from test_gpu_mip_alpha import walk
from util import bit_equal

BELL = [1, 1, 2, 5, 15]  # set partitions of 0 .. 4 elements


def same(a, b):
    return len(a) == len(b) and all(bit_equal(x, y) for x, y in zip(a, b))


def test_the_patterns_are_the_52():
    pats = ms.patterns()
    # by the definition: choose the constant channels, partition the rest
    assert len(pats) == sum(math.comb(4, k) * BELL[4 - k] for k in range(5)) == 52
    assert len(set(pats)) == 52
    for p in pats:
        seen = 0
        for j in p:  # restricted growth: a new class is the next index
            assert j is None or 0 <= j <= seen
            seen = max(seen, -1 if j is None else j + 1)
    three = sum(math.comb(3, k) * BELL[3 - k] for k in range(4))  # the patterns of three channels
    assert three == 15
    assert sum(p[3] is None for p in pats) == three  # a constant alpha beside any R, G, B
    assert len({p[:3] for p in pats}) == len({p[:3] for p in pats if p[3] is None}) == three
    assert sum(any(j is not None for j in p[:3]) for p in pats if p[3] is None) == three - 1  # the normal maps of the roughness sweep
    # R, G, B all constant: alpha a constant, or the one class
    assert [p for p in pats if p[:3] == (None, None, None)] == [(None, None, None, None), (None, None, None, 0)]
    assert pats[0] == (None,) * 4 and pats[-1] == (0, 1, 2, 3)
    assert (0, None, 0, 1) in pats  # the two patterns of the roughness sweep's other powers


def test_the_kind_rotation_reaches_every_pair_and_two_pitches():
    assert sorted(ms.KINDS) == sorted(["pool", "tight", "pad48", "offset", "pending"])
    for rotate in (0, 2):  # the images, and the normal maps of the roughness sweep
        met = set()
        for i, p in enumerate(ms.patterns()):
            kinds = ms.kinds_of(i, p, rotate)
            assert len(kinds) == ms.class_count(p)
            met.update((ch, kinds[j]) for ch, j in enumerate(p) if j is not None)
            for w, _ in ms.SHAPES:
                assert ms.pool_pitch(w) * 4 == (4 * w + 255) // 256 * 256
                pitches = {ms.pitch_of(k, w) for k in kinds}
                assert len(kinds) < 2 or len(pitches) >= 2, (i, p, kinds, w)
                assert all(f % 4 == 0 and f >= w for f in pitches)
        assert met == {(ch, k) for ch in range(4) for k in ms.KINDS}
    for w, _ in ms.SHAPES:  # the four layouts have four pitches
        assert len({ms.pitch_of(k, w) for k in ("pool", "tight", "pad48", "offset")}) == 4


@pytest.mark.parametrize("shape,want", [((130, 70), {False: (2, 1, [6]), True: (7, 0, [1, 2, 3, 4, 5, 6])}),
                                        ((37, 150), {False: (3, 1, [5, 6]), True: (7, 0, [1, 2, 3, 4, 5, 6])})],
                         ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else "walk")
def test_the_level_walks(shape, want):
    w, h = shape
    assert shape in ms.SHAPES and mip_ref.level_count(w, h) == 8
    for per_level in (False, True):
        assert walk(w, h, per_level) == want[per_level]
    if shape == (130, 70):  # six fused levels over 3 x 2 tiles of 64 x 64, partial both ways
        assert w % 4 == 2 and ((w + 63) // 64, (h + 63) // 64) == (3, 2) and w % 64 and h % 64
        assert mip_ref.level_size(w, h, 6) == (2, 1)
    else:  # five fused levels, then the 1-wide levels one by one
        assert w % 4 == 1 and [mip_ref.level_size(w, h, k) for k in (5, 6, 7)] == [(1, 4), (1, 2), (1, 1)]


@pytest.mark.parametrize("shape", ms.SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_rule_differs_from_the_plain_rule_on_every_pattern(shape):
    w, h = shape
    for st in ms.states(w, h):
        p, what = st.planes, repr(st)
        assert not any(np.isnan(q).any() or np.isinf(q).any() for q in p), what
        plain = ms.reference(p, {}, st.keys)
        refs = {ms.flag_id(f): ms.reference(p, f, st.keys) for f in ms.FLAG_SETS}
        rough = [ms.reference(p, dict(roughness=(ch, p[:3], 1.0), roughness_keys=st.keys[:3]), st.keys) for ch in range(4)]
        for name, chains in list(refs.items()) + [("roughness %d" % ch, r) for ch, r in enumerate(rough)]:
            assert len(chains) == 4 and all(len(c) == 8 for c in chains), (what, name)
            assert not any(np.isnan(lv).any() for c in chains for lv in c), (what, name)
        rgb_resident = any(st.resident(ch) for ch in range(3))
        if rgb_resident:
            assert not all(same(refs["normals=True"][c], plain[c]) for c in range(3)), what
        assert same(refs["normals=True"][3], plain[3]), what
        if st.resident(3):
            cov = refs["coverage=128"][3]
            assert bit_equal(cov[0], plain[3][0]) and not same(cov, plain[3]), what
            _, known = mip_alpha_ref.pull(*p)
            assert not known[0].all() and known[0].any() and not known[2].all(), what
            aw = refs["alpha_weighted=True"]
            assert not all(same(aw[c], plain[c]) for c in range(3)), what
            assert any(not bit_equal(aw[c][0], p[c]) for c in range(3)), what  # level 0 is filled too
        for ch in range(4):
            assert all(same(rough[ch][c], plain[c]) for c in range(4) if c != ch), what
            if st.resident(ch) and rgb_resident:
                assert not same(rough[ch][ch], plain[ch]), (what, ch)
            if not rgb_resident:  # flat normals: the plain chain
                assert same(rough[ch][ch], plain[ch]), (what, ch)


def test_a_constant_alpha_of_weight_one_and_zero():
    """The two extra values of a constant alpha: 1 gives the plain chain, 0 constant-zero colour."""
    w, h = ms.SHAPES[0]
    extra = [st for st in ms.states(w, h, dict(alpha_weighted=True)) if st.pattern[3] is None and float(st.values[3]) in ms.EXTRA_ALPHAS]
    assert len(extra) == 2 * 15 and len(ms.states(w, h, dict(normals=True))) == 52
    for st in extra:
        aw = ms.reference(st.planes, dict(alpha_weighted=True), st.keys)
        if st.values[3] == 1.0:
            assert all(same(aw[c], ms.reference(st.planes, {}, st.keys)[c]) for c in range(3)), st
        else:
            assert not any(lv.any() for c in range(3) for lv in aw[c]), st
