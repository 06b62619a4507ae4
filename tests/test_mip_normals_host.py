"""The host half of KC_MIP_NORMALS (include/kanter_core_amd.h), on a machine without a GPU: kc_mip_normal_texel -- the function the
constant fold calls -- equals tests/mip_normals_ref.py bit for bit, the reference itself has the properties the rule is there
for (a flat map stays flat, cancelling vectors take the fallback, every level of a chain decodes to unit vectors), and the flag
stays refused where the contract says so."""
import ctypes as C
import itertools

import numpy as np
import pytest

import mip_normals_ref
import mip_ref
from util import SEED_A, bit_equal, synthetic_rgba

KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 102, 104
MIP_NORMALS = 32
F = np.float32
FLT_MAX = np.finfo(F).max
SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, 3e38, -3e38, FLT_MAX, 0.5, 0.5 + 2.0 ** -24, 0.5 - 2.0 ** -24,
                     0.5 + 2.0 ** -20, 0.5 - 2.0 ** -20], F)
SHAPES = [(64, 64), (130, 70), (1024, 512)]  # (w, h)


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    return kc


def check_triples(kc, triples, what):
    t = np.ascontiguousarray(triples, F)
    want = np.stack(mip_normals_ref.normal_texel(t[:, 0], t[:, 1], t[:, 2]), axis=1)
    got = np.stack([kc.mip_normal_texel(b) for b in t])
    assert got.dtype == F and not np.isnan(got).any(), what
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert bad.size == 0, "%s: %d of %d differ, e.g. box %s got %s want %s" % (what, bad.size, len(t), t[bad[0]], got[bad[0]], want[bad[0]])


def test_texel_equals_the_reference_on_a_grid(kc):
    axis = np.concatenate([np.linspace(0.0, 1.0, 17, dtype=F), np.array([0.3, 0.7071068, 0.9999999, 1.25, -0.25], F)])
    check_triples(kc, list(itertools.product(axis, repeat=3)), "grid")
    rng = np.random.default_rng(SEED_A)
    check_triples(kc, rng.random((4096, 3), dtype=F), "random")
    # unit vectors as height_to_normal writes them, and their shortened boxes
    n = rng.standard_normal((4096, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    check_triples(kc, (n * 0.5 + 0.5).astype(F), "unit")
    check_triples(kc, (n * rng.random((4096, 1)) * 0.5 + 0.5).astype(F), "shortened")


def test_texel_equals_the_reference_on_special_values(kc):
    check_triples(kc, list(itertools.product(SPECIALS, repeat=3)), "specials")
    # each special in each position beside ordinary values
    rows = []
    for pos in range(3):
        for s in SPECIALS:
            for other in ((0.25, 0.75), (0.5, 0.5), (1.0, 0.0)):
                b = list(other)
                b.insert(pos, s)
                rows.append(b)
    check_triples(kc, rows, "specials beside ordinary values")


def test_a_vector_without_a_direction_is_the_fallback(kc):
    flat = np.array([0.5, 0.5, 1.0], F)
    for box in ([0.5, 0.5, 0.5], [np.nan, 0.5, 1.0], [0.5, np.inf, 1.0], [0.5, 0.5, -np.inf], [FLT_MAX, 0.5, 0.5], [3e38, 3e38, 3e38]):
        assert bit_equal(kc.mip_normal_texel(box), flat), box
    assert bit_equal(kc.mip_normal_texel(flat), flat)


def test_null_arguments_and_shapes_are_refused(kc):
    from kanter_core_amd import _lib
    L = _lib.load()
    a, out = np.array([0.5, 0.5, 1.0], F), np.full(3, 7.0, F)
    assert L.kc_mip_normal_texel(None, out.ctypes.data) == KC_ERR_INVALID_ARG
    assert L.kc_mip_normal_texel(a.ctypes.data, None) == KC_ERR_INVALID_ARG
    assert (out == 7.0).all()
    assert L.kc_mip_normal_texel(a.ctypes.data, out.ctypes.data) == 0 and bit_equal(out, a)
    with pytest.raises(ValueError):
        kc.mip_normal_texel([0.5, 0.5])


def test_the_header_keeps_refusing_the_flag(kc):
    from kanter_core_amd import _lib
    L = _lib.load()
    out = (C.c_uint8 * 148)()
    for fmt in (5, 3):
        assert L.kc_dds_header(64, 64, fmt, MIP_NORMALS, 7, out, None) == KC_ERR_UNSUPPORTED
        assert L.kc_dds_header(64, 64, fmt, 0, 7, out, None) == 0
    assert kc.MIP_NORMALS == MIP_NORMALS


# ------------------------------------------------------------------ the reference itself
def test_a_flat_map_stays_flat():
    w, h = 130, 70
    r, g, b = np.full((h, w), 0.5, F), np.full((h, w), 0.5, F), np.full((h, w), 1.0, F)
    levels = mip_normals_ref.chain(r, g, b)
    assert len(levels[0]) == mip_ref.level_count(w, h)
    for c, v in enumerate((0.5, 0.5, 1.0)):
        for k, lv in enumerate(levels[c]):
            assert lv.shape == mip_ref.level_size(w, h, k)[::-1]
            assert bit_equal(lv, np.full(lv.shape, v, F)), (c, k)


def test_cancelling_columns_give_the_fallback_at_level_one():
    w, h = 64, 32
    r = np.tile(np.array([1.0, 0.0], F), (h, w // 2))  # (1, .5, .5) and (0, .5, .5): +x and -x
    g, b = np.full((h, w), 0.5, F), np.full((h, w), 0.5, F)
    levels = mip_normals_ref.chain(r, g, b)
    for c, v in enumerate((0.5, 0.5, 1.0)):
        for k in range(1, len(levels[c])):
            assert bit_equal(levels[c][k], np.full(levels[c][k].shape, v, F)), (c, k)
    plain = mip_ref.reduce(r)
    assert bit_equal(plain, np.full(plain.shape, 0.5, F))  # the plain rule leaves the zero vector (0.5, 0.5, 0.5)


def unit_planes(w, h, seed):
    rng = np.random.default_rng([seed, w, h])
    n = rng.standard_normal((3, h, w))
    n[2] = np.abs(n[2]) + 0.05
    n /= np.sqrt((n * n).sum(axis=0))
    return [(c * 0.5 + 0.5).astype(F) for c in n]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("data", ["random", "unit"])
def test_every_level_decodes_to_unit_vectors(shape, data):
    """| |v| - 1 | <= 1e-6 in float64 for every texel of every level >= 1: the roundings of l, the three quotients and the
    encode step keep the deviation under 8 * 2^-24 = 4.8e-7."""
    w, h = shape
    planes = synthetic_rgba(SEED_A, h, w)[:3] if data == "random" else unit_planes(w, h, 11)
    levels = mip_normals_ref.chain(*planes)
    plain = [mip_ref.chain(p) for p in planes]
    worst, shortest = 0.0, 1.0
    for k in range(1, len(levels[0])):
        d = np.stack([levels[c][k] for c in range(3)]).astype(np.float64)
        assert not np.isnan(d).any(), k
        dev = np.abs(np.sqrt(((d * 2.0 - 1.0) ** 2).sum(axis=0)) - 1.0)
        worst = max(worst, float(dev.max()))
        p = np.stack([plain[c][k] for c in range(3)]).astype(np.float64)
        shortest = min(shortest, float(np.sqrt(((p * 2.0 - 1.0) ** 2).sum(axis=0)).min()))
    print("%s %dx%d: max | |v| - 1 | = %.3g; the plain rule's shortest vector %.3f" % (data, w, h, worst, shortest))
    assert worst <= 1e-6
    assert shortest < 0.9  # what the flag is there for
