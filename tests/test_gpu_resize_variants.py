"""GPU parity of the resize forms and of the variants their launchers pick from the launch size, at the sizes that pick
them: every case is ONE launch, the named counters (kc_stats_counter) show which form and which variant ran, and every
plane equals the CPU oracle's resample (orc.resize_plane) bit for bit.

Options are the defaults, except cache_budget_mb where a case names it (the budget decides resize_down2_kernel's job
order and the nontemporal stores).  The sources hold values in [-0.25, 1.25) and IEEE edge cases (NaN, +-inf, -0.0,
subnormals, 3e38 pairs whose vertical sums overflow) on the edges of bands, strips, tiles and on the last partial quad.
Reference: image::imageops::resize (crate image 0.24.0) as called from src/shared.rs:159-199."""
import numpy as np
import pytest

from util import SEED_A, SEED_B, assert_planes, edge_lines, resize_source, salt

pytestmark = pytest.mark.gpu

# every counter the resize forms keep; a case asserts the delta of each (0 unless the case names it)
COUNTERS = ["upsample_launches", "upsample_chain_launches", "resize_chain_launches", "poly2_launches", "down2_launches",
            "resize_poly_launches", "resize_down_launches", "resize_lds_launches", "resize_wide_launches",
            "resize_two_pass_launches", "poly_rows_4", "poly_rows_8", "poly_rows_12", "poly_rows_32", "poly2_rows_4",
            "poly2_rows_8", "poly2_rows_12", "poly2_rows_24", "poly2_xcd_order", "down2_xcd_order", "down2_by_rows",
            "upsample_nt_stores", "upsample_half_quads"]

CASES = [
    # (id, filter, planes, source (w, h), destination (w, h), cache_budget_mb or None, counters that read 1)
    ("poly_rows_32", "Lanczos3", 4, (4096, 4096), (1024, 1024), None, ["resize_poly_launches", "poly_rows_32"]),
    ("poly_rows_12", "Lanczos3", 1, (4096, 4096), (1024, 1024), None, ["resize_poly_launches", "poly_rows_12"]),
    # resize_poly2_kernel deals its bands to the XCDs whatever the budget (resize.cpp, plan_poly2): the order is the same
    # at budget 0 and 208, and the plain order comes from a launch of fewer than 16 band workgroups
    ("poly2_rows_24", "Gaussian", 4, (4096, 4096), (512, 512), None, ["poly2_launches", "poly2_rows_24", "poly2_xcd_order"]),
    ("poly2_budget_0", "Gaussian", 1, (2048, 2048), (256, 256), 0, ["poly2_launches", "poly2_rows_8", "poly2_xcd_order"]),
    ("poly2_budget_208", "Gaussian", 1, (2048, 2048), (256, 256), 208, ["poly2_launches", "poly2_rows_8", "poly2_xcd_order"]),
    ("poly2_plain_order", "Gaussian", 1, (512, 256), (64, 32), None, ["poly2_launches", "poly2_rows_4"]),
    # resize_down2_kernel: past the budget the plain grid, or row by row where the windows span several chunks
    ("down2_by_rows", "Lanczos3", 4, (4096, 4096), (2048, 2048), None, ["down2_launches", "down2_by_rows"]),
    ("down2_plain", "Lanczos3", 4, (4096, 4096), (3000, 3000), None, ["down2_launches"]),
    ("down2_xcd_budget_208", "Lanczos3", 1, (4096, 4096), (3000, 3000), 208, ["down2_launches", "down2_xcd_order"]),
    ("down2_plain_budget_0", "Lanczos3", 1, (4096, 4096), (3000, 3000), 0, ["down2_launches"]),
    # no down2 tables: windows over 4 chunks and over 32 taps
    ("down", "Lanczos3", 4, (4096, 4096), (600, 600), None, ["resize_down_launches"]),
    ("upsample_half_quads_nt", "CatmullRom", 4, (2048, 2048), (4096, 4096), None,
     ["upsample_launches", "upsample_half_quads", "upsample_nt_stores"]),
    ("upsample_ratio4_nt", "Lanczos3", 4, (1024, 1024), (4096, 4096), None, ["upsample_launches", "upsample_nt_stores"]),
    ("upsample_ratio4_budget_600", "Lanczos3", 4, (1024, 1024), (4096, 4096), 600, ["upsample_launches"]),
    ("lds", "Lanczos3", 4, (3000, 3000), (4096, 4096), None, ["resize_lds_launches"]),
    ("lds_gaussian", "Gaussian", 1, (700, 700), (3000, 3000), None, ["resize_lds_launches"]),
    ("wide", "Gaussian", 4, (3000, 700), (700, 3000), None, ["resize_wide_launches"]),
]


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    budget = kc.get_option("cache_budget_mb")
    yield kc
    kc.set_option("cache_budget_mb", budget)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


@pytest.fixture
def budget(kc):
    saved = kc.get_option("cache_budget_mb")
    yield lambda mb: kc.set_option("cache_budget_mb", saved if mb is None else mb)
    kc.set_option("cache_budget_mb", saved)


def sources(planes, sw, sh, dw, dh, seed=SEED_A):
    """`planes` source planes with edge cases on the source rows and columns of output band / tile / strip edges."""
    ry, rx = sh / dh, sw / dw
    rows = edge_lines(sh, [16, 64]) + [int(y * ry) for y in edge_lines(dh, [4, 8, 12, 16, 24, 32, 64])]
    cols = edge_lines(sw, [4, 64, 256, 1024]) + [int(x * rx) for x in edge_lines(dw, [16, 64, 128, 1024])]
    cols += [sw - 1 - k for k in range(sw % 4 or 4)]  # the last partial (or whole) quad
    return [salt(resize_source(seed, c, sh, sw), rows[c::2], cols[c % 2::2], shift=c) for c in range(planes)]


def snapshot(kc):
    return {n: kc.stats_counter(n) for n in COUNTERS}, kc.stats()["kernel_launches"]


def deltas(kc, before):
    now = snapshot(kc)
    return {n: now[0][n] - before[0][n] for n in COUNTERS if now[0][n] != before[0][n]}, now[1] - before[1]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_resize_variant_equals_oracle(kc, orc, budget, case):
    name, filt, planes, (sw, sh), (dw, dh), mb, expect = case
    src = sources(planes, sw, sh, dw, dh)
    img = kc.SlotImage.from_planes(src)
    budget(mb)
    before = snapshot(kc)
    out = kc.resize_image(img, (dw, dh), kc.ResizeFilter.parse(filt))
    out.materialize()
    seen, launches = deltas(kc, before)
    budget(None)
    assert launches == 1 and seen == {n: 1 for n in expect}, "%s: %d launches, counters %s, expected %s" % (name, launches, seen, expect)
    got = out.planes()
    for c in range(planes):
        assert_planes([got[c]], [orc.resize_plane(src[c], dw, dh, filt)], what="%s %s %s->%s plane %d" % (name, filt, (sw, sh), (dw, dh), c))


def test_resize_chain_many_tiles(kc, orc):
    """A 1000^2 RGBA operand resampled to 4096^2 (Triangle: not an integer ratio, at most 4 horizontal taps) inside the
    launch of the 3-node Add / Multiply / Subtract chain that consumes it: resize_chain_kernel over some 4000 tiles."""
    (sw, sh), (dw, dh) = (1000, 1000), (4096, 4096)
    small = sources(4, sw, sh, dw, dh, SEED_B)
    big = sources(4, dw, dh, dw, dh)
    ia = kc.SlotImage.from_planes(big)
    up = kc.resize_image(kc.SlotImage.from_planes(small), (dw, dh), kc.ResizeFilter.Triangle)
    before = snapshot(kc)
    blend = kc.mix_process(kc.mix_process(kc.mix_process(ia, up, kc.MixType.Add), ia, kc.MixType.Multiply), up, kc.MixType.Subtract)
    got = blend.planes()
    seen, launches = deltas(kc, before)
    assert seen == {"resize_chain_launches": 1}, "counters %s" % seen
    assert launches <= 1, launches
    assert len(got) == 4
    for c in range(3):
        bu = orc.resize_plane(small[c], dw, dh, "Triangle")
        want = orc.mix_plane("Subtract", orc.mix_plane("Multiply", orc.mix_plane("Add", big[c], bu), big[c]), bu)
        assert_planes([got[c]], [want], what="resize_chain channel %d" % c)
    assert_planes([got[3]], [np.ones((dh, dw), np.float32)], what="resize_chain alpha")
