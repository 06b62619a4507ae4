"""Host side of the resample pair sweep (tests/resize_pairs.py), no GPU: for every axis pair of the sets A, B and C and every
filter, what build_taps_host (csrc/resize.cpp) derives from the tap table and the kernels then trust, against the oracle's own
table (orc.resize_taps; reference: image::imageops::resize, crate image 0.24.0, as called from src/shared.rs:159-199):

  * the plain table the library builds equals the oracle's bit for bit (windows and weights);
  * the integer-ratio up-sampling plan (kc_resize_upsample_plan, up_axis_build) is there exactly when the oracle's table has the
    structure upsample.h describes, and the table rebuilt from its class rows is the oracle's table; where it is refused, one of
    the stated reasons holds (up_reasons);
  * the down2 records and padded rows (kc_resize_down2_plan, down2_build) hold exactly the plain table, by the checks of
    test_down2_host.py, the strips cover the outputs and no strip reads more than 64 quads; where they are refused, a reason of
    the header holds;
  * a census: the sets really contain the structures the sweep claims to reach.  A set that lacks one is extended in
    resize_pairs.py; the census is not weakened.

The survey (all tables of all pairs, once per module) takes about 3 s."""
import numpy as np
import pytest

import resize_pairs as rp
from test_upsample_host import up_class

MAX_CHUNKS = 4  # KC_DOWN2_MAX_CHUNKS (csrc/kc_internal.hpp): chunks of 16 source rows per group of four output rows


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    return kc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


class Axis:
    """One (n_in, n_out, filter): the oracle's table and the library's two plans."""

    def __init__(self, kc, orc, n_in, n_out, filt):
        f = kc.ResizeFilter.parse(filt)
        self.n_in, self.n_out, self.filt = n_in, n_out, filt
        self.left, self.count, self.w = orc.resize_taps(n_in, n_out, filt)
        self.left, self.count = self.left.astype(np.int64), self.count.astype(np.int64)
        self.stride = int(self.count.max())
        self.up = kc.resize_upsample_plan(n_in, n_out, f)
        self.d2 = kc.resize_down2_plan(n_in, n_out, f)
        self.what = "%s %d->%d" % (filt, n_in, n_out)

    def group_spans(self):
        """(lo, hi) of the union of the windows of every group of four outputs."""
        out = []
        for y0 in range(0, self.n_out, 4):
            y1 = min(self.n_out, y0 + 4)
            out.append((int(self.left[y0:y1].min()), int((self.left[y0:y1] + self.count[y0:y1]).max())))
        return out

    def chunks(self):
        return max(-(-(hi - lo) // 16) for lo, hi in self.group_spans())


@pytest.fixture(scope="module")
def survey(kc, orc):
    return {(i, o, f): Axis(kc, orc, i, o, f) for f in rp.FILTERS for i, o in rp.ABC}


def axes(survey, filt):
    return [survey[(i, o, filt)] for i, o in rp.ABC]


# ------------------------------------------------------------------ the sets
N_B, N_C, N_ABC, N_CASES = 827, 81, 1289, 3282  # distinct pairs of B, of C, of A, B and C together; all cases


def test_the_sets_are_the_ones_the_sweep_counts_on():
    assert len(rp.A) == 576 and len(set(rp.A)) == 576
    assert (len(rp.B), len(rp.C), len(rp.ABC), len(rp.EXTRA)) == (N_B, N_C, N_ABC, N_ABC - 576)
    assert len(rp.D_DOWN) == 32 and len(set(rp.D_DOWN)) == 32 and len(rp.D_UP) == 64 and len(set(rp.D_UP)) == 64
    assert all(i >= 1 and o >= 1 for i, o in rp.ABC + rp.D_DOWN + rp.D_UP)
    kinds = {k: sum(c.kind == k for c in rp.CASES) for k in ("A", "BC", "D_down", "D_up")}
    assert kinds == {"A": 576, "BC": 2 * len(rp.EXTRA), "D_down": 32 * 32, "D_up": 64 * 4}
    assert len(rp.CASES) == N_CASES and len(rp.D_CASES) == 1280 and len(rp.FUSED_CASES) == 576 + 256
    assert len({(c.v, c.h) for c in rp.D_CASES}) == 1280  # the four partners of an up-sampling pair are four pairs
    # every pair of A, B and C is a vertical table at least once and a horizontal one at least once (for each filter: the cases
    # are the same for all five)
    assert set(rp.ABC) <= {c.v for c in rp.CASES} and set(rp.ABC) <= {c.h for c in rp.CASES}
    assert [c.planes for c in rp.CASES[:4]] == [1, 4, 1, 4] and [c.index for c in rp.CASES] == list(range(len(rp.CASES)))
    for c in rp.CASES:
        (sw, sh), (dw, dh) = c.src, c.dst
        if c.kind.startswith("D"):
            assert max(sw, sh) <= 265 and max(dw, dh) <= 265
        else:
            assert min(sw, sh) <= 24 and max(sw, sh) <= 2056 and min(dw, dh) <= 24 and max(dw, dh) <= 2056, c


def test_the_sources_carry_their_edge_values():
    seen = set()
    for c in rp.CASES[::7]:
        src = rp.sources(c)
        assert len(src) == c.planes and all(p.shape == (c.src[1], c.src[0]) and p.dtype == np.float32 for p in src)
        for k, p in enumerate(src):
            edge = np.zeros(p.shape, bool)
            for r in (0, -1):
                for x in rp.edge_columns(p.shape[1]):
                    edge[r, x] = True
            twins = edge.copy()  # (a 3e38 sample has its twin in the row below it, on the last row above it)
            twins[1:] |= edge[:-1]
            twins[:-1] |= edge[1:]
            body = p[~twins]
            assert np.isfinite(body).all() and (body >= -0.25).all() and (body < 1.25).all()
            assert rp.harsh(c, k) or np.isfinite(p).all()
            if rp.harsh(c, k) and edge.sum() >= 8:  # a whole turn of util.SALT_VALUES
                assert not np.isfinite(p[edge]).all()
                seen.add(c.planes)
    assert seen == {1, 4}


# ------------------------------------------------------------------ the plain table
@pytest.mark.parametrize("filt", rp.FILTERS)
def test_the_library_builds_the_oracles_table(survey, filt):
    for a in axes(survey, filt):
        p = a.d2
        assert p["stride"] == a.stride and p["min_count"] == int(a.count.min()), a.what
        assert np.array_equal(p["left"], a.left) and np.array_equal(p["count"], a.count), a.what
        assert np.array_equal(p["w"].view(np.uint32), a.w.view(np.uint32)), a.what


# ------------------------------------------------------------------ up-sampling
def up_reasons(a):
    """Why up_axis_build must refuse the axis, from the oracle's table alone; empty: it must accept it."""
    if a.n_out % a.n_in:
        return ["not a whole ratio"]
    out = []
    if a.stride % 2 == 0:
        out.append("an even window")
    if a.stride > 7:
        out.append("more than 7 taps")
    if not out:
        # (windows longer than a short source are all cut to it: their starts are not o / R - off)
        u = np.arange(a.n_out) // (a.n_out // a.n_in) - (a.stride - 1) // 2
        if not (np.array_equal(a.left, np.maximum(u, 0)) and np.array_equal(a.left + a.count, np.minimum(u + a.stride, a.n_in))):
            out.append("windows that are not the fixed-length window of o / R cut to the source")
    return out


@pytest.mark.parametrize("filt", rp.FILTERS)
def test_upsample_plan_rebuilds_the_table_or_is_refused_for_a_reason(survey, filt):
    for a in axes(survey, filt):
        why, plan = up_reasons(a), a.up
        if plan is None:
            assert why, "%s: refused although the table has the structure" % a.what
            continue
        assert not why, "%s: accepted although %s" % (a.what, why)
        R, T, off, b_lo, b_hi = (plan[k] for k in ("ratio", "taps", "off", "b_lo", "b_hi"))
        assert (R, T, off) == (a.n_out // a.n_in, a.stride, (a.stride - 1) // 2), a.what
        assert plan["rows"].shape == (R + b_lo + b_hi, T) and b_lo + b_hi <= a.n_out, a.what
        laid = np.zeros((a.n_out, T), np.float32)  # every window of the oracle's table from its unclamped start
        for o in range(a.n_out):
            u = o // R - off
            lo, n = int(a.left[o]), int(a.count[o])
            laid[o, lo - u:lo - u + n] = a.w[o, :n]
        got = np.stack([plan["rows"][up_class(plan, a.n_out, o)] for o in range(a.n_out)])
        assert np.array_equal(got.view(np.uint32), laid.view(np.uint32)), a.what  # weights and the +0.0 outside the source
        # the border classes are no longer than they must be
        ref = (a.n_in // 2) * R
        phase = lambda o: laid[ref + o % R].view(np.uint32)
        assert b_lo <= ref and b_hi <= a.n_out - ref - R, a.what
        assert b_lo == 0 or not np.array_equal(laid[b_lo - 1].view(np.uint32), phase(b_lo - 1)), a.what
        assert b_hi == 0 or not np.array_equal(laid[a.n_out - b_hi].view(np.uint32), phase(a.n_out - b_hi)), a.what


# ------------------------------------------------------------------ down2
def d2_refusals(a):
    """Why down2_build gives no vertical records (nc == 0), from the oracle's table alone; empty: it must give them."""
    if a.n_in <= a.n_out:
        return ["not a down-sampling axis"]
    if a.stride < 4:
        return ["fewer than 4 taps"]  # (the register-tap kernels' ground; the header's "at most 8" is the older bound)
    return ["a group's windows span more than 64 source samples"] if a.chunks() > MAX_CHUNKS else []


@pytest.mark.parametrize("filt", rp.FILTERS)
def test_down2_vertical_records_hold_exactly_the_table(survey, filt):
    for a in axes(survey, filt):
        p, why = a.d2, d2_refusals(a)
        if why:
            assert p["nc"] == 0 and p["vrec"] is None, "%s: records although %s" % (a.what, why)
            continue
        nc = p["nc"]
        assert nc == a.chunks() and 1 <= nc <= MAX_CHUNKS, "%s: nc %d, the windows need %d" % (a.what, nc, a.chunks())
        wbits, rec = a.w.view(np.uint32), p["vrec"]
        assert rec.shape == (-(-a.n_out // 4), nc, 72), a.what
        for g, (lo, hi) in enumerate(a.group_spans()):
            used = -(-(hi - lo) // 16)
            want = np.zeros((nc, 72), np.uint32)
            taps = {y: 0 for y in range(4 * g, min(a.n_out, 4 * g + 4))}
            for ch in range(nc):
                # loads are clamped to the last sample of the group's windows: never past them
                assert lo <= rec[g, ch, 0] <= hi - 1, (a.what, g, ch)
                want[ch, 0], want[ch, 3], want[ch, 4], want[ch, 5] = rec[g, ch, 0], hi - 1, used, -(-(hi - lo) // 8)
                if ch >= used:
                    continue  # mask and weights stay zero
                s0, mask = lo + 16 * ch, 0
                want[ch, 0] = s0
                for y in taps:
                    k, l, n = y - 4 * g, int(a.left[y]), int(a.count[y])
                    s_lo, s_hi = max(s0, l), min(s0 + 16, l + n)
                    if s_lo < s_hi:
                        u = np.arange(s_lo - s0, s_hi - s0)
                        want[ch, 8 + 4 * u + k] = wbits[y, s_lo - l:s_hi - l]
                        mask |= sum(1 << int(4 * v + k) for v in u)
                        taps[y] += len(u)
                want[ch, 1], want[ch, 2] = mask & 0xFFFFFFFF, mask >> 32
            assert np.array_equal(rec[g], want), (a.what, g)
            assert all(taps[y] == a.count[y] for y in taps), (a.what, g)  # every tap once


@pytest.mark.parametrize("filt", rp.FILTERS)
def test_down2_horizontal_rows_and_strips(survey, filt):
    for a in axes(survey, filt):
        p = a.d2
        if a.n_in <= a.n_out or a.stride < 4 or -(-a.stride // 4) > 8:
            assert p["hstride"] == 0 and p["tile_w"] == 0 and p["hw"] is None, a.what
            continue
        hs, tw = p["hstride"], p["tile_w"]
        assert hs % 4 == 0 and a.stride <= hs < a.stride + 4, a.what
        keep = np.arange(hs)[None, :] < a.count[:, None]
        padded = np.zeros((a.n_out, hs), np.float32)
        padded[:, :a.stride] = a.w
        assert np.array_equal(p["hw"].view(np.uint32), np.where(keep, padded.view(np.uint32), 0)), a.what
        cols_per_lane = 3 if hs // 4 <= 3 else 2 if hs // 4 == 4 else 1
        assert 1 <= tw <= 64 * cols_per_lane, a.what
        starts = list(range(0, a.n_out, tw))
        assert starts[0] == 0 and starts[-1] < a.n_out <= starts[-1] + tw  # the strips cover [0, out_n), the last one not empty
        for x0 in starts:
            x1 = min(a.n_out, x0 + tw)
            c0 = int(a.left[x0]) & ~3
            assert (int(a.left[x1 - 1] + a.count[x1 - 1]) - c0 + 3) // 4 <= 64, (a.what, x0)
            assert int(a.left[x0:x1].min()) >= c0  # (window starts ascend: the strip's first column has the leftmost one)


# ------------------------------------------------------------------ the census
def test_census_of_the_structures_the_sets_contain(survey):
    have = set()
    for a in survey.values():
        if a.up is not None:
            u = a.up
            have.add("up b_lo == 0" if u["b_lo"] == 0 else "up b_lo > 0")
            if u["b_hi"] > u["b_lo"]:
                have.add("up b_hi > b_lo")
            if u["ratio"] == 2:
                have.add("up ratio 2, out_n %% 4 %s 0, in_n %s 8" % ("==" if a.n_out % 4 == 0 else "!=", ">=" if a.n_in >= 8 else "<"))
            if u["ratio"] > 1:
                have.add("up ratio % 4 == 0" if u["ratio"] % 4 == 0 else "up ratio % 4 != 0")
            have.add("up taps %d" % u["taps"])
            have.add("up out_n %% 4 == %d" % (a.n_out % 4))
        if a.d2["nc"]:
            have.add("down2 nc %d" % a.d2["nc"])
            have.add("down2 out_n %% 4 == %d" % (a.n_out % 4))
        else:
            have.update("down2 refused: " + w for w in d2_refusals(a))
        if a.n_in > a.n_out and a.stride >= 4:
            have.add("down2 horizontal" if a.d2["hstride"] else "down2 horizontal refused: more than 32 taps")
            if a.d2["tile_w"] and a.d2["tile_w"] < a.n_out:
                have.add("down2 several strips")
    for c in rp.CASES:
        for axis, p in (("vertical", c.v), ("horizontal", c.h)):
            if p[0] == 1:
                have.add("%s n_in == 1" % axis)
            if p[1] == 1:
                have.add("%s n_out == 1" % axis)
    want = ["up b_lo == 0", "up b_lo > 0", "up b_hi > b_lo", "up ratio % 4 == 0", "up ratio % 4 != 0",
            "down2 refused: not a down-sampling axis", "down2 refused: fewer than 4 taps",
            "down2 refused: a group's windows span more than 64 source samples",
            "down2 horizontal", "down2 horizontal refused: more than 32 taps", "down2 several strips"]
    want += ["up ratio 2, out_n %% 4 %s 0, in_n %s 8" % (m, n) for m in ("==", "!=") for n in (">=", "<")]
    want += ["up taps %d" % t for t in (1, 3, 5, 7)]
    want += ["down2 nc %d" % n for n in range(1, MAX_CHUNKS + 1)]
    want += ["%s out_n %% 4 == %d" % (k, m) for k in ("up", "down2") for m in range(4)]
    want += ["%s %s == 1" % (axis, n) for axis in ("vertical", "horizontal") for n in ("n_in", "n_out")]
    missing = [w for w in want if w not in have]
    assert not missing, "the sets lack: %s" % missing
    assert not have - set(want), "counted but not asked for: %s" % sorted(have - set(want))


# ------------------------------------------------------------------ the oracle's side of the device sweep
def test_the_oracle_resamples_every_case(orc):
    """Shapes, NaN-safe comparison and the edge values' reach, for one filter of each window length class."""
    nan_cases = finite_cases = 0
    for filt in ("Triangle", "Lanczos3"):
        for c in rp.CASES[::3]:
            src = rp.sources(c)
            for k, p in enumerate(src):
                want = orc.resize_plane(p, c.dst[0], c.dst[1], filt)
                assert want.shape == (c.dst[1], c.dst[0]) and rp.first_difference(want, want.copy()) is None
                ok = ~np.isnan(want)
                assert (want[ok] >= 0).all() and (want[ok] <= 1).all()
                if rp.harsh(c, k):
                    nan_cases += int((~ok).any())
                else:
                    assert ok.all(), c
                    finite_cases += 1
    assert nan_cases >= 500 and finite_cases >= 500
    a = np.array([[np.nan, 1.0], [0.0, -0.0]], np.float32)
    b = np.array([[np.nan, 1.0], [0.0, 0.0]], np.float32)
    assert rp.first_difference(a, a.copy()) is None and rp.first_difference(a, b) == (1, 1, "0x80000000", "0x00000000")
