"""GPU parity of every resample form at the smallest shapes where it can still go wrong: the cases of tests/resize_pairs.py
(every axis pair up to 24 x 24, whole ratios and their neighbours, outputs on quad, tile and strip edges, and two crosses of
structured axes), each as ONE kc.resize_image(SlotImage.from_planes(src), (dw, dh), filter).materialize(), every plane equal to
orc.resize_plane bit for bit (any NaN equals any NaN), under the planner's own choice and under the options that force the other
forms.  Reference: image::imageops::resize (crate image 0.24.0) as called from src/shared.rs:159-199.

A test id is one filter under one option mode and runs all of the mode's cases; per case it records which counters of
test_gpu_resize_variants.COUNTERS moved and how many kernels were launched.  A failure names the filter, both pairs, the plane
count, the mode, the form that ran and the first differing (plane, y, x) with both bit patterns.  The fused tests evaluate
mix_process(base, resize_image(small, size, filter), Add) against orc.mix_plane("Add", base, orc.resize_plane(...)); a case
the runtime does not fuse is compared all the same.  The last test is the census over the whole module.

Cases per filter: 3282 in each of the modes default, resize_mode 2, 3 and 4 (576 of set A, 1426 of B and C, 1024 + 256 of D);
1280 (D) in each of the twelve D modes of resize_pairs.MODES_D; 832 fused cases (A and the up-sampling D cases) for Nearest and
Triangle each.  In all 5 x (4 x 3282 + 12 x 1280) + 2 x 832 = 144104 resamples.

Tap tables: the cases need 1289 distinct axis pairs (the D pairs are all pairs of B), so 6445 (n_in, n_out, filter) tables in the
five filters; get_taps keeps each in a device block of its own for the life of the process.

Counters of COUNTERS the census does not ask for, with the condition of plan_poly / plan_poly2 (csrc/resize.cpp) that excludes
them at these sizes -- the band height is 4 rows while a row of bands times the bands has at most 1100 waves:
  poly_rows_8, poly_rows_12:   need gx * planes * ceil(regular / 4) > 1100 band waves; here gx = 1, planes <= 4, regular <= 252 (2056 -> 257)
  poly_rows_32:                needs gx * planes * ceil(regular / 12) >= 6000
  poly2_rows_8, poly2_rows_12: need 4 * n_wgx * planes * ceil(regular / 4) > 1100; here n_wgx = 1, planes <= 4, regular <= 252
  poly2_rows_24:               needs 4 * n_wgx * planes * ceil(regular / 12) >= 6000

Run time on an MI355X: 30 s for the module (84 tests); the slowest test id, Lanczos3-default, takes 0.93 s for its 3282 cases
(0.28 ms a case, references included), resize_mode 3 about 0.6 s, a D mode about 0.2 s.  The
6445 live tap tables cost nothing that shows: the last filter's ids are as fast as the first one's."""
import time

import numpy as np
import pytest

import resize_pairs as rp
from test_gpu_resize_variants import COUNTERS, deltas, snapshot

pytestmark = pytest.mark.gpu

FORMS = [n for n in COUNTERS if n.endswith("_launches")]
SEEN_ONCE = ["upsample_half_quads", "down2_by_rows", "down2_xcd_order", "poly2_xcd_order", "upsample_nt_stores"]
EXEMPT = ["poly_rows_8", "poly_rows_12", "poly_rows_32", "poly2_rows_8", "poly2_rows_12", "poly2_rows_24"]  # (module docstring)
FUSED_FORMS = ["resize_chain_launches", "upsample_chain_launches"]
MODES = dict(rp.MODES_ALL + rp.MODES_D)
RUNS = [(f, m) for f in rp.FILTERS for m, _ in rp.MODES_ALL] + [(f, m) for f in rp.FILTERS for m, _ in rp.MODES_D]
MAX_REPORTED = 5  # failing cases spelled out per test id

_CASES_RUN = {}   # (filter, mode) -> cases compared
_FORM_CASES = {}  # (counter, planes) -> cases in which it moved
_SEEN = set()     # every counter that moved in some case
_FUSED = {}       # did the runtime fuse the case? -> fused cases
_TIMES = {}       # test id -> seconds
_WANT = {}        # the one filter whose references are kept: {"filter": name, case index: planes}


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    return kc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


@pytest.fixture
def mode(kc):
    """Sets a mode's options; whatever it set is put back after the test."""
    saved = {}

    def enter(name):
        for opt, value in MODES[name].items():
            saved.setdefault(opt, kc.get_option(opt))
            kc.set_option(opt, value)
    yield enter
    for opt, value in saved.items():
        kc.set_option(opt, value)


def want_planes(orc, case, filt):
    """orc.resize_plane of the case's sources, computed once per filter (the test ids of a filter run one after another)."""
    if _WANT.get("filter") != filt:
        _WANT.clear()
        _WANT["filter"] = filt
    if case.index not in _WANT:
        _WANT[case.index] = [orc.resize_plane(p, case.dst[0], case.dst[1], filt) for p in rp.sources(case)]
    return _WANT[case.index]


def form_of(seen):
    return "+".join(n[:-len("_launches")] for n in FORMS if n in seen) or "no resize form"


def compare(got, want, what, failures):
    """Appends a description of the first difference to `failures`; True when every plane is bit-equal."""
    if len(got) != len(want):
        failures.append("%s: %d planes, expected %d" % (what, len(got), len(want)))
        return False
    for c, (g, w) in enumerate(zip(got, want)):
        d = rp.first_difference(g, w)
        if d is not None:
            failures.append("%s: first difference at (plane %d, y %d, x %d): got %s, oracle %s" % ((what, c) + d))
            return False
    return True


def tally(case, seen):
    _SEEN.update(seen)
    for n in seen:
        if n.endswith("_launches"):
            _FORM_CASES[(n, case.planes)] = _FORM_CASES.get((n, case.planes), 0) + 1


def report(failures, n_cases, what):
    assert not failures, "%s: %d of %d cases differ from the oracle or launched otherwise than one resample does:\n%s" % (
        what, len(failures), n_cases, "\n".join(failures[:MAX_REPORTED]))


@pytest.mark.parametrize("filt,mode_name", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_every_case_equals_the_oracle(kc, orc, mode, filt, mode_name):
    t0 = time.perf_counter()
    cases = rp.CASES if mode_name in dict(rp.MODES_ALL) else rp.D_CASES
    f = kc.ResizeFilter.parse(filt)
    mode(mode_name)
    failures, done = [], 0
    for case in cases:
        want = want_planes(orc, case, filt)
        img = kc.SlotImage.from_planes(rp.sources(case))
        before = snapshot(kc)
        try:
            out = kc.resize_image(img, case.dst, f)
            out.materialize()
        except kc.TexProError as e:  # a refused case is a failed case; the sweep goes on
            failures.append("%s %r, mode %s: refused: %s" % (filt, case, mode_name, e))
            continue
        seen, launches = deltas(kc, before)
        what = "%s %r, mode %s, ran %s %s" % (filt, case, mode_name, form_of(seen), {n: v for n, v in seen.items() if n not in FORMS})
        forms = [n for n in FORMS if n in seen]
        # one resample: one form, counted once (two_pass: once per plane, a vertical and a horizontal launch each)
        two_pass = forms == ["resize_two_pass_launches"]
        expect = 2 * case.planes if two_pass else 1
        if len(forms) != 1 or seen[forms[0]] != (case.planes if two_pass else 1) or launches != expect:
            failures.append("%s: %d launches, expected %d of one form" % (what, launches, expect))
        elif mode_name == "mode3" and not two_pass or mode_name == "default" and two_pass:
            failures.append("%s: not the form of the mode" % what)
        else:
            compare(out.planes(), want, what, failures)
        tally(case, seen)
        done += 1
    _CASES_RUN[(filt, mode_name)] = done
    _TIMES["%s-%s" % (filt, mode_name)] = time.perf_counter() - t0
    report(failures, done, "%s, mode %s" % (filt, mode_name))


@pytest.mark.parametrize("filt", rp.FUSED_FILTERS)
def test_every_fused_case_equals_the_oracle(kc, orc, filt):
    t0 = time.perf_counter()
    f = kc.ResizeFilter.parse(filt)
    failures, done = [], 0
    for case in rp.FUSED_CASES:
        small, base = rp.sources(case), rp.bases(case)
        up = kc.resize_image(kc.SlotImage.from_planes(small), case.dst, f)
        left = kc.SlotImage.from_planes(base)
        before = snapshot(kc)
        got = kc.mix_process(left, up, kc.MixType.Add).planes()
        seen, launches = deltas(kc, before)
        what = "%s %r, fused with Add, ran %s" % (filt, case, form_of(seen))
        # (an RGBA Mix gives alpha 1: src/node/mix.rs:51-134)
        want = [orc.mix_plane("Add", base[c], orc.resize_plane(small[c], case.dst[0], case.dst[1], filt)) for c in range(min(case.planes, 3))]
        if case.planes == 4:
            want.append(np.ones_like(want[0]))
        compare(got, want, what, failures)
        fused = [n for n in FUSED_FORMS if n in seen]
        if fused and (len(seen) != 1 or seen[fused[0]] != 1):
            failures.append("%s: a fused launch next to %s" % (what, seen))
        tally(case, seen)
        _FUSED[bool(fused)] = _FUSED.get(bool(fused), 0) + 1
        done += 1
    _CASES_RUN[(filt, "fused")] = done
    _TIMES["%s-fused" % filt] = time.perf_counter() - t0
    report(failures, done, "%s, fused" % filt)


def test_narrow_output_with_long_horizontal_windows_runs_as_poly(kc, orc):
    """Found by the sweep (Gaussian and Lanczos3, default mode): 176 x 88 -> 22 x 22.  The vertical ratio 4 picks
    resize_poly_kernel, whose four waves each stage their strip's horizontal taps; the planner took the 64-column tile although
    the image is 22 columns wide, and 4 x (64 columns x 49 taps) floats are more than 64 KB of LDS: the launch was refused
    ("resize launch: invalid argument").  choose_tile (csrc/resize.cpp) now takes no tile wider than the image."""
    case = next(c for c in rp.D_CASES if (c.v, c.h) == ((88, 22), (176, 22)))
    for filt in ("Gaussian", "Lanczos3"):
        before = snapshot(kc)
        out = kc.resize_image(kc.SlotImage.from_planes(rp.sources(case)), case.dst, kc.ResizeFilter.parse(filt))
        out.materialize()
        seen, launches = deltas(kc, before)
        assert launches == 1 and seen == {"resize_poly_launches": 1, "poly_rows_4": 1}, seen
        failures = []
        compare(out.planes(), [orc.resize_plane(p, 22, 22, filt) for p in rp.sources(case)], "%s %r" % (filt, case), failures)
        assert not failures, failures


# ------------------------------------------------------------------ the census
def test_the_sweep_reached_what_it_claims():
    """Runs after the other tests of this file: every case of every filter and mode was compared (none skipped or refused: the
    exact counts), every form ran on at least 20 cases with 1 plane and with 4 planes, and the variants were seen."""
    expected = {(f, m): len(rp.CASES) for f in rp.FILTERS for m, _ in rp.MODES_ALL}
    expected.update({(f, m): len(rp.D_CASES) for f in rp.FILTERS for m, _ in rp.MODES_D})
    expected.update({(f, "fused"): len(rp.FUSED_CASES) for f in rp.FUSED_FILTERS})
    if set(_CASES_RUN) != set(expected):
        pytest.skip("only meaningful after all %d sweep tests of this module have run (%d did)" % (len(expected), len(_CASES_RUN)))
    assert (len(rp.CASES), len(rp.D_CASES), len(rp.FUSED_CASES)) == (3282, 1280, 832)
    assert _CASES_RUN == expected
    assert sum(_CASES_RUN.values()) == 5 * (4 * 3282 + 12 * 1280) + 2 * 832 == 144104
    print("\nresize pairs: cases per (form, planes): %s\ncounters seen: %s\nfused or not: %s\nseconds per test id: %s" % (
        sorted(_FORM_CASES.items()), sorted(_SEEN), _FUSED, sorted(_TIMES.items(), key=lambda kv: -kv[1])[:8]))
    thin = {(n, p): _FORM_CASES.get((n, p), 0) for n in FORMS for p in (1, 4) if _FORM_CASES.get((n, p), 0) < 20}
    assert not thin, "forms that ran on fewer than 20 cases: %s" % thin
    assert not [n for n in SEEN_ONCE if n not in _SEEN], "never seen: %s" % [n for n in SEEN_ONCE if n not in _SEEN]
    assert set(COUNTERS) - set(FORMS) - set(SEEN_ONCE) - set(EXEMPT) <= _SEEN  # poly_rows_4, poly2_rows_4
    assert not set(EXEMPT) & _SEEN, "reached after all: take %s out of EXEMPT" % sorted(set(EXEMPT) & _SEEN)
