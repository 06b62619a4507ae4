"""GPU parity of every plane-reading kernel on CALLER-OWNED planes (kc_plane_wrap) of any legal pitch and base alignment.

kc_plane_wrap accepts any 16-byte-aligned pointer and any pitch that is a multiple of 16 and at least 16 * ceil(w / 4); the
library may read, for each row y, the 16 * ceil(w / 4) bytes from ptr + y * pitch, and nothing else, and never writes there.
Here every source is a view into a larger tensor the test owns (util.wrapped_image): at least 8 guard rows above and below,
guard floats in the last quad's tail, in the padding and before the first column, so a read past the contract lands in the
test's own memory and shows in the result.  Layouts (util.wrap_layout): "tight", "pad48", "offset" (rows 16 bytes off a
32-byte boundary, pitch no multiple of 64 bytes), and for RGBA "mixed" (R tight, G pad48, B offset, A a pool plane -- or a
constant in the chain cases).  Every case runs under two guards: NaN (any use of a foreign float poisons the result) and 1e30
(finite: a kernel whose fast arm needs finite samples stays on it; a zero weight times it is 0, any other weight shows).

Every measured call is ONE call; the family's whole counter vector (kc_stats_counter) says which form ran; the result equals
the reference of the family's own test bit for bit (any NaN equals any NaN) and the same call on a pool image of the same
pixels; afterwards every parent tensor still holds its bits (assert_untouched).  The pool is scrubbed first
(test_gpu_streaming_variants.scrub_planes), so a result block cannot already hold the answer.

A flat compiled chain launch (runtime.cpp chain_dispatch: every pitch dense, P.rows == 1) has no counter of its own; the two
quads per lane form ("_q2", chain_codegen.cpp chain_quads_for) exists for flat signatures only, so a {+, -, *} program under
nt_force 0x101 reads "specialized_nt_101_q2" when the launch is flat and "specialized_nt_101" when it is not.  The signature
the kernel was generated for is read as well, from the list of programs a launch compiles (KC_KERNEL_CACHE_MANIFEST).

Run time on an MI355X: 15 s for the module (75 tests), of which 12 s are the first test's set-up (library start-up); no test
takes longer than 0.25 s.  DESIGN.md section 5 has the mutations these cases were checked against."""
import contextlib
import json
import os

import numpy as np
import pytest

import bc6h_ref
import bc_decode_ref
import bc_modes_ref
from golden_graphs import G
from test_gpu_chain_variants import COUNTERS as CHAIN_COUNTERS, edge_plane
from test_gpu_fuzz_consumers import (ALL_FORMS, BC6H, BC7, BC_ALL_MODES, BC_SRGB, _consume, _flat_record, _ref_blocks, _same,
                                     _want_record)
from test_gpu_resize_variants import COUNTERS as RESIZE_COUNTERS, sources
from test_gpu_streaming_variants import (EXPORT, H2N, U8, bits_to_torch, counted, export_bits, h2n_counters, h2n_ref, height_plane,
                                         is_nan_bits, ones, options, scrub_planes, scrub_staging, torch_to_bits)
from util import MIXED, SEED_A, SEED_B, assert_planes, assert_pow_planes, splitmix_plane, with_edge_cases, wrapped_image

pytestmark = pytest.mark.gpu

LAYOUTS = ["tight", "pad48", "offset"]
GUARDS = [("nan", np.float32(np.nan)), ("1e30", np.float32(1e30))]
OPTIONS = ["cache_budget_mb", "nt_force", "tune_cap", "h2n_tiled", "down2", "down2_by_rows", "poly2", "poly2_min_ratio", "resize_mode",
           "chain1", "join", "wide"]
SPEC_Q = ["specialized_nt_%03x_q%d" % (m | r, q) for m in range(16) for r in (0, 0x100) for q in (2, 4)]
CHAIN = CHAIN_COUNTERS + SPEC_Q + ["join_launches"]
_SAVED = {}
SEEN = set()  # (counter, layout) of every form that ran on a wrapped source


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    _SAVED.update({n: kc.get_option(n) for n in OPTIONS})
    spec, quads = kc.get_specialize(), kc.get_chain_quads()
    try:
        yield kc
    finally:
        for n, v in _SAVED.items():
            kc.set_option(n, v)
        kc.set_specialize(spec)
        kc.set_chain_quads(quads)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@contextlib.contextmanager
def specialize(kc, mode, quads=None):
    saved, q = kc.get_specialize(), kc.get_chain_quads()
    try:
        kc.set_specialize(mode)
        if quads is not None:
            kc.set_chain_quads(quads)
        yield
    finally:
        kc.set_specialize(saved)
        kc.set_chain_quads(q)


def note(seen, layout):
    SEEN.update((n, layout) for n in seen)


_REF = {}


def cached(key, make):
    """A reference computed once per key and shared read-only"""
    if key not in _REF:
        ref = make()
        for r in ref:
            if isinstance(r, np.ndarray):
                r.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


# ------------------------------------------------------------------ resize
def resize_planes(n, sw, sh, dw, dh, finite, seed=SEED_A):
    """test_gpu_resize_variants.sources; for the finite guard the first and last two rows and the last eight columns lie in
    (0.1, 0.9), so a leak of the guard, clamped to 0 or 1, cannot coincide with the true value there"""
    planes = sources(n, sw, sh, dw, dh, seed)
    if finite:
        for c, p in enumerate(planes):
            inner = np.random.default_rng([seed, c, sw, sh]).random((sh, sw), dtype=np.float32) * np.float32(0.7) + np.float32(0.15)
            for sl in (np.s_[:2], np.s_[-2:], np.s_[:, -8:]):
                p[sl] = inner[sl]
    return planes


# (id, filter, source (w, h), destination (w, h), options, counters that read 1 -- the form first, launches of a Gray plane)
RESIZE_CASES = [
    # (these planes fit the cache budget: without the order by rows the tiles go to the XCDs in turn; one strip has nothing to
    # order by rows, resize.cpp plan_down2)
    ("down2_catmull_rows0", "CatmullRom", (130, 70), (61, 33), {"down2_by_rows": 0}, ["down2_launches", "down2_xcd_order"], 1),
    ("down2_catmull_rows1", "CatmullRom", (130, 70), (61, 33), {"down2_by_rows": 1}, ["down2_launches", "down2_xcd_order"], 1),
    ("down2_lanczos_rows0", "Lanczos3", (700, 300), (513, 219), {"down2_by_rows": 0}, ["down2_launches", "down2_xcd_order"], 1),
    ("down2_lanczos_rows1", "Lanczos3", (700, 300), (513, 219), {"down2_by_rows": 1}, ["down2_launches", "down2_by_rows"], 1),
    ("down2_triangle_rows0", "Triangle", (1030, 70), (515, 35), {"down2_by_rows": 0}, ["down2_launches", "down2_xcd_order"], 1),
    ("down2_triangle_rows1", "Triangle", (1030, 70), (515, 35), {"down2_by_rows": 1}, ["down2_launches", "down2_by_rows"], 1),
    ("poly2_odd_strips", "Gaussian", (520, 256), (65, 32), {"poly2_min_ratio": 2}, ["poly2_launches", "poly2_rows_4"], 1),
    ("poly2_ratio2", "Gaussian", (1030, 140), (515, 70), {"poly2_min_ratio": 2}, ["poly2_launches", "poly2_rows_4", "poly2_xcd_order"], 1),
    ("poly", "Lanczos3", (1000, 96), (250, 24), {"poly2": 0}, ["resize_poly_launches", "poly_rows_4"], 1),
    ("down_ratio4", "Lanczos3", (1000, 96), (250, 24), {"down2": 0, "resize_mode": 1}, ["resize_down_launches"], 1),
    ("down", "Lanczos3", (260, 333), (190, 64), {"down2": 0, "resize_mode": 1}, ["resize_down_launches"], 1),
    ("lds_lanczos", "Lanczos3", (37, 29), (100, 77), {}, ["resize_lds_launches"], 1),
    ("lds_gaussian", "Gaussian", (70, 70), (300, 300), {}, ["resize_lds_launches"], 1),
    ("wide", "Gaussian", (300, 70), (70, 300), {}, ["resize_wide_launches"], 1),
    ("two_pass", "CatmullRom", (131, 67), (97, 141), {"resize_mode": 3}, ["resize_two_pass_launches"], 2),
    ("upsample_triangle_x8", "Triangle", (16, 16), (128, 128), {}, ["upsample_launches"], 1),
    # (Lanczos3's border classes need 7 source samples: 37 x 5 goes to resize_lds_kernel)
    ("upsample_lanczos_x4", "Lanczos3", (37, 7), (148, 28), {}, ["upsample_launches"], 1),
    ("upsample_half_quads", "CatmullRom", (64, 32), (128, 64), {}, ["upsample_launches", "upsample_half_quads"], 1),
]


@pytest.mark.parametrize("case", RESIZE_CASES, ids=[c[0] for c in RESIZE_CASES])
def test_resize_of_a_wrapped_source(kc, orc, torch, case):
    name, filt, (sw, sh), (dw, dh), opts, expect, gray_launches = case
    f = kc.ResizeFilter.parse(filt)
    for gname, guard in GUARDS:
        finite = bool(np.isfinite(guard))
        src = cached(("resize src", name, finite), lambda: resize_planes(4, sw, sh, dw, dh, finite))
        want = cached(("resize", name, finite), lambda: [orc.resize_plane(p, dw, dh, filt) for p in src])
        results = {}
        for layout in LAYOUTS + ["mixed", "pool"]:
            n = 4 if layout == "mixed" else 1
            if layout == "pool":
                wi, img = None, kc.SlotImage.from_planes(src)
                n = 4
            else:
                wi = wrapped_image(kc, torch, src[:n], MIXED if layout == "mixed" else layout, guard)
                img = wi.image
            scrub_planes(kc, dw, dh)
            out, seen, launches = counted(kc, RESIZE_COUNTERS, opts, lambda: kc.resize_image(img, (dw, dh), f).materialize())
            what = "%s %s guard %s" % (name, layout, gname)
            two_pass = "resize_two_pass_launches" in expect
            exp = {k: (n if two_pass else 1) for k in expect}
            assert seen == exp and launches == (gray_launches * n if two_pass else 1), "%s: %d launches, counters %s, expected %s" % (
                what, launches, seen, exp)
            got = out.planes()
            assert_planes(got, want[:n], what=what)
            results[layout] = got
            if wi is not None:
                wi.assert_untouched()
                note(seen, layout)
        for layout in LAYOUTS:
            assert_planes(results[layout], results["pool"][:1], what="%s %s against the pool image" % (name, layout))
        assert_planes(results["mixed"], results["pool"], what="%s mixed against the pool image" % name)


# the three-node Add / Multiply / Subtract blend of test_resize_chain_many_tiles: the small operand is resampled inside the launch
# of the chain that consumes it.  (id, small (w, h), big (w, h), specialize, layout of the small / of the full-size operand, counter)
RESIZE_CHAIN_CASES = [
    ("upsample_chain_interp", (130, 12), (2080, 96), 0, "offset", "pad48", "upsample_chain_launches"),
    ("upsample_chain_compiled", (130, 12), (2080, 96), 2, "tight", "offset", "upsample_chain_launches"),
    ("resize_chain_interp", (100, 100), (410, 410), 0, "pad48", "offset", "resize_chain_launches"),
    ("resize_chain_compiled", (100, 100), (410, 410), 2, "offset", "tight", "resize_chain_launches"),
]


@pytest.mark.parametrize("case", RESIZE_CHAIN_CASES, ids=[c[0] for c in RESIZE_CHAIN_CASES])
def test_resize_inside_a_chain_of_wrapped_operands(kc, orc, torch, case):
    name, (sw, sh), (dw, dh), mode, lay_small, lay_big, counter = case

    def blend(ia, ib):
        up = kc.resize_image(ib, (dw, dh), kc.ResizeFilter.Triangle)
        mix = kc.mix_process
        return mix(mix(mix(ia, up, kc.MixType.Add), ia, kc.MixType.Multiply), up, kc.MixType.Subtract)

    def make_want(small, big):
        out = []
        for c in range(3):
            bu = orc.resize_plane(small[c], dw, dh, "Triangle")
            out.append(orc.mix_plane("Subtract", orc.mix_plane("Multiply", orc.mix_plane("Add", big[c], bu), big[c]), bu))
        return out + [np.ones((dh, dw), np.float32)]

    for gname, guard in GUARDS:
        finite = bool(np.isfinite(guard))
        small = cached(("chain small", name, finite), lambda: resize_planes(4, sw, sh, dw, dh, finite, SEED_B))
        big = cached(("chain big", name), lambda: sources(4, dw, dh, dw, dh))
        want = cached(("resize chain", name, finite), lambda: make_want(small, big))
        results = {}
        with specialize(kc, mode):
            for layout in ("wrapped", "pool"):
                if layout == "pool":
                    ws = wb = None
                    ia, ib = kc.SlotImage.from_planes(big), kc.SlotImage.from_planes(small)
                else:
                    ws = wrapped_image(kc, torch, small, [lay_small] * 3 + [("const", 1.0)], guard)
                    wb = wrapped_image(kc, torch, big, [lay_big] * 3 + [("const", 1.0)], guard)
                    ia, ib = wb.image, ws.image
                scrub_planes(kc, dw, dh)
                img = blend(ia, ib)
                got, seen, launches = counted(kc, RESIZE_COUNTERS, {}, lambda: img.planes())
                what = "%s %s guard %s" % (name, layout, gname)
                assert seen == {counter: 1} and launches == 1, "%s: %d launches, counters %s" % (what, launches, seen)
                assert_planes(got, want, what=what)
                results[layout] = got
                if ws is not None:
                    ws.assert_untouched()
                    wb.assert_untouched()
                    note(seen, lay_small)
        assert_planes(results["wrapped"], results["pool"], what="%s against the pool images" % name)


def band_graph(kind, filt=None, policy="MostPixels"):
    g = G()
    if kind == "h2n":
        e = g.add({"Embed": 0})
        sep = g.add("SeparateRgba")
        g.connect(e, sep, 0, 0)
        node = g.add("HeightToNormal")
        g.connect(sep, node, 0, 0)
    else:
        e0, e1 = g.add({"Embed": 0}), g.add({"Embed": 1})
        node = g.add({"Mix": "Add"}, policy=policy, filt=filt)
        g.connect(e0, node, 0, 0)
        g.connect(e1, node, 0, 1)
    return g.dict(), node


def embedded(kc, graph, images):
    tp = kc.TextureProcessor.new()
    lg = tp.new_live_graph()
    lg.set_node_graph(kc.NodeGraph.from_json(json.dumps(graph)))
    for k, img in images.items():
        lg.embed_slot_data_with_id(kc.SlotData(0, 0, img), k)
    return tp, lg


# One case per form a band's resample can take (a band's vertical tap table has no integer-ratio structure: no up-sampling,
# poly or poly2 kernel).  The first three: the sizes of test_resize_and_height_to_normal_bands, the smaller image resampled to the
# larger one's size (MostPixels); the others the other way round (LeastPixels), at the ratios of the "down" and "wide" cases above.
# (id, filter, (h, w) of image 0, of image 1, policy, options, the form's counter)
BAND_CASES = [("up_x4", "Triangle", (48, 64), (12, 16), "MostPixels", {}, "resize_lds_launches"),
              ("up", "Lanczos3", (40, 72), (131, 200), "MostPixels", {}, "resize_lds_launches"),
              ("one_axis", "CatmullRom", (57, 33), (57, 90), "MostPixels", {}, "resize_lds_launches"),
              ("down2", "Lanczos3", (333, 260), (64, 190), "LeastPixels", {}, "down2_launches"),
              ("down", "Lanczos3", (333, 260), (64, 190), "LeastPixels", {"down2": 0, "resize_mode": 1}, "resize_down_launches"),
              ("two_pass", "Lanczos3", (333, 260), (64, 190), "LeastPixels", {"resize_mode": 3}, "resize_two_pass_launches"),
              ("wide", "Gaussian", (70, 300), (299, 70), "LeastPixels", {}, "resize_wide_launches")]


@pytest.mark.parametrize("case", BAND_CASES, ids=[c[0] for c in BAND_CASES])
def test_resize_bands_of_a_wrapped_embedded_source(kc, orc, torch, case):
    """Embed + Embed -> Mix(Add), both embedded images caller-owned (the Mix resamples one of them to the other's size inside
    its launch): the first, a middle and the last row band against the oracle's crop."""
    name, filt, small, big, policy, opts, form = case
    (h0, w0), (h1, w1) = small, big
    graph, node = band_graph("mix", filt, policy)
    for gname, guard in GUARDS:
        finite = bool(np.isfinite(guard))
        a = cached(("band a", small, big, finite), lambda: resize_planes(4, w0, h0, w1, h1, finite, SEED_B))
        b = cached(("band b", small, big, finite), lambda: resize_planes(4, w1, h1, w0, h0, finite, SEED_A))
        ref = cached(("band ref", filt, small, big, finite),
                     lambda: list(orc.RefGraph(graph, embedded={0: orc.Image(list(a)), 1: orc.Image(list(b))}).slot_data(node, 0).image.planes))
        dh = ref[0].shape[0]
        results = {}
        for i, layout in enumerate(LAYOUTS + ["pool"]):
            wi = None if layout == "pool" else wrapped_image(kc, torch, a, [layout] * 3 + ["pool"], guard)
            wj = None if layout == "pool" else wrapped_image(kc, torch, b, [LAYOUTS[(i + 1) % 3]] * 3 + ["pool"], guard)
            for y0, y1 in ((0, 5), (dh // 2, dh // 2 + 3), (dh - 4, dh)):
                tp, lg = embedded(kc, graph, {0: kc.SlotImage.from_planes(a) if wi is None else wi.image,
                                              1: kc.SlotImage.from_planes(b) if wj is None else wj.image})
                scrub_planes(kc, ref[0].shape[1], y1 - y0)
                got, seen, launches = counted(kc, RESIZE_COUNTERS, opts, lambda: lg.evaluate_band(node, y0, y1).planes())
                what = "%s band %d:%d %s guard %s" % (name, y0, y1, layout, gname)
                forms = {k: v for k, v in seen.items() if k.endswith("_launches")}
                assert set(forms) == {form} and launches >= 1, "%s: %d launches, counters %s" % (what, launches, seen)
                assert_planes(got, [r[y0:y1] for r in ref], what=what)
                results[(layout, y0)] = (got, seen)
                if wi is not None:
                    note(["band:" + k for k in forms], layout)
            if wi is not None:
                wi.assert_untouched()
                wj.assert_untouched()
        for (layout, y0), (got, seen) in results.items():
            assert seen == results[("pool", y0)][1], (layout, y0, seen)
            assert_planes(got, results[("pool", y0)][0], what="%s band at %d %s against the pool image" % (name, y0, layout))


# ------------------------------------------------------------------ chains compiled at run time
CONST = (0.375, -1.25, 2.0)
PROGRAM_DIV = [("Add", False, 1), ("Multiply", True, CONST[0]), ("Subtract", True, 2), ("Divide", False, 1), ("Subtract", False, 0)]
PROGRAM_MUL = [("Add", False, 1), ("Multiply", True, CONST[0]), ("Subtract", True, 2), ("Multiply", False, 1), ("Subtract", False, 0)]


def run_steps(kc, orc, imgs, planes, steps, w, h):
    """(lazy image, None) when orc is None, else the oracle's plane: input 0, then (Mix type, running value on the right, operand)"""
    acc = imgs[0] if orc is None else planes[0]
    for op, right, opnd in steps:
        if orc is None:
            x = imgs[opnd] if isinstance(opnd, int) else kc.SlotImage.from_value((w, h), opnd, False)
            acc = kc.mix_process(x, acc, kc.MixType.parse(op)) if right else kc.mix_process(acc, x, kc.MixType.parse(op))
        else:
            x = planes[opnd] if isinstance(opnd, int) else np.full((h, w), opnd, np.float32)
            acc = orc.mix_plane(op, x, acc) if right else orc.mix_plane(op, acc, x)
    return acc


def chain_inputs(k, h, w):
    return cached(("chain in", k, h, w), lambda: [edge_plane(SEED_A + 17 * i, 0, h, w) for i in range(k)])


# (id, (w, h), program, layout of each input, options, chain_quads, the counter)
COMPILED_CASES = [
    ("nonflat_37x29", (37, 29), PROGRAM_DIV, ["tight", "pad48", "offset"], {}, None, "specialized_nt_000"),
    ("nonflat_64x17_padded", (64, 17), PROGRAM_DIV, ["tight", "pad48", "offset"], {}, None, "specialized_nt_000"),
    ("nonflat_64x17_padded_no_q2", (64, 17), PROGRAM_MUL, ["tight", "pad48", "offset"], {"nt_force": 0x101}, 2, "specialized_nt_101"),
    ("flat_64x17_tight_q2", (64, 17), PROGRAM_MUL, ["tight"] * 3, {"nt_force": 0x101}, 2, "specialized_nt_101_q2"),
    ("flat_128x9_tight", (128, 9), PROGRAM_DIV, ["tight"] * 3, {}, None, "specialized_nt_000"),
    ("flat_128x9_tight_q2", (128, 9), PROGRAM_MUL, ["tight"] * 3, {"nt_force": 0x101}, 2, "specialized_nt_101_q2"),
    ("flat_128x9_tight_rule", (128, 9), PROGRAM_MUL, ["tight"] * 3, {"nt_force": 0x101}, 0, "specialized_nt_101_q2"),
    ("nonflat_128x9_offset", (128, 9), PROGRAM_MUL, ["tight", "tight", "offset"], {"nt_force": 0x101}, 0, "specialized_nt_101"),
]


@pytest.mark.parametrize("case", COMPILED_CASES, ids=[c[0] for c in COMPILED_CASES])
def test_compiled_chain_over_wrapped_inputs(kc, orc, torch, case, tmp_path):
    """The counter says which kernel ran; the signature it was generated for is read from the list of programs the launch
    compiled (KC_KERNEL_CACHE_MANIFEST, kernel_cache.cpp disk_store): the first launch of a case starts from no kernels, in
    memory or on disk, so it compiles exactly its own program, and that program's `flat` must be the case's."""
    name, (w, h), steps, lays, opts, quads, counter = case
    planes = chain_inputs(3, h, w)
    want = cached(("compiled", name), lambda: [run_steps(kc, orc, None, planes, steps, w, h)])
    results = {}
    manifest = tmp_path / "compiled.jsonl"
    with specialize(kc, 2, quads):
        for gname, guard in GUARDS:
            wis = [wrapped_image(kc, torch, [p], lay, guard) for p, lay in zip(planes, lays)]
            scrub_planes(kc, w, h)
            img = run_steps(kc, None, [x.image for x in wis], None, steps, w, h)
            first = not results
            if first:
                kc.specialize_wait()
                kc.kernel_cache_set_dir("off")
                kc.specialize_reset()
                os.environ["KC_KERNEL_CACHE_MANIFEST"] = str(manifest)
            try:
                got, seen, launches = counted(kc, CHAIN, opts, lambda: img.planes())
            finally:
                if first:
                    del os.environ["KC_KERNEL_CACHE_MANIFEST"]
                    kc.kernel_cache_set_dir(None)
            what = "%s guard %s" % (name, gname)
            assert seen == {counter: 1} and launches == 1, "%s: %d launches, counters %s" % (what, launches, seen)
            if first:
                compiled = [json.loads(line) for line in manifest.read_text().splitlines()]
                assert [(c["n_in"], c["flat"], c["up_taps"]) for c in compiled] == [(3, int(name.startswith("flat")), 0)], "%s: compiled %s" % (what, compiled)
            assert_planes(got, want, what=what)
            for x in wis:
                x.assert_untouched()
            note(["flat" if name.startswith("flat") else "nonflat", counter], lays[-1])
            results[gname] = got
        pool = [kc.SlotImage.from_planes([p]) for p in planes]
        got = run_steps(kc, None, pool, None, steps, w, h).planes()
    for gname, _ in GUARDS:
        assert_planes(results[gname], got, what="%s against pool images" % name)


def test_joined_chains_with_one_chain_on_wrapped_sources(kc, orc, torch):
    """(a * b) - (c + d): two chains that have not run meet in one launch (test_gpu_join); a and b are caller-owned."""
    h, w = 33, 50
    a, b, c, d = chain_inputs(4, h, w)
    want = cached(("joined",), lambda: [orc.mix_plane("Subtract", orc.mix_plane("Multiply", a, b), orc.mix_plane("Add", c, d))])
    M = lambda o, l, r: kc.mix_process(l, r, getattr(kc.MixType, o))  # noqa: E731
    with specialize(kc, 2):
        for gname, guard in GUARDS:
            wa, wb = wrapped_image(kc, torch, [a], "offset", guard), wrapped_image(kc, torch, [b], "tight", guard)
            ic, id_ = kc.SlotImage.from_planes([c]).materialize(), kc.SlotImage.from_planes([d]).materialize()
            scrub_planes(kc, w, h)
            z = M("Subtract", M("Multiply", wa.image, wb.image), M("Add", ic, id_))
            got, seen, launches = counted(kc, CHAIN, {"join": 1}, lambda: z.planes())
            assert seen == {"specialized_nt_000": 1, "join_launches": 1} and launches == 1, "joined guard %s: %d launches, counters %s" % (gname, launches, seen)
            assert_planes(got, want, what="joined chains guard %s" % gname)
            wa.assert_untouched()
            wb.assert_untouched()
            note(["join_launches"], "offset")


def test_wide_program_over_wrapped_inputs(kc, orc, torch):
    """Seven planes per channel (more than the interpreter's four: a compiled kernel's "wide" form), cycling through the layouts."""
    w, h, k = 70, 21, 7
    planes = chain_inputs(k, h, w)
    ops = ["Add", "Multiply", "Subtract"]
    steps = [(ops[i % 3], i % 2 == 1, i + 1) for i in range(k - 1)]
    want = cached(("wide",), lambda: [run_steps(kc, orc, None, planes, steps, w, h)])
    with specialize(kc, 2):
        for gname, guard in GUARDS:
            wis = [wrapped_image(kc, torch, [p], LAYOUTS[i % 3], guard) for i, p in enumerate(planes)]
            scrub_planes(kc, w, h)
            img = run_steps(kc, None, [x.image for x in wis], None, steps, w, h)
            got, seen, launches = counted(kc, CHAIN, {"wide": 1}, lambda: img.planes())
            assert seen == {"specialized_nt_000": 1} and launches == 1, "wide guard %s: %d launches, counters %s" % (gname, launches, seen)
            assert_planes(got, want, what="wide program guard %s" % gname)
            for x in wis:
                x.assert_untouched()
            note(["wide"], "offset")


@pytest.mark.parametrize("op", ["Add", "Divide", "Pow"])
@pytest.mark.parametrize("wrapped_side", ["operand", "start"])
def test_one_step_kernel_with_one_wrapped_input(kc, orc, torch, op, wrapped_side):
    """chain1.hip: the start plane and the operand have different pitches and alignments (one pool, one "offset")."""
    w, h = 130, 33
    a, b = chain_inputs(2, h, w)
    want = cached(("chain1", op), lambda: [orc.mix_plane(op, a, b)])
    check = assert_pow_planes if op == "Pow" else assert_planes
    for gname, guard in GUARDS:
        wi = wrapped_image(kc, torch, [b if wrapped_side == "operand" else a], "offset", guard)
        other = kc.SlotImage.from_planes([a if wrapped_side == "operand" else b])
        ia, ib = (other, wi.image) if wrapped_side == "operand" else (wi.image, other)
        scrub_planes(kc, w, h)
        img = kc.mix_process(ia, ib, kc.MixType.parse(op))
        got, seen, launches = counted(kc, CHAIN, {"chain1": 1}, lambda: img.planes())
        what = "%s wrapped %s guard %s" % (op, wrapped_side, gname)
        assert seen == {"chain1_nt0": 1, "chain1_launches": 1} and launches == 1, "%s: %d launches, counters %s" % (what, launches, seen)
        check(got, want, what=what)
        pool = kc.mix_process(kc.SlotImage.from_planes([a]), kc.SlotImage.from_planes([b]), kc.MixType.parse(op)).planes()
        assert_planes(got, pool, what=what + " against pool images")  # the same kernel: the same bits, Pow included
        wi.assert_untouched()
        note(seen, "offset")


# ------------------------------------------------------------------ HeightToNormal
H2N_WRAPPED = [((130, 13), 5, ["pad48", "offset"]), ((262, 7), 6, LAYOUTS), ((517, 5), 7, LAYOUTS), ((1024, 9), 5, LAYOUTS),
               ((2048, 3), 6, LAYOUTS), ((5, 3), 0, LAYOUTS)]
H2N_FORMS = [("default", {}, True), ("plain", {"h2n_tiled": 0}, False)]


@pytest.mark.parametrize("shape,tq,layouts", H2N_WRAPPED, ids=["%dx%d" % s for s, _, _ in H2N_WRAPPED])
def test_h2n_of_a_wrapped_plane(kc, orc, torch, shape, tq, layouts):
    """HeightToNormal wraps around in x and y: the guard rows directly above and below the view, and the guard floats on both
    sides of a row, are what a wrong wrap-around would pick up."""
    w, h = shape
    p = height_plane(w, h)
    want = h2n_ref(orc, shape, p)
    pool = kc.SlotImage.from_planes([p])
    for gname, guard in GUARDS:
        for layout in layouts:
            wi = wrapped_image(kc, torch, [p], layout, guard)
            for name, opts, tiled in H2N_FORMS:
                scrub_planes(kc, w, h)
                got, seen, launches = counted(kc, H2N, opts, lambda: kc.height_to_normal_process(wi.image))
                what = "h2n %dx%d %s %s guard %s" % (w, h, layout, name, gname)
                assert launches == 1 and seen == h2n_counters(tq if tiled else 0), "%s: %d launches, counters %s" % (what, launches, seen)
                got = got.planes()
                assert_planes(got, want, what=what)
                with options(kc, opts):
                    assert_planes(got, kc.height_to_normal_process(pool).planes(), what=what + " against the pool image")
                note(seen, layout)
            wi.assert_untouched()


def test_h2n_band_of_a_wrapped_embedded_source(kc, orc, torch):
    w, h, tq = 130, 13, 5
    p = height_plane(w, h)
    want = h2n_ref(orc, (w, h), p)
    zero = np.zeros_like(p)
    graph, node = band_graph("h2n")
    for gname, guard in GUARDS:
        for layout in LAYOUTS:
            wi = wrapped_image(kc, torch, [p, zero, zero, zero], [layout, "pool", "pool", "pool"], guard)
            for y0, y1 in ((0, 5), (5, 6), (6, h)):
                tp, lg = embedded(kc, graph, {0: wi.image})
                scrub_planes(kc, w, y1 - y0)
                got, seen, launches = counted(kc, H2N, {}, lambda: lg.evaluate_band(node, y0, y1))
                what = "h2n band %d:%d %s guard %s" % (y0, y1, layout, gname)
                assert launches >= 1 and seen == h2n_counters(tq, band=True), "%s: counters %s" % (what, seen)
                assert_planes(got.planes(), [r[y0:y1] for r in want], what=what)
                note(seen, layout)
            wi.assert_untouched()


# ------------------------------------------------------------------ consumers
CONSUMER_SIZES = [(70, 33), (131, 67)]


def consumer_planes(w, h):
    """Values in [-0.2, 1.3) with the IEEE edge cases at the head of every plane and on the last quad of some rows"""
    def make():
        out = []
        for c in range(4):
            p = with_edge_cases(splitmix_plane(SEED_B, c, h, w) * np.float32(1.5) - np.float32(0.2), shift=c + 1)
            p[h // 2, w - 3:] = [np.nan, np.inf, -0.0][c % 3:] + [np.nan, np.inf, -0.0][:c % 3]
            p[h - 1, w - 2:] = [1.25, -0.25]
            out.append(p)
        return out
    return cached(("consumer", w, h), make)


def consumer_sources(kc, orc, torch, w, h, guard):
    """[(kind, WrappedImage, oracle image, channel keys)]: `mixed` RGBA and `offset` Gray"""
    p = consumer_planes(w, h)
    return [("mixed", wrapped_image(kc, torch, p, MIXED, guard), orc.Image(list(p)), ["tight", "pad48", "offset", "pool"]),
            ("offset", wrapped_image(kc, torch, p[:1], "offset", guard), orc.Image([p[0]]), ["offset"])]


def rgba_view(image):
    p = list(image.planes)
    return p if len(p) == 4 else [p[0], p[0], p[0], np.ones_like(p[0])]


@pytest.mark.parametrize("size", CONSUMER_SIZES, ids=lambda s: "%dx%d" % s)
def test_to_u8_and_to_f32_of_wrapped_planes(kc, orc, torch, size):
    from kanter_core_amd import _lib
    L = _lib.load()
    w, h = size
    half = np.full((h, w), 0.5, np.float32)
    junk_img = kc.SlotImage.from_planes([half, half, half, half])
    for gname, guard in GUARDS:
        for kind, wi, image, _ in consumer_sources(kc, orc, torch, w, h, guard):
            what = "%dx%d %s guard %s" % (w, h, kind, gname)
            for srgb in (False, True):
                scrub_staging(kc, junk_img)
                got, seen, launches = counted(kc, U8, {}, lambda: wi.image.to_u8(srgb))
                assert launches == 1 and seen == {}, "to_u8 %s: %d launches, counters %s" % (what, launches, seen)
                assert np.array_equal(got, orc.to_u8(image, srgb)), "to_u8 srgb=%s %s" % (srgb, what)
            assert_planes(wi.image.planes(), image.planes, what="to_f32 " + what)
            for c, hnd in enumerate(wi.image.plane_handles()):
                out = np.full((h, w + 5), -7.25, np.float32)
                assert L.kc_plane_download_f32(hnd, out.ctypes.data, (w + 5) * 4) == 0
                L.kc_plane_release(hnd)
                assert_planes([out[:, :w]], [image.planes[c]], what="plane download %d %s" % (c, what))
                assert (out[:, w:] == np.float32(-7.25)).all(), what
            wi.assert_untouched()
            note(["to_u8", "to_f32", "plane_download"], kind)


def export_geometry(e, layout, channels, w, h, aligned):
    """(offset, shape, strides, elements) of the destination inside a flat buffer, in elements: rows of an allocation 16
    pixels wider than the image (every pitch a multiple of 16 bytes), from its start or one pixel (chw: one element) in"""
    aw = (w + 31) // 16 * 16
    if layout == "hwc":
        shape, strides, offset = (h, w, channels), (aw * channels, channels, 1), 0 if aligned else channels
    else:
        shape, strides, offset = (channels, h, w), ((h + 1) * aw, aw, 1), 0 if aligned else 1
    return offset, shape, strides, offset + sum((n - 1) * s for n, s in zip(shape, strides)) + 1 + 19


@pytest.mark.parametrize("name", ["uint8", "float16"])
@pytest.mark.parametrize("size", CONSUMER_SIZES, ids=lambda s: "%dx%d" % s)
def test_device_export_of_wrapped_planes(kc, orc, torch, size, name):
    """kc_image_to_device onto an aligned (whole-quad stores) and a misaligned destination (scalar stores): only the described
    elements of the destination change, and they are the conversion of the pixels."""
    w, h = size
    e = 1 if name == "uint8" else 2
    bits = np.uint8 if e == 1 else np.uint16
    for gname, guard in GUARDS:
        for kind, wi, image, _ in consumer_sources(kc, orc, torch, w, h, guard):
            planes = rgba_view(image)
            for layout in ("hwc", "chw"):
                full = export_bits(orc, torch, name, planes, False)
                want = full if layout == "hwc" else full.transpose(2, 0, 1)
                for aligned in (True, False):
                    offset, shape, strides, n = export_geometry(e, layout, 4, w, h, aligned)
                    expect_flat = np.full(n, 0x47, np.uint8).repeat(e).view(bits).copy()
                    dev = bits_to_torch(torch, name, expect_flat.copy()).cuda()
                    np.lib.stride_tricks.as_strided(expect_flat[offset:], shape, tuple(s * e for s in strides))[...] = want
                    dview = torch.as_strided(dev, shape, strides, offset)
                    _, seen, launches = counted(kc, EXPORT, {}, lambda: wi.image.to_torch(layout=layout, out=dview))
                    what = "export %s %s %dx%d %s %s guard %s" % (name, layout, w, h, kind, "aligned" if aligned else "misaligned", gname)
                    form = "image_export_vec" if aligned else "image_export_scalar"
                    assert launches == 1 and seen == ones([form]), "%s: %d launches, counters %s" % (what, launches, seen)
                    got = torch_to_bits(torch, name, dev)
                    gn, wn = is_nan_bits(name, got), is_nan_bits(name, expect_flat)
                    assert np.array_equal(gn, wn) and np.array_equal(got[~gn], expect_flat[~wn]), what
                    note(seen, kind)
            wi.assert_untouched()


@pytest.mark.parametrize("row", ["stats", "mips", "bc_mips", "bc", "bc7", "bc6h"])
@pytest.mark.parametrize("size", CONSUMER_SIZES, ids=lambda s: "%dx%d" % s)
def test_consumer_rows_on_wrapped_planes(kc, orc, torch, size, row):
    """test_gpu_fuzz_consumers' rows (their numpy references, launch and byte counts): channel_stats in its three modes, mips()
    as a pyramid and per level, a BC mip chain, to_bc in BC1, BC3, BC4, BC5 (linear and sRGB), BC7 and BC6H."""
    w, h = size
    for gname, guard in GUARDS:
        for kind, wi, image, keys in consumer_sources(kc, orc, torch, w, h, guard):
            src = dict(image=image, keys=keys, img=lambda: wi.image)
            _consume(kc, orc, torch, row, lambda: src, np.random.default_rng([w, len(row), len(kind)]), "%s %dx%d %s guard %s" % (row, w, h, kind, gname))
            wi.assert_untouched()
            note([row], kind)


@pytest.mark.parametrize("size", CONSUMER_SIZES, ids=lambda s: "%dx%d" % s)
def test_bc_error_and_compare_on_wrapped_planes(kc, orc, torch, size):
    """kc_image_bc_error of the library's own blocks in every format, kc_image_bc_compare against another encoder's blocks
    without KC_BC_ALL_MODES (the single-subset decoder, bc_decode_ref) and with it (every mode, bc_modes_ref)."""
    w, h = size
    for gname, guard in GUARDS:
        for kind, wi, image, _ in consumer_sources(kc, orc, torch, w, h, guard):
            what = "%dx%d %s guard %s" % (w, h, kind, gname)
            for fmt, srgb in ALL_FORMS:
                if fmt == BC6H:
                    own = bc6h_ref.compare(image.planes, bc6h_ref.encode(image.planes))
                else:
                    own = bc_decode_ref.error_record(orc.to_u8(image, srgb), _ref_blocks(orc, image, fmt, srgb), fmt)
                _same(_flat_record(wi.image.bc_error(fmt, srgb)), _want_record(own, BC_SRGB if srgb else 0), "bc_error BC%d srgb=%s %s" % (fmt, srgb, what))
                if fmt != BC6H:
                    blk = bc_decode_ref.random_image_blocks(fmt, h, w, seed=3)
                    want = bc_decode_ref.error_record(orc.to_u8(image, srgb), blk, fmt)
                    got = wi.image.bc_error(fmt, srgb, blocks=torch.from_numpy(blk).cuda())
                    _same(_flat_record(got), _want_record(want, BC_SRGB if srgb else 0), "bc_compare BC%d srgb=%s %s" % (fmt, srgb, what))
            for fmt, srgb in ((BC7, False), (BC7, True), (BC6H, False)):
                blk = bc_modes_ref.random_image_blocks(fmt, h, w, seed=5)
                want = bc_modes_ref.error_record(orc.to_u8(image, srgb) if fmt == BC7 else image.planes, blk, fmt)
                got = wi.image.bc_error(fmt, srgb, blocks=torch.from_numpy(blk).cuda(), all_modes=True)
                _same(_flat_record(got), _want_record(want, BC_ALL_MODES | (BC_SRGB if srgb else 0)), "bc_compare all modes BC%d srgb=%s %s" % (fmt, srgb, what))
            wi.assert_untouched()
            note(["bc_error"], kind)


@pytest.mark.parametrize("size", CONSUMER_SIZES, ids=lambda s: "%dx%d" % s)
def test_u8_pipe_download_of_wrapped_planes(kc, orc, torch, size):
    w, h = size
    for gname, guard in GUARDS:
        p = consumer_planes(w, h)
        wi = wrapped_image(kc, torch, p, MIXED, guard)
        pipe = kc.U8Pipe(w, h, 4, depth=1)
        try:
            for srgb in (False, True):
                pipe.out_buffer(0)[...] = 0x47
                _, seen, launches = counted(kc, U8, {}, lambda: pipe.download(0, wi.image, srgb=srgb))
                got = pipe.wait_download(0).copy()
                assert launches == 1 and seen == {}, "pipe download guard %s: %d launches, counters %s" % (gname, launches, seen)
                assert np.array_equal(got, orc.to_u8(orc.Image(list(p)), srgb)), "pipe download %dx%d srgb=%s guard %s" % (w, h, srgb, gname)
        finally:
            pipe.close()
        wi.assert_untouched()
        note(["u8_pipe"], "mixed")


# ------------------------------------------------------------------ coverage, and the options are as they were
def test_every_form_ran_on_a_wrapped_source(kc):
    """Runs after the other tests of this module: every resize form (and every form a row band's resample takes), the compiled
    chain in flat, non-flat and "_q2" form, the one-step kernel, every HeightToNormal mapping and both export forms were seen
    with a source in a layout other than "pool"."""
    ran = {n for n, layout in SEEN if layout != "pool"}
    if not ran:
        pytest.skip("only meaningful after the other tests of this module")
    print("forms seen on wrapped sources:", {n: sorted(l for m, l in SEEN if m == n) for n in sorted(ran)})
    need = ["upsample_launches", "upsample_chain_launches", "resize_chain_launches", "poly2_launches", "down2_launches", "down2_by_rows",
            "resize_poly_launches", "resize_down_launches", "resize_lds_launches", "resize_wide_launches", "resize_two_pass_launches",
            "upsample_half_quads", "specialized_nt_000", "specialized_nt_101", "specialized_nt_101_q2", "flat", "nonflat", "join_launches",
            "wide", "chain1_nt0", "chain1_launches", "h2n_plain", "h2n_tiled_q5", "h2n_tiled_q6", "h2n_tiled_q7", "h2n_band",
            "image_export_vec", "image_export_scalar"]
    missing = [n for n in need if n not in ran]
    assert not missing, missing
    bands = {"band:" + c[-1] for c in BAND_CASES}
    assert bands <= ran, sorted(bands - ran)
    assert {n: kc.get_option(n) for n in OPTIONS} == _SAVED
