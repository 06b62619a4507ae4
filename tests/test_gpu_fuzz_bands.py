"""GPU parity, differential: row bands (csrc/bands.cpp -- kc_live_graph_evaluate_band, kc_live_graph_band_source_rows,
kc_live_graph_embed_slot_data_band) of random graphs against the rows of the oracle's whole image, bit for bit.

The band walk is a second walk of the graph with its own size and type inference, its own need propagation (toroidal halo
for HeightToNormal, tap windows for every implicit resize), its own flattening of Graph nodes and vertical tap tables rebuilt
per band.  The graphs, the targets and the band sets come from tests/band_fuzz.py: the random graphs of test_gpu_fuzz_graphs on
a size list without tiny images, the nodes of 16 rows or more whose plan has a halo, a partly read resized source or a wrap,
and a second generator with Graph nodes.  The host side of the same fuzz is tests/test_band_plan_fuzz_host.py."""
import gc

import numpy as np
import pytest

import band_fuzz as bf
from test_gpu_bands import band_splits, build, mix_band_graph
from test_gpu_resize_variants import COUNTERS
from test_gpu_wrapped_planes import RESIZE_CASES
from util import SEED_A, SEED_B, assert_planes, edge_lines, resize_source, salt

pytestmark = pytest.mark.gpu

SEED_BANDS, SEED_SHARDS = 0xF0AD0000, 0xF0AE0000


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    return kc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


def check_band(kc, lg, node, sd, y0, y1, what):
    got = lg.evaluate_band(node, y0, y1, slot_id=int(sd.slot_id))
    assert got.is_rgba() == sd.image.is_rgba, what
    planes = got.planes()
    assert planes[0].shape[0] == y1 - y0, "%s: %d rows" % (what, planes[0].shape[0])
    assert_planes(planes, [p[y0:y1] for p in sd.image.planes], what=what)


def check_whole(kc, lg, node, want, what):
    got = sorted(lg.await_clean(node).node_slot_datas(node), key=lambda s: s.slot_id)
    assert [int(g.slot_id) for g in got] == [int(w.slot_id) for w in want], what
    for g, w in zip(got, want):
        assert g.image.is_rgba() == w.image.is_rgba, what
        assert_planes(g.image.planes(), w.image.planes, what="%s slot %d" % (what, int(g.slot_id)))


def check_target_bands(kc, case, node, seed, use_cache=False):
    """Every slot of the node, every band set: each band on a fresh live graph; then all bands one after the other on one live
    graph, after which the whole-image evaluation of the node on that graph is still the oracle's."""
    want = case.want(node)
    rng = np.random.default_rng([seed, node])
    same = case.live_graph(kc)
    same.use_cache = use_cache
    for sd in want:
        h = sd.image.size[1]
        for name, bands in bf.band_sets(h, rng):
            for y0, y1 in bands:
                what = "seed %d node %d slot %d, %s, band %d..%d" % (seed, node, int(sd.slot_id), name, y0, y1)
                fresh = case.live_graph(kc)
                fresh.use_cache = use_cache
                check_band(kc, fresh, node, sd, y0, y1, what + ", fresh graph")
                check_band(kc, same, node, sd, y0, y1, what + ", same graph")
    check_whole(kc, same, node, want, "seed %d node %d, whole image after the bands" % (seed, node))


def check_refused(kc, case, node, seed):
    """A node the oracle refuses: every band of every slot it might have raises."""
    lg = case.live_graph(kc)
    graph = next((n for n in case.graph["nodes"] if n["node_id"] == node and node in case.graph_nodes), None)
    slots = [n["node_id"] for n in graph["node_type"]["Graph"]["nodes"] if case.orc._node_kind(n)[0].startswith("Output")] if graph else [0]
    for slot in slots:
        for y0, y1 in ((0, 1), (0, 5), (3, 9), (15, 16)):
            with pytest.raises(kc.TexProError):
                lg.evaluate_band(node, y0, y1, slot_id=slot)
                pytest.fail("seed %d node %d slot %d band %d..%d: the oracle refuses the node, the band walk does not" % (seed, node, slot, y0, y1))


# ---- (a) bands equal the oracle's rows ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(120))
def test_bands_of_random_graphs_equal_the_oracles_rows(kc, orc, seed):
    case = bf.random_case(orc, SEED_BANDS + seed)
    for node, _, _ in bf.case_targets(case):
        check_target_bands(kc, case, node, seed, use_cache=bool(seed & 1))
    refused = [n for n in case.nodes if case.want(n) is None]
    for node in refused[-1:]:  # the deepest one: most of the graph above it
        check_refused(kc, case, node, seed)


# ---- (b) sharded sources with exactly the planned halo ---------------------------------------------------------
@pytest.mark.parametrize("seed", range(60))
def test_sharded_sources_with_exactly_the_planned_rows(kc, orc, seed):
    """Per band, every Embed holds only the rows band_source_rows names (wrapped rows first; a source the plan omits is not
    embedded at all): the band is the oracle's.  With one source one row short at either end the call is refused -- it never
    returns other pixels."""
    case = bf.random_case(orc, SEED_SHARDS + seed)
    rng = np.random.default_rng([seed, 1])
    planner = case.live_graph(bf.host_kc())
    for node, h, _ in bf.case_targets(case):
        want = case.want(node)
        for y0, y1 in bf.fixed_bands(h):
            plan = planner.band_source_rows(node, y0, y1)
            rows = {case.embed_nodes[n]: (a, b) for n, (a, b, _, _) in plan.items()}
            images = {eid: case.embedded[eid] for eid in rows}
            for sd in want:
                lg = case.live_graph(kc, bands=rows, images=images)
                check_band(kc, lg, node, sd, y0, y1, "seed %d node %d slot %d band %d..%d, sources %s" % (seed, node, int(sd.slot_id), y0, y1, rows))
            cut = [eid for eid, (a, b) in rows.items() if b - a >= 2]
            if not cut:
                continue
            eid = cut[rng.integers(len(cut))]
            a, b = rows[eid]
            for short in ((a + 1, b), (a, b - 1)):
                lg = case.live_graph(kc, bands={**rows, eid: short}, images=images)
                with pytest.raises(kc.TexProError):
                    lg.evaluate_band(node, y0, y1, slot_id=int(want[0].slot_id))
                    pytest.fail("seed %d node %d band %d..%d: source %d holds rows %s of the planned %s and the band is not refused" % (
                        seed, node, y0, y1, eid, short, (a, b)))


# ---- (c) Graph nodes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(bf.N_GRAPH_NODES))
def test_graphs_with_graph_nodes_whole_and_in_bands(kc, orc, seed):
    """The whole-image evaluation (csrc/graph.cpp) of every node at or below a Graph node equals the oracle, refusals
    included; bands of the chosen targets below a Graph node and of every output slot of every Graph node equal its rows."""
    case = bf.graph_node_case(orc, bf.SEED_GRAPH_NODES + seed)
    below = bf.below_graph_nodes(case)
    for node in below:
        want = case.want(node)
        lg = case.live_graph(kc)
        if want is None:
            with pytest.raises(kc.TexProError):
                lg.await_clean(node)
            continue
        check_whole(kc, lg, node, want, "seed %d node %d, whole image" % (seed, node))
    targets = [n for n, _, _ in bf.case_targets(case, nodes=below)]
    targets += [n for n in case.graph_nodes if n not in targets and case.want(n) is not None]
    for node in targets:
        check_target_bands(kc, case, node, seed, use_cache=bool(seed & 1))
    for node in [n for n in below if case.want(n) is None][-1:]:
        check_refused(kc, case, node, seed)


@pytest.mark.parametrize("generator,seed", [("graph_nodes", 6), ("graph_nodes", 53)])
def test_soak_band_seeds_that_found_defects(kc, orc, generator, seed):
    """Seeds of this module's fuzz that found defects.  Graph-node graph 6: a nested Graph node with an InputGray nothing is
    connected to and nothing reads; the reference never processes such a node (graph::process asks for the Output nodes only),
    the band walk's expansion refused the whole graph for it.  Graph-node graph 53: a child graph with two Output nodes, one
    of them behind a node that fails; the reference fails the Graph node whichever output is asked for, the band walk looked
    at the ancestors of the requested Output only and returned its band."""
    {"random": test_bands_of_random_graphs_equal_the_oracles_rows, "graph_nodes": test_graphs_with_graph_nodes_whole_and_in_bands}[generator](kc, orc, seed)


# ---- (d) every resize form inside a band ----------------------------------------------------------------------
# What the counters of test_gpu_resize_variants.COUNTERS read over all bands of band_splits, per (case of
# test_gpu_wrapped_planes.RESIZE_CASES, HeightToNormal behind the Mix): the form of a band's resample is the launcher's decision
# on the BAND's table (fewer output rows, a source band instead of the source), not the whole image's.  As observed on the
# MI355X: a band never goes through resize_poly_kernel, resize_poly2_kernel or the integer-ratio up-sampling kernels -- the
# shapes that take them whole go to resize_down2_kernel, resize_down_kernel and resize_lds_kernel band by band -- and the band
# of a HeightToNormal consumer that wraps (rows of both ends in one table) leaves down2 for resize_down / resize_lds.
BAND_FORM_COUNTERS = {
    ('down2_catmull_rows0', False): {'down2_launches': 16, 'down2_xcd_order': 1},
    ('down2_catmull_rows0', True): {'down2_launches': 15, 'resize_down_launches': 1, 'down2_xcd_order': 1},
    ('down2_catmull_rows1', False): {'down2_launches': 16, 'down2_xcd_order': 1},
    ('down2_catmull_rows1', True): {'down2_launches': 15, 'resize_down_launches': 1, 'down2_xcd_order': 1},
    ('down2_lanczos_rows0', False): {'down2_launches': 20, 'down2_xcd_order': 1},
    ('down2_lanczos_rows0', True): {'down2_launches': 19, 'resize_down_launches': 1, 'down2_xcd_order': 1},
    ('down2_lanczos_rows1', False): {'down2_launches': 20, 'down2_by_rows': 20},
    ('down2_lanczos_rows1', True): {'down2_launches': 19, 'resize_down_launches': 1, 'down2_by_rows': 19},
    ('down2_triangle_rows0', False): {'down2_launches': 16, 'down2_xcd_order': 1},
    ('down2_triangle_rows0', True): {'down2_launches': 15, 'resize_lds_launches': 1, 'down2_xcd_order': 1},
    ('down2_triangle_rows1', False): {'down2_launches': 16, 'down2_by_rows': 16},
    ('down2_triangle_rows1', True): {'down2_launches': 15, 'resize_lds_launches': 1, 'down2_by_rows': 15},
    ('poly2_odd_strips', False): {'resize_down_launches': 16},
    ('poly2_odd_strips', True): {'resize_down_launches': 16},
    ('poly2_ratio2', False): {'down2_launches': 19, 'down2_by_rows': 9},
    ('poly2_ratio2', True): {'down2_launches': 18, 'resize_down_launches': 1, 'down2_by_rows': 8},
    ('poly', False): {'down2_launches': 15, 'down2_by_rows': 13},
    ('poly', True): {'down2_launches': 14, 'resize_down_launches': 1, 'down2_by_rows': 14},
    ('down_ratio4', False): {'resize_down_launches': 15},
    ('down_ratio4', True): {'resize_down_launches': 15},
    ('down', False): {'resize_down_launches': 18},
    ('down', True): {'resize_down_launches': 18},
    ('lds_lanczos', False): {'resize_lds_launches': 19},
    ('lds_lanczos', True): {'resize_lds_launches': 19},
    ('lds_gaussian', False): {'resize_lds_launches': 20},
    ('lds_gaussian', True): {'resize_lds_launches': 20},
    ('wide', False): {'resize_wide_launches': 20},
    ('wide', True): {'resize_wide_launches': 20},
    ('two_pass', False): {'resize_two_pass_launches': 80},
    ('two_pass', True): {'resize_two_pass_launches': 80},
    ('upsample_triangle_x8', False): {'resize_lds_launches': 20},
    ('upsample_triangle_x8', True): {'resize_lds_launches': 20},
    ('upsample_lanczos_x4', False): {'resize_lds_launches': 15},
    ('upsample_lanczos_x4', True): {'resize_lds_launches': 15},
    ('upsample_half_quads', False): {'resize_lds_launches': 18},
    ('upsample_half_quads', True): {'resize_lds_launches': 18},
}


@pytest.mark.parametrize("h2n", [False, True], ids=["mix", "height_to_normal"])
@pytest.mark.parametrize("case", RESIZE_CASES, ids=[c[0] for c in RESIZE_CASES])
def test_every_resize_form_in_bands_equals_oracle_crops(kc, orc, case, h2n):
    """Embed A -> Mix(Add) <- Embed B with A resampled to B's size [-> SeparateRgba -> HeightToNormal], at the shapes and under
    the options at which the whole-image resample takes each form: every band of band_splits equals the crop of the oracle."""
    name, filt, (aw, ah), (bw, bh), opts, _, _ = case
    splits = band_splits(bh)
    rows = edge_lines(ah, [4, 16]) + [min(ah - 1, y * ah // bh) for band in splits for y in (band[0], band[1] - 1)]
    cols = edge_lines(aw, [4, 64])
    a = [salt(resize_source(SEED_A, c, ah, aw), rows[c::3] if h2n else rows[c::2], cols[c % 2::2], shift=c) for c in range(4)]
    b = [resize_source(SEED_B, c, bh, bw) for c in range(4)]
    if h2n:  # NaN and inf would reach every normal of their neighbourhood through the normalisation: keep them to one plane
        a[0] = resize_source(SEED_A, 0, ah, aw)
    mixed = [orc.mix_plane("Add", orc.resize_plane(a[c], bw, bh, filt), b[c]) for c in range(3)] + [np.ones((bh, bw), np.float32)]
    want = list(orc.height_to_normal(mixed[0])) + [np.ones((bh, bw), np.float32)] if h2n else mixed
    graph, root = mix_band_graph((aw, ah), (bw, bh), filt, h2n)
    # (mix_band_graph picks the policy by pixel count; "wide" has as many pixels in A as in B: name B's slot)
    graph["nodes"][2]["resize_policy"] = {"SpecificSlot": 1}
    saved = {k: kc.get_option(k) for k in opts}
    before = {n: kc.stats_counter(n) for n in COUNTERS}
    try:
        for k, v in opts.items():
            kc.set_option(k, v)
        _, lg = build(kc, graph, {0: a, 1: b})
        for (y0, y1) in splits:
            got = lg.evaluate_band(root, y0, y1).planes()
            assert_planes(got, [p[y0:y1] for p in want], what="%s %s band %d..%d" % (name, "h2n" if h2n else "mix", y0, y1))
    finally:
        for k, v in saved.items():
            kc.set_option(k, v)
    seen = {n: kc.stats_counter(n) - before[n] for n in COUNTERS if kc.stats_counter(n) != before[n]}
    print("BAND_FORM_COUNTERS %r: %r," % ((name, h2n), seen))
    pinned = BAND_FORM_COUNTERS[(name, h2n)]
    assert seen == pinned, "%s %s: counters %s, pinned %s" % (name, "h2n" if h2n else "mix", seen, pinned)


# ---- (e) the band-table LRU -----------------------------------------------------------------------------------
def test_more_band_tables_than_the_lru_holds(kc, orc):
    """1-row bands down a 100-row up-sample of a 37-row source, two filters: 200 distinct (in, out, filter, a, b, src_y0)
    tables through the 64-entry LRU of get_band_taps (csrc/resize.cpp), then the first ones again; every band is right, and
    when the images are gone so are the bytes."""
    kc.sync()
    gc.collect()
    in_use = kc.stats()["bytes_in_use"]
    (aw, ah), (bw, bh) = (29, 37), (77, 100)
    a = [resize_source(SEED_A, c, ah, aw) for c in range(4)]
    b = [resize_source(SEED_B, c, bh, bw) for c in range(4)]
    for filt in ("Lanczos3", "CatmullRom"):
        want = [orc.mix_plane("Add", orc.resize_plane(a[c], bw, bh, filt), b[c]) for c in range(3)] + [np.ones((bh, bw), np.float32)]
        graph, root = mix_band_graph((aw, ah), (bw, bh), filt, False)
        _, lg = build(kc, graph, {0: a, 1: b})
        for y in list(range(bh)) + [0, 1, 2, bh - 1]:
            got = lg.evaluate_band(root, y, y + 1).planes()
            assert_planes(got, [p[y:y + 1] for p in want], what="%s row %d" % (filt, y))
        del lg, got
    gc.collect()
    kc.sync()
    assert kc.stats()["bytes_in_use"] == in_use


# ---- (f) one-row results --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_any_band_of_a_one_row_result_is_the_row(kc, orc, seed):
    """A target of height 1 has nothing to cut: whatever (y0, y1) says, the band is the 1-row image (propagate_needs)."""
    case = bf.random_case(orc, SEED_BANDS + 0x1000 + seed)
    done = 0
    for node in reversed(case.nodes):
        want = case.want(node)
        if want is None or want[0].image.size[1] != 1:
            continue
        for sd in want:
            for y0, y1 in ((0, 1), (0, 7), (5, 6), (3, 2), (40, 41)):
                lg = case.live_graph(kc)
                got = lg.evaluate_band(node, y0, y1, slot_id=int(sd.slot_id))
                assert got.is_rgba() == sd.image.is_rgba
                assert_planes(got.planes(), sd.image.planes, what="seed %d node %d slot %d band %d..%d" % (seed, node, int(sd.slot_id), y0, y1))
        done += 1
        if done == 2:
            break
