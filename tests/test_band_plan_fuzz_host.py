"""The row-band PLANNER under random graphs, on the host (no GPU): kc_live_graph_band_source_rows against the oracle.

Soundness: a plan names, per source image, the rows a band of the result reads.  Every source row the plan does NOT name is
overwritten with noise and the oracle evaluates the graph again: rows [y0, y1) of every slot of the target must keep their
bits.  (The check has teeth: with the plan's first or last row dropped as well, 48 % and 44 % of the plane comparisons of a
prototype changed; with the plan as it is, none of 3 076.)  A plan too small is what made the only GPU memory fault of the
band path; this looks for it without a device.

The graphs are those of tests/band_fuzz.py: the random graphs of test_gpu_fuzz_graphs on a size list without tiny images,
targets chosen by band_targets, and graphs with Graph nodes, which the planner flattens on the host.  The coverage test keeps
the choice from degenerating: its floors stand below what these seeds gave when the test was written (see its docstring)."""
import functools

import numpy as np
import pytest

import band_fuzz as bf
from util import bit_equal


@functools.lru_cache(maxsize=None)
def _orc():
    from oracle import oracle as orc
    return orc


@functools.lru_cache(maxsize=None)
def random_case(seed):
    case = bf.random_case(_orc(), bf.SEED_PLAN + seed)
    return case, bf.case_targets(case)


@functools.lru_cache(maxsize=None)
def graph_node_case(seed):
    case = bf.graph_node_case(_orc(), bf.SEED_GRAPH_NODES + seed)
    return case, bf.case_targets(case, nodes=bf.below_graph_nodes(case))


def check_plan(case, node, h, seed):
    """Shape and soundness of the plans of the fixed bands of one target; -> plane comparisons made."""
    orc = _orc()
    lg = case.live_graph(bf.host_kc())
    want = case.want(node)
    if node in case.graph_nodes:
        # a Graph node is planned by its first Output node (csrc/bands.cpp, band_source_rows): that slot's rows only
        first = next(n["node_id"] for n in case.graph["nodes"][node]["node_type"]["Graph"]["nodes"]
                     if orc._node_kind(n)[0] in ("OutputGray", "OutputRgba"))
        want = [s for s in want if s.slot_id == first]
        h = want[0].image.size[1]
    rng = np.random.default_rng([seed, node])
    compared = 0
    for y0, y1 in bf.fixed_bands(h):
        plan = lg.band_source_rows(node, y0, y1)  # a refusal (TexProError) of a target the oracle accepts fails the test
        noised = {}
        for n, (a, b, w, sh) in plan.items():
            assert n in case.embed_nodes, "seed %d node %d: the plan names node %d, which is no Embed" % (seed, node, n)
            img = case.embedded[case.embed_nodes[n]]
            assert (w, sh) == img.size, "seed %d node %d band %d..%d: source %d is %s, the plan says %s" % (seed, node, y0, y1, n, img.size, (w, sh))
            assert -sh <= a < b <= sh, "seed %d node %d band %d..%d: rows %d..%d of a %d-row source" % (seed, node, y0, y1, a, b, sh)
        rows_of = {}
        for n, (a, b, _, sh) in plan.items():  # (two Embed nodes of one image: the union, which is what a host would load)
            eid = case.embed_nodes[n]
            rows_of.setdefault(eid, set()).update(r % sh for r in range(a, b))
        for eid, img in case.embedded.items():
            keep = rows_of.get(eid)  # None: the plan omits the source, replaced whole
            planes = []
            for p in img.planes:
                q = (rng.random(p.shape, dtype=np.float32) * np.float32(4.0) - np.float32(2.0)).astype(np.float32)
                if keep:
                    q[sorted(keep)] = p[sorted(keep)]
                planes.append(q)
            noised[eid] = orc.Image(planes)
        again = sorted(orc.RefGraph(case.graph, embedded=noised).node_slot_datas(node), key=lambda s: s.slot_id)
        again = [s for s in again if s.slot_id in {w_.slot_id for w_ in want}]
        assert len(again) == len(want)
        for g, w_ in zip(again, want):
            assert g.image.size == w_.image.size
            one_row = w_.image.size[1] == 1  # (a slot of another height than the first: 1 x 1, the only other height a node has)
            for c, (pg, pw) in enumerate(zip(g.image.planes, w_.image.planes)):
                compared += 1
                assert bit_equal(pg if one_row else pg[y0:y1], pw if one_row else pw[y0:y1]), (
                    "seed %d node %d slot %d plane %d: rows %d..%d change with the rows outside the plan %s" % (seed, node, g.slot_id, c, y0, y1, plan))
    return compared


@pytest.mark.parametrize("seed", range(bf.N_PLAN))
def test_plans_of_random_graphs_are_sound(seed):
    case, targets = random_case(seed)
    for node, h, _ in targets:
        check_plan(case, node, h, seed)


@pytest.mark.parametrize("seed", range(bf.N_GRAPH_NODES))
def test_plans_through_graph_nodes_are_sound(seed):
    case, targets = graph_node_case(seed)
    assert 1 <= len(case.graph_nodes) <= 3
    for node, h, _ in targets:
        check_plan(case, node, h, seed)


def shares(all_targets):
    flat = [t for ts in all_targets for t in ts]
    n = max(len(flat), 1)
    return (sum(bool(ts) for ts in all_targets) / len(all_targets), sum("halo" in f for _, _, f in flat) / n,
            sum("part" in f for _, _, f in flat) / n, sum("wrap" in f for _, _, f in flat) / n, len(flat))


def test_the_fuzz_reaches_the_band_code():
    """Coverage of the chosen targets over the seed range.  Measured when written: 148 of 150 seeds yield a target; of 292
    targets 45 % need a halo row of a same-height source, 64 % read a strict part of a source of another height (a resize on
    the way), 16 % wrap (row -1 of a source).  The floors stand below that: 90 % of seeds, 25 %, 50 % and 10 % of targets.
    Graph-node graphs: see test_graph_node_graphs_reach_the_band_code."""
    with_target, halo, part, wrap, n = shares([random_case(s)[1] for s in range(bf.N_PLAN)])
    print("random graphs: %.1f %% of seeds with a target, %d targets: halo %.0f %%, part %.0f %%, wrap %.0f %%" % (
        100 * with_target, n, 100 * halo, 100 * part, 100 * wrap))
    assert with_target >= 0.90 and halo >= 0.25 and part >= 0.50 and wrap >= 0.10, (with_target, halo, part, wrap)


def test_graph_node_graphs_reach_the_band_code():
    """The generator's promises and its reach: one to three Graph nodes per graph, nesting up to depth 2, a child with two
    Output nodes and a HeightToNormal inside in every graph; most seeds offer a target at or below a Graph node.  Measured
    when written: 54 of 60 seeds, 94 targets, 23 % with a halo, 62 % with a partly read resized source, 14 % with a wrap; 68
    nested Graph nodes."""
    orc = _orc()
    depth2 = 0

    def kinds(graph, depth):
        nonlocal depth2
        out = []
        for n in graph["nodes"]:
            k, arg = orc._node_kind(n)
            out.append(k)
            if k == "Graph":
                depth2 += depth == 1
                out += kinds(arg, depth + 1)
                assert depth < 2
        return out

    for s in range(bf.N_GRAPH_NODES):
        case, _ = graph_node_case(s)
        assert 1 <= len(case.graph_nodes) <= 3
        forced = [n for n in case.graph["nodes"] if orc._node_kind(n)[0] == "Graph"]
        assert any(orc.output_slot_count(n) == 2 and "HeightToNormal" in [orc._node_kind(c)[0] for c in n["node_type"]["Graph"]["nodes"]]
                   for n in forced), s
        kinds(case.graph, 0)
    with_target, halo, part, wrap, n = shares([graph_node_case(s)[1] for s in range(bf.N_GRAPH_NODES)])
    print("graph-node graphs: %.0f %% of seeds with a target, %d targets: halo %.0f %%, part %.0f %%, wrap %.0f %%; %d nested Graph nodes" % (
        100 * with_target, n, 100 * halo, 100 * part, 100 * wrap, depth2))
    # (non-degeneracy guards of this generator: three seeds in four with a target, and each effect in at least one target in
    # ten, the lowest floor the random graphs have)
    assert depth2 >= 5 and with_target >= 0.75 and halo >= 0.10 and part >= 0.10 and wrap >= 0.10, (depth2, with_target, halo, part, wrap)


def test_generator_size_list_leaves_the_graph_fuzz_alone():
    """sizes= defaults to the graph fuzz's own list: the same stream, the same graph as before the parameter existed."""
    import test_gpu_fuzz_graphs as fz
    kc, orc = bf.host_kc(), _orc()
    a = fz._build(kc, orc, 0xF0220000 + 7)[0].node_graph().to_json()
    b = fz._build(kc, orc, 0xF0220000 + 7, sizes=fz.SIZES)[0].node_graph().to_json()
    assert a == b
