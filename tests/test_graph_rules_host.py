"""The graph rules every walk shares (csrc/graph.cpp: edges_by_input_slot, policy_slot_index, ancestors_topological), seen
from the host (no GPU): the size the row-band planner infers for a node under every resize policy is the size of the result
the oracle's literal process_node computes, on graphs whose edge insertion order differs from their slot order; and a cycle
among a node's ancestors is reported by the band walk as it is by the planner."""
import numpy as np
import pytest

import kanter_core_amd as kc
from golden_graphs import G
from test_bands_host import live_graph_with_sizes
from test_multi_gpu_gloo import host_live_graph

# (width, height) of Embed 0..3: no two policies that look at different things agree on them
SIZES = {0: (24, 16), 1: (12, 20), 2: (7, 9), 3: (16, 5)}
SPECIFIC_SIZE = {"SpecificSize": {"width": 10, "height": 6}}


def six_policies(slot):
    return ["MostPixels", "LeastPixels", "LargestAxes", "SmallestAxes", {"SpecificSlot": slot}, SPECIFIC_SIZE]


def mix_right_first(policy, filt="Triangle"):
    """Mix whose right input (Embed 1) was connected before its left one (Embed 0): insertion order [slot 1, slot 0]."""
    g = G()
    e0, e1 = g.add({"Embed": 0}), g.add({"Embed": 1})
    mix = g.add({"Mix": "Add"}, policy=policy, filt=filt)
    g.connect(e1, mix, 0, 1)
    g.connect(e0, mix, 0, 0)
    return g.dict(), mix


def combine_3_0_2(policy, filt="Triangle"):
    """CombineRgba with slot 3 <- Embed 0's R, slot 0 <- Embed 3's G, slot 2 <- Embed 1's B, connected in that order."""
    g = G()
    seps = []
    for eid in (0, 3, 1):
        e = g.add({"Embed": eid})
        s = g.add("SeparateRgba")
        g.connect(e, s, 0, 0)
        seps.append(s)
    comb = g.add("CombineRgba", policy=policy, filt=filt)
    g.connect(seps[0], comb, 0, 3)
    g.connect(seps[1], comb, 1, 0)
    g.connect(seps[2], comb, 2, 2)
    return g.dict(), comb


def single_input(policy, filt="Triangle"):
    g = G()
    e = g.add({"Embed": 2})
    out = g.add({"OutputRgba": "out"}, policy=policy, filt=filt)
    g.connect(e, out, 0, 0)
    return g.dict(), out


# (id, builder, policy): every graph under the six policies; the Mix also with the named slot unconnected (falls back to the
# lowest connected slot, which is NOT the first connected one)
POLICY_CASES = []
for _name, _build, _slot, _more in (("mix", mix_right_first, 1, [{"SpecificSlot": 0}, {"SpecificSlot": 5}]),
                                    ("combine", combine_3_0_2, 2, [{"SpecificSlot": 1}]),
                                    ("single", single_input, 0, [{"SpecificSlot": 3}])):
    for _p in six_policies(_slot) + _more:
        _pid = _p if isinstance(_p, str) else next(iter(_p)) + (str(_p["SpecificSlot"]) if "SpecificSlot" in _p else "")
        POLICY_CASES.append(pytest.param(_build, _p, id="%s-%s" % (_name, _pid)))


def oracle_size(graph, root):
    from oracle import oracle as orc
    emb = {i: orc.Image([np.full((h, w), 0.5, np.float32) for _ in range(4)]) for i, (w, h) in SIZES.items()}
    return orc.RefGraph(graph, embedded=emb).slot_data(root, 0).image.size


def planned_size(graph, root):
    lg, keep = live_graph_with_sizes(graph, SIZES)
    plan = lg.partition(root, 2, kc.PartitionPolicy.Bands)
    assert plan.kind == kc.PlanKind.Bands and plan.bands[0][0] == 0 and plan.bands[-1][1] == plan.full_size[1]
    return plan.full_size


@pytest.mark.parametrize("build,policy", POLICY_CASES)
def test_planned_size_is_the_oracles_under_every_policy(build, policy):
    graph, root = build(policy)
    assert planned_size(graph, root) == oracle_size(graph, root)


def test_the_policies_tell_the_inputs_apart():
    """The sizes are chosen so that a wrong input order shows: on the three-input graph the six policies give at least four
    different sizes (they give six), SpecificSlot(2) is neither the first connected nor the first sorted input, and on the Mix the fallback of
    an unconnected slot (the lowest connected slot) is not the first connected input."""
    sizes = [oracle_size(*combine_3_0_2(p)) for p in six_policies(2)]
    assert len(set(sizes)) >= 4
    assert sizes[4] == SIZES[1] and sizes[5] == (10, 6)
    assert oracle_size(*mix_right_first({"SpecificSlot": 1})) == SIZES[1]
    assert oracle_size(*mix_right_first({"SpecificSlot": 5})) == SIZES[0]


def test_band_walk_reports_a_cycle_among_the_ancestors():
    g = G()
    a, b, c = g.add({"Mix": "Add"}), g.add({"Mix": "Add"}), g.add({"Mix": "Add"})
    g.connect(a, b, 0, 0)
    g.connect(b, a, 0, 0)
    g.connect(b, c, 0, 0)
    lg = host_live_graph(g.dict())
    with pytest.raises(kc.TexProError, match="graph has a cycle through node"):
        lg.band_source_rows(c, 0, 1)
