"""What the row-band fuzz tests share (tests/test_band_plan_fuzz_host.py, tests/test_gpu_fuzz_bands.py, profiles/soak_fuzz.py):
the random graphs of tests/test_gpu_fuzz_graphs._build on a size list without tiny images, a second generator of graphs WITH
Graph nodes, the choice of the nodes worth cutting into bands, and the band sets.

Why the targets are chosen: of the nodes _build asks for (seeds 0xF0AA0000 + 0..149, its own size list) 47 % of the results the
oracle accepts are ONE row high -- Value nodes, LeastPixels / SmallestAxes and SeparateRgba of a gray image collapse most
graphs to 1 x 1 -- and there is nothing to cut in those.  band_targets therefore looks at every node of a graph, keeps those
of 16 rows or more and prefers the ones whose plan (kc_live_graph_band_source_rows) has a halo, a partly read resized source
or a wrap in it.  The planner runs on the host: a live graph of a HostOnlyTexPro with constant planes will do (host_kc)."""
import json

import numpy as np

import test_gpu_fuzz_graphs as fz
from golden_graphs import G

# (w, h); no extent above 1100.  From (130, 70) on: the shapes of test_gpu_wrapped_planes.RESIZE_CASES' small forms
BAND_SIZES = [(24, 16), (48, 32), (17, 29), (64, 24), (300, 40), (40, 300), (7, 260), (130, 70), (61, 33), (37, 29), (100, 77),
              (16, 16), (128, 128), (1, 1)]
MIN_ROWS = 16  # a target has at least this many rows
# How the oracle fails a node the reference fails: InvalidBufferCount / NodeProcessing, the panic of CombineRgba on an RGBA
# input, and the index out of bounds of an InputRgba in a Graph node nothing is connected to (src/node/input_rgba.rs:7-13)
REFUSALS = (RuntimeError, AssertionError, IndexError)

SEED_PLAN, N_PLAN = 0xF0AB0000, 150         # host: plan soundness, random graphs
SEED_GRAPH_NODES, N_GRAPH_NODES = 0xF0AC0000, 60  # host and GPU: graphs with Graph nodes


# ---------------------------------------------------------------------------------------------- a host-only kc
class _HostTextureProcessor:
    @staticmethod
    def new():
        from test_multi_gpu_gloo import HostOnlyTexPro
        return HostOnlyTexPro()


class _HostSlotImage:
    @staticmethod
    def from_planes(planes):
        """A constant image of the planes' size and count: the planner looks at sizes and types only."""
        import ctypes as C
        import kanter_core_amd as kc
        from kanter_core_amd import _lib
        L = _lib.load()
        h, w = planes[0].shape
        handles = []
        for _ in planes:
            p = C.c_void_p()
            assert L.kc_plane_const(w, h, 0.5, C.byref(p)) == 0  # constant planes need no device
            handles.append(p)
        im = C.c_void_p()
        if len(handles) == 4:
            assert L.kc_image_rgba((C.c_void_p * 4)(*[p.value for p in handles]), C.byref(im)) == 0
        else:
            assert L.kc_image_gray(handles[0], C.byref(im)) == 0
        for p in handles:
            L.kc_plane_release(p)
        return kc.SlotImage(im.value)


class HostKc:
    """kanter_core_amd as _build uses it, without a device: texture processors that never touch one and constant images."""
    TextureProcessor = _HostTextureProcessor
    SlotImage = _HostSlotImage

    def __getattr__(self, name):
        import kanter_core_amd as kc
        return getattr(kc, name)


def host_kc():
    return HostKc()


# ---------------------------------------------------------------------------------------------- cases
class Case:
    """One random graph: .graph (the JSON dict), .embedded ({embed id: orc.Image}), .ref (orc.RefGraph), .nodes (ids of the
    nodes targets are chosen from), .embed_nodes ({node id: embed id}), .graph_nodes (ids of the outer graph's Graph nodes)."""

    def __init__(self, orc, graph, embedded, nodes):
        self.orc, self.graph, self.embedded, self.nodes = orc, graph, embedded, [int(n) for n in nodes]
        self.ref = orc.RefGraph(graph, embedded=embedded)
        self.embed_nodes = {n["node_id"]: n["node_type"]["Embed"] for n in graph["nodes"]
                            if isinstance(n["node_type"], dict) and "Embed" in n["node_type"]}
        self.graph_nodes = [n["node_id"] for n in graph["nodes"] if isinstance(n["node_type"], dict) and "Graph" in n["node_type"]]

    def live_graph(self, kc, bands=None, images=None):
        """A fresh live graph of the case on `kc` (host_kc() for planning); bands: {embed id: (y0, y1)} embeds only those rows,
        the wrapped ones first; images: other pixels than the case's."""
        lg = kc.TextureProcessor.new().new_live_graph()
        lg.set_node_graph(kc.NodeGraph.from_json(json.dumps(self.graph)))
        for eid, img in (images or self.embedded).items():
            planes = img.planes
            if bands is None or eid not in bands:
                lg.embed_slot_data_with_id(kc.SlotData(0, 0, kc.SlotImage.from_planes(planes)), eid)
            else:
                y0, y1 = bands[eid]
                h = planes[0].shape[0]
                rows = [r % h for r in range(y0, y1)]
                lg.embed_slot_data_band(kc.SlotData(0, 0, kc.SlotImage.from_planes([p[rows] for p in planes])), eid, y0, h)
        return lg

    def want(self, node):
        """The oracle's slot datas of the node, sorted by slot id; None where the reference fails the node."""
        try:
            return sorted(self.ref.node_slot_datas(int(node)), key=lambda s: s.slot_id)
        except REFUSALS as e:
            assert str(e) in ("InvalidBufferCount", "NodeProcessing", "list index out of range") or "RGBA image into this slot" in str(e), e
            return None


def random_case(orc, seed):
    """The graph of fz._build(seed) on BAND_SIZES."""
    info = {}
    lg, _, _ = fz._build(host_kc(), orc, seed, info, sizes=BAND_SIZES)
    graph = json.loads(lg.node_graph().to_json())
    return Case(orc, graph, info["embedded"], [n[0] for n in info.get("nodes", [])])


# ---------------------------------------------------------------------------------------------- graphs with Graph nodes
# (weighted towards the policies that keep an image large: LeastPixels and SmallestAxes meet a 1 x 1 Value and collapse the rest)
_POLICIES = ["MostPixels", "MostPixels", "MostPixels", "LargestAxes", "LargestAxes", "LeastPixels", "SmallestAxes", "SpecificSlot",
             "SpecificSize", "SpecificSize"]


class _Builder:
    """Random nodes from the menu of fz._build (Mix without Pow, invert, SeparateRgba, CombineRgba, HeightToNormal) added to a
    G.  Every output slot is kept with its static type ("G", "R", "X": what connect() checks) and the type that flows at run
    time ("G" / "R"), so that most choices give a node the reference accepts; one in ten is made on the static type alone."""

    def __init__(self, rng):
        self.rng, self.g, self.outs, self.made = rng, G(), [], []

    def out(self, node, slot, static, runtime):
        self.outs.append((node, slot, static, runtime))

    def pick(self, static, runtime=None):
        rng = self.rng
        cands = [o for o in self.outs if static == "X" or o[2] in (static, "X")]
        if runtime is not None and rng.random() < 0.9:
            strict = [o for o in cands if o[3] == runtime]
            cands = strict or cands
        return cands[rng.integers(len(cands))] if cands else None

    def policy(self, n_inputs, slots=None):
        rng = self.rng
        k = _POLICIES[rng.integers(len(_POLICIES))]
        if k == "SpecificSlot":
            return {"SpecificSlot": int(slots[rng.integers(len(slots))]) if slots else int(rng.integers(max(n_inputs, 1)))}
        if k == "SpecificSize":
            w, h = BAND_SIZES[rng.integers(len(BAND_SIZES) - 1)]
            return {"SpecificSize": {"width": w + int(rng.integers(3)), "height": h}}
        return k

    def filt(self):
        return fz.FILTERS[self.rng.integers(len(fz.FILTERS))]

    def connect(self, ins, node, slots=None):
        order = list(range(len(ins)))
        self.rng.shuffle(order)  # edge insertion order != slot order
        for i in order:
            if ins[i] is not None:
                self.g.connect(ins[i][0], node, ins[i][1], slots[i] if slots else i)

    def menu_node(self, kind=None):
        rng, g = self.rng, self.g
        r = rng.random()
        if kind is None:
            kind = "Mix" if r < 0.55 else "SeparateRgba" if r < 0.67 else "CombineRgba" if r < 0.79 else "HeightToNormal" if r < 0.92 else "invert"
        if kind == "Mix":
            ins = [self.pick("X") if rng.random() < 0.93 else None for _ in range(2)]
            first = ins[0] or ins[1]
            n = g.add({"Mix": fz.OPS[rng.integers(len(fz.OPS))]}, self.policy(2), self.filt())
            produces = [(0, "X", first[3] if first else "G")]
        elif kind == "SeparateRgba":
            ins = [self.pick("R", "R")]
            n = g.add("SeparateRgba", self.policy(1), self.filt())
            produces = [(s, "G", "G") for s in range(4)]
        elif kind == "CombineRgba":
            ins = [self.pick("G", "G") if rng.random() < 0.8 else None for _ in range(4)]
            n = g.add("CombineRgba", self.policy(4), self.filt())
            produces = [(0, "R", "R")]
        elif kind == "HeightToNormal":
            ins = [self.pick("G", "G")]
            n = g.add("HeightToNormal", self.policy(1), self.filt())
            produces = [(0, "R", "R")]
        else:  # invert: Mix(Subtract)(Value 1, x)
            one = g.add({"Value": 1.0})
            ins = [(one, 0, "G", "G"), self.pick("X")]
            n = g.add({"Mix": "Subtract"}, self.policy(2), self.filt())
            produces = [(0, "X", "G")]
        self.connect(ins, n)
        for s, st, rt in produces:
            self.out(n, s, st, rt)
        self.made.append(n)
        return n

    def graph_node(self, depth, force=False):
        """A Graph node with its own policy and filter around child_graph(); inputs from this builder's outputs."""
        rng, g = self.rng, self.g
        child, inputs, outputs = child_graph(rng, depth, force)
        ins = []
        for _, static in inputs:
            ins.append(self.pick(static, static) if rng.random() < 0.95 else None)  # (an unconnected Input: the reference fails the node)
        slots = [i for i, _ in inputs]
        n = g.add({"Graph": child}, self.policy(len(ins), slots), self.filt())
        self.connect(ins, n, slots)
        for o, static in outputs:
            self.out(n, o, static, static if static != "X" else "G")
        self.made.append(n)
        return n


def child_graph(rng, depth, force=False):
    """-> (graph dict, [(Input node id, static type)], [(Output node id, static type)]).  One to three Input nodes, nodes from
    the menu (below depth 2 sometimes another Graph node), one or two Output nodes; force: two Outputs and a HeightToNormal."""
    b = _Builder(rng)
    inputs = []
    for i in range(int(rng.integers(1, 4))):
        rgba = bool(rng.random() < 0.3) and i > 0  # (the first one gray: HeightToNormal and CombineRgba have something to read)
        n = b.g.add({"InputRgba" if rgba else "InputGray": "in%d" % i})
        inputs.append((n, "R" if rgba else "G"))
        b.out(n, 0, "R" if rgba else "G", "R" if rgba else "G")
    if rng.random() < 0.3:
        v = b.g.add({"Value": float(np.float32(rng.random() * 1.5 - 0.25))})
        b.out(v, 0, "G", "G")
    nested = False
    for k in range(int(rng.integers(2, 7))):
        if force and k == 1:
            b.menu_node("HeightToNormal")
        elif depth < 2 and not nested and rng.random() < 0.25:
            b.graph_node(depth + 1)
            nested = True
        else:
            b.menu_node()
    outputs = []
    for i in range(2 if force else int(rng.integers(1, 3))):
        rgba = bool(rng.random() < 0.5)
        src = b.pick("R" if rgba else "G", "R" if rgba else "G")
        if force and i == 0:  # the first Output behind the child's last node: nothing of the child is idle
            last = [o for o in b.outs if o[0] == b.made[-1]][0]
            rgba, src = last[3] == "R" and last[2] != "G", last
        n = b.g.add({"OutputRgba" if rgba else "OutputGray": "out%d" % i}, b.policy(1), b.filt())
        if src is not None:
            b.g.connect(src[0], n, src[1], 0)
        outputs.append((n, "R" if rgba else "G"))
    return b.g.dict(), inputs, outputs


def graph_node_case(orc, seed):
    """An outer graph (golden_graphs.G) of two to four Embeds, up to two Values and menu nodes, one to three of them Graph
    nodes (nesting up to depth 2, each with its own resize policy and filter); the first Graph node's child has two Output
    nodes and a HeightToNormal inside.  Embeds live in the outer graph only: a plan names them by the outer graph's node ids."""
    rng = np.random.default_rng(seed)
    b = _Builder(rng)
    embedded = {}
    for eid in range(int(rng.integers(2, 5))):
        rgba = bool(rng.random() < 0.6) or eid == 0
        planes = fz._source(rng, rgba, BAND_SIZES[:-1])
        embedded[eid] = orc.Image(planes)
        n = b.g.add({"Embed": eid})
        b.out(n, 0, "R", "R" if rgba else "G")
    for _ in range(int(rng.integers(0, 3))):
        n = b.g.add({"Value": float(np.float32(rng.random() * 1.5 - 0.25))})
        b.out(n, 0, "G", "G")
    b.menu_node("SeparateRgba")  # of the first Embed, an RGBA image: gray planes of real size for the Graph nodes' gray Inputs
    n_nodes = int(rng.integers(5, 16))
    at = sorted(int(i) for i in rng.choice(np.arange(1, n_nodes), size=int(rng.integers(1, 4)), replace=False))
    for k in range(n_nodes):
        if k in at:
            b.graph_node(1, force=k == at[0])
        else:
            b.menu_node()
    return Case(orc, b.g.dict(), embedded, b.made)


def below_graph_nodes(case):
    """The case's candidate nodes that are Graph nodes or have one among their ancestors."""
    reach = set(case.graph_nodes)
    grew = True
    while grew:
        grew = False
        for e in case.graph["edges"]:
            if e["output_id"] in reach and e["input_id"] not in reach:
                reach.add(e["input_id"])
                grew = True
    return [n for n in case.nodes if n in reach]


# ---------------------------------------------------------------------------------------------- targets and bands
def plan_flags(plan, h, y0, y1):
    """What a plan {node: (a, b, width, height)} of band [y0, y1) of an `h`-row result has in it."""
    flags = set()
    for a, b, _, sh in plan.values():
        if sh == h and b - a > y1 - y0:
            flags.add("halo")     # a same-height source asked for more rows than the band
        if sh != h and b - a < sh:
            flags.add("part")     # a strict part of a source of another height: a resize on the way
        if a < 0:
            flags.add("wrap")     # row -1: the last row, first
    return flags


def band_targets(ref, info, k=2):
    """The `k` nodes of info["nodes"] (ids, or the tuples of fz._build) most worth cutting into bands, as [(node id, rows of its
    first slot, flags)]: nodes the oracle `ref` evaluates and whose first slot has MIN_ROWS rows or more, scored by what
    band_source_rows of info["lg"] (a live graph of the same graph; a host-only one will do) says of the bands (h // 3, 2h // 3)
    and (0, 1) -- see plan_flags -- later nodes first among equals.  A plan the library refuses for a node the oracle accepts
    raises TexProError."""
    lg = info["lg"]
    scored = []
    for entry in info["nodes"]:
        n = int(entry[0] if isinstance(entry, tuple) else entry)
        try:
            slots = sorted(ref.node_slot_datas(n), key=lambda s: s.slot_id)
        except REFUSALS:
            continue
        if not slots:
            continue
        h = slots[0].image.size[1]
        if h < MIN_ROWS:
            continue
        flags = set()
        for y0, y1 in ((h // 3, 2 * h // 3), (0, 1)):
            flags |= plan_flags(lg.band_source_rows(n, y0, y1), h, y0, y1)
        scored.append((len(flags), n, h, flags))
    scored.sort(key=lambda t: (-t[0], -t[1]))
    return [(n, h, flags) for _, n, h, flags in scored[:k]]


def case_targets(case, k=2, nodes=None):
    return band_targets(case.ref, {"nodes": case.nodes if nodes is None else nodes, "lg": case.live_graph(host_kc())}, k)


def fixed_bands(h):
    return sorted(b for b in {(0, 1), (h - 1, h), (0, h), (h // 3, 2 * h // 3), (max(0, h - 3), h)} if b[0] < b[1])  # (h == 1: one band)


def band_sets(h, rng):
    """[(name, [(y0, y1), ...])]: the fixed bands, a tiling by 7 rows, and two to four random cuts stacked to the whole."""
    cuts = sorted({0, h} | {int(c) for c in rng.integers(1, h, size=int(rng.integers(1, 4)))}) if h > 1 else [0, 1]
    return [("fixed", fixed_bands(h)), ("tiles of 7", [(y, min(y + 7, h)) for y in range(0, h, 7)]),
            ("random cuts", list(zip(cuts[:-1], cuts[1:])))]


def noise_outside(rng, image, rows):
    """A copy of the orc.Image with every row outside `rows` = (a, b) (a < 0: row r means r mod h; None: no row is kept)
    replaced by fresh random values."""
    out = []
    for p in image.planes:
        h, w = p.shape
        q = (rng.random((h, w), dtype=np.float32) * np.float32(4.0) - np.float32(2.0)).astype(np.float32)
        if rows is not None:
            keep = sorted({r % h for r in range(rows[0], rows[1])})
            q[keep] = p[keep]
        out.append(q)
    return type(image)(out)
