"""What the steady-state fuzz tests share (tests/test_steady_fuzz_host.py, tests/test_gpu_fuzz_steady.py): random graphs in the
manner of tests/test_gpu_fuzz_graphs._build, shaped so that a LONG-LIVED graph reaches the forms only a repeated evaluation runs --
kernels compiled for a program (csrc/specialize.cpp), joined and wide programs, packed copies of sources (csrc/chain_pack.cpp),
the compiled up-sampling chain kernel and replay (csrc/replay.cpp).

A case is built on the host as graph JSON (golden_graphs.G), so the oracle needs nothing else and the same seed gives the same
graph whatever the device did before.  What differs from _build:
  * sizes: one "main" size per graph, mostly a dense one (w % 64 == 0: the pool's pitch is 4 w, rows flatten into one run, the
    two-quads-per-lane form and packing are eligible) whose quad count straddles the lane and workgroup edges of the one- and
    two-quad kernels (256, 272, 512, 528 quads ...), else one of _build's pitched and tiny sizes;
  * sources: 2 to 6 of the main size, each of one value kind -- "f32" (fits no tier), "fix24" (k * 2^-24), "u8" (k / 255.0f,
    as planes or through SlotImage.from_u8) -- and either clean (it packs) or carrying _build's IEEE edge values (it fails its
    tier); in graphs that are not "pure" one or two more of another size, the first a quarter as wide: integer-ratio up-sampling;
  * shape: a random body as in _build (Mix, invert, SeparateRgba, CombineRgba, HeightToNormal, policies and filters), then a Mix
    tree over 2 to 12 branches of the main size (BASELINE config #4's add tree is the model): joins inside joins, more than 4
    and more than 8 distinct planes in one program, the same plane on both sides of a Mix; "pure" seeds keep to the node types
    and sizes a recording allows (replay.cpp), the others cut chains with HeightToNormal and resized operands;
  * every output is tracked with the type and size that flow at run time, and in four graphs of five inputs are picked among the
    producers of the right type 19 times in 20: the reference refuses few graphs (test_steady_fuzz_host.py holds the cap of one
    quarter), and the ones it refuses the device must refuse too.
The requested node is the last one made.  Case.plugs lists one edge out of every Embed node: re-plugging them (connect with the
same ends) dirties everything below the sources, and the graph JSON already has those edges last, in that order, so a re-plugged
live graph keeps the edge order the oracle saw."""
import json

import numpy as np

from golden_graphs import G

DENSE = [(64, 16), (64, 17), (64, 32), (64, 33), (128, 3), (256, 5), (320, 1)]  # 256, 272, 512, 528, 96, 320, 80 quads
PITCHED = [(24, 16), (17, 29), (5, 3), (1, 1), (300, 40)]
KINDS = ["f32", "fix24", "u8"]
OPS = ["Add", "Subtract", "Multiply", "Divide"]
OP_WEIGHTS = [0.36, 0.26, 0.26, 0.12]  # Divide (and Pow) keep a program f32 and one quad per lane: fewer of them
FILTERS = ["Nearest", "Triangle", "CatmullRom", "Gaussian", "Lanczos3"]
EDGE_VALUES = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-42, 3e38], np.float32)  # _build's
CACHE_POLICIES = ["defaults", "budget0", "warm"]  # nothing, cache_budget_mb = 0, nt_force = 0x101 (the form that selects "_q2")
REFUSALS = (RuntimeError, AssertionError)

SEED_FORCED, N_FORCED = 0xF0510000, 60
SEED_NATURAL, N_NATURAL = 0xF0520000, 40
SEED_POW, N_POW = 0xF0530000, 24


class Source:
    """One embedded image: .kind, .clean (no edge values: the planes are what the kind says), .planes (float32, 1 or 4),
    .px (uint8 (h, w, 4) when the device image is made with SlotImage.from_u8, else None)."""

    def __init__(self, kind, clean, planes, px=None):
        self.kind, self.clean, self.planes, self.px = kind, clean, planes, px


def make_source(orc, rng, kind, w, h, rgba, clean, via_u8=False):
    if via_u8:
        px = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
        return Source("u8", True, orc.deconstruct_u8(px), px)
    planes = []
    for _ in range(4 if rgba else 1):
        u = rng.random((h, w), dtype=np.float32)
        if kind == "f32":
            p = (u * np.float32(1.6) - np.float32(0.3)).astype(np.float32)
        elif kind == "fix24":
            p = u
        else:
            p = np.floor(u * np.float32(256.0)).astype(np.float32) / np.float32(255.0)
        if not clean and p.size >= 12:
            p.reshape(-1)[rng.integers(p.size, size=3)] = rng.choice(EDGE_VALUES, 3)
        planes.append(p)
    return Source(kind, clean or planes[0].size < 12, planes)


def derived_size(policy, sizes):
    """The size a node's inputs are resized to where it follows without the reference's tie rules, else None.
    sizes: {input slot: (w, h) or None}, connected slots only."""
    if isinstance(policy, dict) and "SpecificSize" in policy:
        return (policy["SpecificSize"]["width"], policy["SpecificSize"]["height"])
    if not sizes:
        return (1, 1)
    if isinstance(policy, dict):  # SpecificSlot: that slot's input, else the lowest connected slot's
        slot = policy["SpecificSlot"]
        return sizes[slot] if slot in sizes else sizes[min(sizes)]
    known = list(sizes.values())
    if None in known:
        return None
    if len(set(known)) == 1:
        return known[0]
    if policy in ("MostPixels", "LargestAxes"):
        w, h = max(s[0] for s in known), max(s[1] for s in known)
        return (w, h) if (w, h) in known else None
    if policy in ("LeastPixels", "SmallestAxes"):
        w, h = min(s[0] for s in known), min(s[1] for s in known)
        return (w, h) if (w, h) in known else None
    return None


class _Builder:
    """Outputs are (node, slot, static type, run-time type, run-time size or None); static: "G", "R", "X" as connect() checks
    them (src/node/mod.rs:209-221), run-time: "G" / "R"."""

    def __init__(self, rng, main, pure, ops, weights):
        self.rng, self.g, self.main, self.pure, self.ops, self.weights = rng, G(), main, pure, ops, weights
        self.outs, self.made, self.quarter = [], [], None
        self.typed = 0.95 if rng.random() < 0.8 else 0.3  # one graph in five wires on the static types mostly, as _build does

    def op(self):
        return self.ops[self.rng.choice(len(self.ops), p=self.weights)]

    def pick(self, static, runtime=None, main=None):
        """An output a slot of the static type accepts; mostly (self.typed) one of the run-time type as well, and with main = True
        (False) one of the main size (of another size) where there is one."""
        rng = self.rng
        cands = [o for o in self.outs if static == "X" or o[2] in (static, "X")]
        if runtime is not None and rng.random() < self.typed:
            cands = [o for o in cands if o[3] == runtime] or cands
        if main is not None:
            const = main and rng.random() < 0.2  # a 1 x 1 constant beside the images now and then
            cands = [o for o in cands if (o[4] == self.main) == main or (const and o[4] == (1, 1))] or cands
        return cands[rng.integers(len(cands))] if cands else None

    def policy(self, ins):
        rng = self.rng
        sizes = {s: o[4] for s, o in enumerate(ins) if o is not None}
        same = None not in sizes.values() and len(set(sizes.values())) <= 1
        if self.pure:  # nothing that resamples an image: any policy where the inputs agree, the main size against constants
            names = ["MostPixels", "LeastPixels", "LargestAxes", "SmallestAxes", "SpecificSlot"] if same else ["MostPixels", "LargestAxes"]
        else:
            names = ["MostPixels"] * 4 + ["LargestAxes"] * 2 + ["LeastPixels", "SmallestAxes", "SpecificSlot", "SpecificSize", "SpecificSize"]
        k = names[rng.integers(len(names))]
        if k == "SpecificSlot":
            return {"SpecificSlot": int(rng.integers(max(len(ins), 1)))}
        if k == "SpecificSize":
            w, h = self.main if rng.random() < 0.7 else PITCHED[rng.integers(len(PITCHED))]
            return {"SpecificSize": {"width": w, "height": h}}
        return k

    def filt(self):
        rng = self.rng
        return ["Nearest", "Triangle"][rng.integers(2)] if rng.random() < 0.6 else FILTERS[rng.integers(len(FILTERS))]

    def node(self, node_type, ins, produces, policy=None):
        """Adds the node with a policy (a random one unless given) and a filter, connects `ins` (by slot, None: unconnected) in a
        shuffled order and registers `produces`: [(slot, static, run-time type)]."""
        pol = policy or self.policy(ins)
        n = self.g.add(node_type, pol, self.filt())
        order = list(range(len(ins)))
        self.rng.shuffle(order)  # edge insertion order != slot order: calculate_size iterates edges
        for s in order:
            if ins[s] is not None:
                self.g.connect(ins[s][0], n, ins[s][1], s)
        size = derived_size(pol, {s: o[4] for s, o in enumerate(ins) if o is not None})
        for slot, static, runtime in produces:
            self.outs.append((n, slot, static, runtime, size))
        self.made.append(n)
        return self.outs[-len(produces):]

    def mix(self, left, right, op=None, policy=None):
        first = left or right
        return self.node({"Mix": op or self.op()}, [left, right], [(0, "X", first[3] if first else "G")], policy)[0]

    def mix_resampled(self, x, y):
        """x (of the main size) with the image y of another size -- on either side where the types agree, else on the right: Mix
        converts its right input (src/node/mix.rs:51-134) -- under a policy that keeps x's size mostly."""
        rng = self.rng
        left = x[3] != y[3] or bool(rng.random() < 0.5)
        keep = [{"SpecificSlot": 0 if left else 1}, {"SpecificSlot": 0 if left else 1}, "MostPixels", "LargestAxes"][rng.integers(4)]
        return self.mix(x, y, policy=keep) if left else self.mix(y, x, policy=keep)

    def separate(self, src):
        outs = self.node("SeparateRgba", [src], [(s, "G", "G") for s in range(4)])
        if src is None or src[3] != "R":  # four 1 x 1 zeros (src/node/separate_rgba.rs:38-69)
            n = len(self.outs)
            self.outs[n - 4:] = [o[:4] + ((1, 1),) for o in outs]
        return self.outs[-4:]

    def menu_node(self):
        rng = self.rng
        r = rng.random()
        side = None if self.pure else (False if rng.random() < 0.3 else None)  # a resized operand now and then
        if r < 0.55:
            a = self.pick("X", main=True)
            b = a if rng.random() < 0.08 else self.pick("X", a[3] if a else None, main=True if side is None else False)
            ins = [a, b]
            if rng.random() < 0.5:
                ins.reverse()
            if rng.random() < 0.06:
                ins[rng.integers(2)] = None
            self.mix(ins[0], ins[1])
        elif r < 0.68:
            self.separate(self.pick("R", "R", main=True))
        elif r < 0.80:
            self.node("CombineRgba", [self.pick("G", "G", main=True) if rng.random() < 0.8 else None for _ in range(4)], [(0, "R", "R")])
        elif r < 0.90 and not self.pure:
            self.node("HeightToNormal", [self.pick("G", "G")], [(0, "R", "R")])
        else:  # invert: Mix(Subtract)(Value 1, x)
            one = self.g.add({"Value": 1.0})
            x = self.pick("X", main=True)
            self.node({"Mix": "Subtract"}, [(one, 0, "G", "G", (1, 1)), x], [(0, "X", "G")])

    def tree(self, raw_gray):
        """A Mix tree over 2 to 12 branches of the main size and one type.  raw_gray: the leaves and the branches' operands are
        planes of the sources themselves (gray Embeds, channels of a SeparateRgba of an RGBA Embed): every one a distinct input of
        the program.  -> the distinct planes among them (raw_gray), else 0."""
        rng = self.rng
        if raw_gray:
            pool = [o for o in self.outs if o[4] == self.main and o[3] == "G" and o[0] in self.raw_nodes]
            rt = "G"
        else:
            rt = "G" if rng.random() < 0.4 else "R"
            pool = [o for o in self.outs if o[4] == self.main and o[3] == rt]
            if len(pool) < 2:
                rt = "R" if rt == "G" else "G"
                pool = [o for o in self.outs if o[4] == self.main and o[3] == rt]
        if len(pool) < 2:
            return 0
        n_leaves = int(rng.integers(2, 13)) if raw_gray or rng.random() < 0.5 else int(rng.integers(2, 6))
        # images of another size, resampled by the branch that takes one (not in "pure" graphs: a recording holds no resample)
        sides = [] if self.pure else [o for o in self.outs if o[4] not in (self.main, (1, 1), None)]
        sides += [o for o in sides if o[4] == self.quarter]  # (the integer-ratio source twice as often)
        used = set()
        level = []
        for _ in range(n_leaves):
            x = pool[rng.integers(len(pool))]
            used.add(x[:2])
            for _ in range(int(rng.integers(0, 3))):  # the branch: up to two steps on the leaf
                if sides and rng.random() < 0.4:
                    x = self.mix_resampled(x, sides[rng.integers(len(sides))])
                    continue
                y = x if rng.random() < 0.1 else pool[rng.integers(len(pool))]
                used.add(y[:2])
                x = self.mix(x, y) if rng.random() < 0.6 else self.mix(y, x)
            level.append(x)
        while len(level) > 1:  # pairs, left to right; an odd one out moves up as it is
            nxt = []
            for i in range(0, len(level) - 1, 2):
                nxt.append(self.mix(level[i], level[i + 1], "Add" if rng.random() < 0.5 else None))
            if len(level) & 1:
                nxt.append(level[-1])
            level = nxt
        for _ in range(int(rng.integers(0, 3))):  # a tail on the root
            if sides and rng.random() < 0.3:
                level[0] = self.mix_resampled(level[0], sides[rng.integers(len(sides))])
            elif rng.random() < 0.5:
                y = pool[rng.integers(len(pool))]
                used.add(y[:2])
                level[0] = self.mix(level[0], y)
            else:
                v = self.g.add({"Value": float(np.float32(rng.random() * 1.5 - 0.25))})
                level[0] = self.mix(level[0], (v, 0, "G", "G", (1, 1)), None)
        return len(used) if raw_gray else 0


class Case:
    """One random graph: .graph (the JSON dict), .sources ({embed id: Source}), .embedded ({embed id: orc.Image}), .root (the
    requested node), .plugs ([(output node, input node, output slot, input slot)]: one edge out of every Embed node that has one),
    .cache_policy (one of CACHE_POLICIES), .raw_planes (distinct source planes under a raw gray tree, else 0), .pure."""

    def __init__(self, orc, seed, graph, sources, root, plugs, cache_policy, raw_planes, pure):
        self.orc, self.seed, self.graph, self.sources, self.root = orc, seed, graph, sources, int(root)
        self.plugs, self.cache_policy, self.raw_planes, self.pure = plugs, cache_policy, raw_planes, pure
        self.embedded = {eid: orc.Image([p.copy() for p in s.planes]) for eid, s in sources.items()}

    def json(self):
        return json.dumps(self.graph, sort_keys=True)

    def live_graph(self, kc):
        lg = kc.TextureProcessor.new().new_live_graph()
        lg.set_node_graph(kc.NodeGraph.from_json(json.dumps(self.graph)))
        for eid, s in self.sources.items():
            img = kc.SlotImage.from_u8(s.px) if s.px is not None else kc.SlotImage.from_planes(s.planes)
            lg.embed_slot_data_with_id(kc.SlotData(0, 0, img), eid)
        return lg

    def replug(self, lg):
        for o, i, os_, is_ in self.plugs:
            lg.connect(o, i, os_, is_)

    def want(self):
        """The oracle's slot datas of the requested node, sorted by slot id; None where the reference refuses it: mixed types ->
        InvalidBufferCount (src/node/node_type.rs:134), an RGBA image in a CombineRgba slot (src/node/combine_rgba.rs:23)."""
        try:
            ref = self.orc.RefGraph(self.graph, embedded=self.embedded)
            return sorted(ref.node_slot_datas(self.root), key=lambda s: s.slot_id)
        except REFUSALS as e:
            assert str(e) in ("InvalidBufferCount", "NodeProcessing") or "RGBA image into this slot" in str(e), e
            return None


def random_case(orc, seed, pow_ops=False):
    rng = np.random.default_rng(seed)
    main = DENSE[rng.integers(len(DENSE))] if rng.random() < 0.75 else PITCHED[rng.integers(len(PITCHED))]
    pure = bool(rng.random() < 0.5)
    raw_gray = bool(rng.random() < 0.35)
    ops, weights = (OPS + ["Pow"], [0.30, 0.22, 0.22, 0.10, 0.16]) if pow_ops else (OPS, OP_WEIGHTS)
    b = _Builder(rng, main, pure, ops, weights)
    sources, embeds = {}, []

    def embed(w, h, rgba):
        eid = len(sources)
        kind = KINDS[rng.integers(len(KINDS))]
        clean = bool(rng.random() < 0.65)
        via_u8 = kind == "u8" and rgba and clean and bool(rng.random() < 0.5)
        sources[eid] = make_source(orc, rng, kind, w, h, rgba, clean, via_u8)
        n = b.g.add({"Embed": eid})
        b.outs.append((n, 0, "R", "R" if rgba else "G", (w, h)))
        embeds.append(n)
        return b.outs[-1]

    mains = [embed(main[0], main[1], bool(rng.random() < (0.8 if raw_gray else 0.6))) for _ in range(int(rng.integers(2, 7)))]
    if not pure:
        for k in range(int(rng.integers(1, 3))):
            w, h = main
            ratio = [r for r in (4, 3, 1) if h % r == 0]
            if k == 0 and w % 4 == 0:  # a quarter as wide, a quarter, a third or all of the height: the up-sampling kernels
                size = b.quarter = (w // 4, h // ratio[rng.integers(len(ratio))])
            else:
                size = (DENSE + PITCHED)[rng.integers(len(DENSE) + len(PITCHED))]
            embed(size[0], size[1], bool(rng.random() < 0.6))
    for _ in range(int(rng.integers(0, 3))):
        n = b.g.add({"Value": float(np.float32(rng.random() * 1.5 - 0.25))})
        b.outs.append((n, 0, "G", "G", (1, 1)))
    b.raw_nodes = {o[0] for o in mains if o[3] == "G"}
    if raw_gray:
        for o in mains:  # the channels of every RGBA source of the main size: gray planes for the tree
            if o[3] == "R":
                b.raw_nodes.add(b.separate(o)[0][0])
    for _ in range(int(rng.integers(1, 8))):
        b.menu_node()
    raw_planes = b.tree(raw_gray) if rng.random() < 0.8 else 0
    return finish(orc, seed, b.g, sources, embeds, b.made[-1], CACHE_POLICIES[rng.choice(3, p=[0.3, 0.3, 0.4])], raw_planes, pure)


def finish(orc, seed, g, sources, embeds, root, cache_policy="defaults", raw_planes=0, pure=False):
    """The Case of a finished golden_graphs.G: one edge out of every Embed node of `embeds` becomes a plug and moves to the end
    of the edge list, as the live graph's connect will move it."""
    plugs = []
    for n in embeds:
        e = next((e for e in g.edges if e["output_id"] == n), None)
        if e is not None:
            plugs.append((e["output_id"], e["input_id"], e["output_slot"], e["input_slot"]))
    for p in plugs:
        g.connect(*p)
    return Case(orc, seed, g.dict(), sources, root, plugs, cache_policy, raw_planes, pure)


def joined_then_resampled(orc, small, big, filt):
    """The smallest graph with a resampled operand behind a join: ((a + b) - (a * b)) + s, a and b of the size `big`, s of the
    size `small`, resampled by the last Mix with the filter `filt`."""
    rng = np.random.default_rng([small[0], small[1], big[0], big[1]])
    g = G()
    sources = {0: make_source(orc, rng, "f32", big[0], big[1], False, True), 1: make_source(orc, rng, "fix24", big[0], big[1], False, True),
               2: make_source(orc, rng, "f32", small[0], small[1], False, True)}
    a, b, s_ = (g.add({"Embed": eid}) for eid in range(3))
    x, y, j = g.add({"Mix": "Add"}), g.add({"Mix": "Multiply"}), g.add({"Mix": "Subtract"})
    r = g.add({"Mix": "Add"}, "MostPixels", filt)
    for node, (left, right) in ((x, (a, b)), (y, (a, b)), (j, (x, y)), (r, (j, s_))):
        g.connect(left, node, 0, 0)
        g.connect(right, node, 0, 1)
    return finish(orc, "%dx%d -> %dx%d %s" % (small + big + (filt,)), g, sources, [a, b, s_], r)
