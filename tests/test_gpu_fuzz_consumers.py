"""GPU parity, differential: every consumer of an image -- the BC1/3/4/5, BC7 and BC6H encoders, mip chains, BC mip chains, the BC
error record, channel statistics and the typed device export -- put behind the plane states that random graphs produce.  The
graphs are test_gpu_fuzz_graphs._build's; a seed's requested slot is handed to a consumer straight after await_clean, so the
consumer is what forces a pending chain or a deferred resize, and the result is compared with the consumer's numpy reference
applied to the ORACLE's planes of that slot (oracle.RefGraph), never to planes downloaded from the device.  After the call the
image's planes must still be the oracle's, and a second call (the forced state) must give the same result again.

What is counted: on the second call, where nothing is left to force, the launches and algorithmic_bytes of a call are the formulas
of the consumers' own tests (test_gpu_bc, test_gpu_bc6h, test_gpu_bc_decode, test_gpu_bc_modes, test_gpu_channel_stats,
test_gpu_mips), with the number of distinct resident planes derived from the graph's JSON and the oracle (_provenance): a channel
is constant when it comes from a Value, a missing Mix or Combine input, the alpha of a Mix or HeightToNormal result, the outputs
of a SeparateRgba of a Gray image, or a Mix of two constants; two channels are one plane when they come from the same slot.
Launches only, no bytes, for the states where that derivation would be a guess: a constant plane larger than 1 x 1 that is
resized, and a CombineRgba that takes the same slot twice through a resize (whether the two results are one plane is the
evaluator's memo's business).  The fused mip kernel's launch count is a table of shapes in test_gpu_mips, not a formula: bytes only.

Two rows put the later mip rules behind the same states: "mips_rules" calls mips() under the five flag sets that are not the plain
rule (normals, coverage, both, alpha_weighted, alpha_weighted with coverage; tests/mip_states.py), fused and per level, in an order
drawn from the seed, against mip_states.reference of the oracle's planes, launches by test_gpu_mip_states.expected_mips_cost;
"bc_mips_rules" holds to_bc_mips under each rule to levels_to_bc_mips of the chain mips() builds and to bc_ref / bc1a_ref of the
reference levels.  The rules are for RGBA images: on a Gray slot both rows assert the documented refusal and that nothing is launched.

Each seed runs ROWS_PER_SEED of the ten consumer rows, drawn from the seed (all ten fit the time).  Among the slots of the
nodes _build requests, the one taken is larger than 1 x 1 and an aliased CombineRgba if it can be (either alone comes next), then has a
constant channel, then is Gray: left to chance, two thirds of the seeds would hand over a 1 x 1 image and aliased channels
would hardly occur.  The last test asserts that every row met every state and that at most a quarter of the seeds had to be
skipped because the reference refuses their nodes.  No seed has found a defect so far; one that does is pinned in a
test_seeds_that_found_defects case here, with its cause, as test_gpu_fuzz_graphs does.

test_exporters_count_distinct_resident_planes pins the same count of distinct resident planes on the exporters the rows' formulas
leave out -- to_u8, to_torch to U8 and the u8 pipe's download -- on hand-made aliased, constant and Gray images, next to BC3.

Run time on an MI355X: 19 s for the module (163 tests: 120 seeds with ten rows each, 40 hand-made cases, the two exporter-count
cases, the coverage test), of
which 12 s are the first test's set-up (library start-up); no seed takes longer than 0.3 s."""
import ctypes as C

import numpy as np
import pytest

import bc1a_ref
import bc6h_ref
import bc7_ref
import bc_decode_ref
import bc_modes_ref
import bc_ref
import mip_ref
import mip_states
from test_gpu_bc_decode import record
from test_gpu_device_image import u16_formula
from test_gpu_fuzz_graphs import _build
from test_gpu_mip_states import EXPORT, expected_mips_cost
from util import SEED_A, assert_planes, bit_equal, key_range, splitmix_plane

pytestmark = pytest.mark.gpu

BASE = 0xF0270000  # test_gpu_fuzz_graphs uses 0xF0220000 .. 0xF0260000 and the soak 0xF0990000
SEEDS = 120
ROWS_PER_SEED = 10
BC7, BC6H = 98, 95
BC_SRGB, BC_ALL_MODES = 1, 16
BC_FORMS = [(1, False), (1, True), (3, False), (3, True), (4, False), (5, False)]
ALL_FORMS = BC_FORMS + [(BC7, False), (BC7, True), (BC6H, False)]
BLOCK_BYTES = {1: 8, 3: 16, 4: 8, 5: 16, BC7: 16, BC6H: 16}
READ_MASK = {1: 0x7, 3: 0xF, 4: 0x1, 5: 0x3, BC7: 0xF, BC6H: 0x7}  # the channels a format's encoder and comparison read
ROWS = ["bc", "bc7", "bc6h", "mips", "bc_mips", "bc_error", "stats", "export", "mips_rules", "bc_mips_rules"]
STATES = ["gray", "aliased", "constant", "mix", "resize", "w%4", "h%4", "1x1"]

_TALLY = set()   # (row, state) pairs that a seed test reached
_RAN = {}        # seed -> "skipped" or "ran"


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    return kc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ------------------------------------------------------------------ the state of a slot, from the graph's JSON and the oracle
class _Ambiguous(Exception):
    """the number of resident planes is not derivable from the oracle side for this slot"""


def _kind(node):
    nt = node["node_type"]
    return (nt, None) if isinstance(nt, str) else next(iter(nt.items()))


def _inputs(orc, ref, nid):
    """-> (edges in slot order, {input slot: (source node, source slot, oracle size)}, the size the node resizes them to)"""
    edges = [e for e in ref.edges if e["input_id"] == nid]
    by_slot = sorted(edges, key=lambda e: e["input_slot"])
    sds = [ref.slot_data(e["output_id"], e["output_slot"]) for e in edges]
    target = orc.ref_calculate_size(sds, by_slot, ref.nodes[nid]) if sds else None
    return by_slot, {e["input_slot"]: (e["output_id"], e["output_slot"], sd.size) for e, sd in zip(edges, sds)}, target


def _provenance(orc, ref, nid, memo):
    """{output slot: [key per channel]} of a node: None for a constant channel, otherwise a value that two channels share exactly
    when they are one resident plane.  Raises _Ambiguous where that cannot be told from the graph."""
    if nid in memo:
        return memo[nid]
    kind, arg = _kind(ref.nodes[nid])
    if kind == "Embed":
        out = {0: [("embed", arg, c) for c in range(len(ref.embedded[arg].planes))]}
    elif kind == "Value":
        out = {0: [None]}
    else:
        _, srcs, target = _inputs(orc, ref, nid)
        ins, resized_from = {}, []
        for slot, (src, src_slot, size) in srcs.items():
            keys = list(_provenance(orc, ref, src, memo)[src_slot])
            if size != target:
                for c, k in enumerate(keys):
                    if k is None:
                        if size != (1, 1):
                            raise _Ambiguous("a constant plane of %s is resized" % (size,))
                    else:
                        if (src, src_slot) in resized_from and kind == "CombineRgba":
                            raise _Ambiguous("one slot resized into two CombineRgba inputs")
                        keys[c] = ("resized", nid, slot, c)
                resized_from.append((src, src_slot))
            ins[slot] = keys
        if kind == "Mix":
            left, right = ins.get(0), ins.get(1)
            if left is None and right is None:
                out = {0: [None]}
            else:
                n = len(left if left is not None else right)
                if left is None:
                    left = [None] * n
                if right is None:
                    right = [None] * n
                elif len(right) != n:  # as_type: Gray -> [p, p, p, ones]; RGBA -> (r + g + b) / 3, constants fold
                    right = [right[0]] * 3 + [None] if n == 4 else [None if right[:3] == [None] * 3 else ("as gray", nid)]
                mixed = [None if l is None and r is None else ("mix", nid, c) for c, (l, r) in enumerate(zip(left, right))]
                out = {0: mixed[:3] + [None] if n == 4 else mixed}
        elif kind == "SeparateRgba":
            keys = ins.get(0)
            out = {i: [keys[i]] if keys is not None and len(keys) == 4 else [None] for i in range(4)}
        elif kind == "CombineRgba":
            out = {0: [ins[i][0] if i in ins else None for i in range(4)]}
        elif kind == "HeightToNormal":
            out = {0: [("normal", nid, c) for c in range(3)] + [None]}
        else:
            raise NotImplementedError(kind)
    memo[nid] = out
    return out


def _resident(keys, mask=0xF, rgba_view=True):
    """distinct resident planes among the channels of `mask`; a Gray image is read as (v, v, v, 1) where rgba_view"""
    if keys is None:
        return None
    if len(keys) == 1 and rgba_view:
        keys = [keys[0]] * 3 + [None]
    return len({k for c, k in enumerate(keys) if (mask >> c) & 1 and k is not None})


def _states(orc, ref, nid, slot, image):
    kind, _ = _kind(ref.nodes[nid])
    by_slot, srcs, target = _inputs(orc, ref, nid)
    w, h = image.size
    st = set()
    if not image.is_rgba:
        st.add("gray")
    if kind == "CombineRgba":
        seen = {}
        for e in by_slot:
            first = seen.setdefault((e["output_id"], e["output_slot"]), e["input_slot"])
            if first != e["input_slot"] and bit_equal(image.planes[first], image.planes[e["input_slot"]]):
                st.add("aliased")
        if len(srcs) < 4 or any(_kind(ref.nodes[s[0]])[0] == "Value" for s in srcs.values()):
            st.add("constant")
    if kind == "Mix":
        st.add("mix")
        if srcs and all(_kind(ref.nodes[s[0]])[0] == "Value" for s in srcs.values()):
            st.add("constant")
    if any(s[2] != target for s in srcs.values()):
        st.add("resize")
    if w % 4:
        st.add("w%4")
    if h % 4:
        st.add("h%4")
    if (w, h) == (1, 1):
        st.add("1x1")
    return st


def _plan(kc, orc, seed):
    """-> None when the reference refuses every requested node, else a dict: the node and slot to consume, the oracle's image,
    the slot's states, its channel keys (None: ambiguous) and the consumer rows of this seed"""
    _, ref, requested = _build(kc, orc, seed)
    cands = []
    for n in dict.fromkeys(int(n) for n in requested):
        try:
            sds = ref.node_slot_datas(n)
        except (RuntimeError, AssertionError) as e:
            assert str(e) in ("InvalidBufferCount", "NodeProcessing") or "RGBA image into this slot" in str(e), e
            continue
        for sd in sorted(sds, key=lambda s: s.slot_id):
            st = _states(orc, ref, n, int(sd.slot_id), sd.image)
            cands.append(((("aliased" not in st) + ("1x1" in st), "constant" not in st, "gray" not in st), len(cands), n, int(sd.slot_id), sd.image, st))
    if not cands:
        return None
    _, _, n, slot, image, st = min(cands, key=lambda c: c[:2])
    try:
        keys = _provenance(orc, ref, n, {})[slot]
        assert len(keys) == len(image.planes)
    except _Ambiguous:
        keys = None
    rng = np.random.default_rng([seed, 1])
    rows = [ROWS[i] for i in sorted(rng.choice(len(ROWS), size=ROWS_PER_SEED, replace=False))]
    return dict(node=n, slot=slot, image=image, states=st, keys=keys, rows=rows)


# ------------------------------------------------------------------ the consumer rows
# A row is a function (kc, orc, torch, src, rng) -> variants; a variant is (name, call, want, cost): call() -> the result in a
# comparable form (see _same), want the reference's, cost (launches or None, algorithmic bytes or None) of a call on the forced
# image.  The first variant is called first (it forces), then again; the others once each.  src: a dict with the oracle's image
# ("image"), the channel keys ("keys"), img() -> the SlotImage, and for a graph slot "lg", "node" and "slot".
def _ref_blocks(orc, image, fmt, srgb):
    if fmt == BC6H:
        return bc6h_ref.encode(image.planes)
    px = orc.to_u8(image, srgb)
    return bc7_ref.encode(px) if fmt == BC7 else bc_ref.encode(px, fmt)


def _encode_cost(src, fmt):
    w, h = src["image"].size
    n = _resident(src["keys"], READ_MASK[fmt])
    return 1, None if n is None else w * h * 4 * n + ((w + 3) // 4) * ((h + 3) // 4) * BLOCK_BYTES[fmt]


def _encode_variants(kc, orc, torch, src, rng, forms):
    out = []
    for fmt, srgb in forms:
        entry = ["host", "torch", "live"][rng.integers(3 if "lg" in src else 2)]
        if entry == "host":
            call = lambda fmt=fmt, srgb=srgb: src["img"]().to_bc(fmt, srgb)  # noqa: E731
        elif entry == "torch":
            call = lambda fmt=fmt, srgb=srgb: src["img"]().to_bc_torch(fmt, srgb).cpu().numpy()  # noqa: E731
        else:
            call = lambda fmt=fmt, srgb=srgb: src["lg"].buffer_bc_torch(src["node"], src["slot"], fmt, srgb).cpu().numpy()  # noqa: E731
        out.append(("BC%d srgb=%s %s" % (fmt, srgb, entry), call, _ref_blocks(orc, src["image"], fmt, srgb), _encode_cost(src, fmt)))
    return out


def row_bc(kc, orc, torch, src, rng):
    return _encode_variants(kc, orc, torch, src, rng, [BC_FORMS[i] for i in rng.permutation(len(BC_FORMS))])


def row_bc7(kc, orc, torch, src, rng):
    first = bool(rng.integers(2))
    return _encode_variants(kc, orc, torch, src, rng, [(BC7, first), (BC7, not first)])


def row_bc6h(kc, orc, torch, src, rng):
    return _encode_variants(kc, orc, torch, src, rng, [(BC6H, False)])


def _ref_levels(image):
    """[level][channel] planes of the oracle image's mip chain"""
    chains = [mip_ref.chain(p) for p in image.planes]
    w, h = image.size
    assert len(chains[0]) == mip_ref.level_count(w, h)
    for k in range(len(chains[0])):
        assert chains[0][k].shape == mip_ref.level_size(w, h, k)[::-1]
    return [[c[k] for c in chains] for k in range(len(chains[0]))]


def row_mips(kc, orc, torch, src, rng):
    image = src["image"]
    w, h = image.size
    want = _ref_levels(image)
    n = _resident(src["keys"], rgba_view=False)
    texels = sum(a * b for a, b in (mip_ref.level_size(w, h, k) for k in range(len(want))))
    nbytes = None if n is None else (4 * n * texels if w * h > 1 else 0)

    def call(per_level):
        levels = src["img"]().mips(per_level=per_level)
        return [lv.planes() for lv in levels]
    first = bool(rng.integers(2))
    out = []
    for per_level in (first, not first):
        launches = (0 if n == 0 else None if n is None else len(want) - 1) if per_level else (0 if n == 0 or w * h == 1 else None)
        out.append(("mips per_level=%s" % per_level, lambda p=per_level: call(p), want, (launches, nbytes)))
    return out


def row_bc_mips(kc, orc, torch, src, rng):
    image = src["image"]
    w, h = image.size
    fmt, srgb = ALL_FORMS[rng.integers(len(ALL_FORMS))]
    per_level = bool(rng.integers(2))
    levels = [_ref_blocks(orc, orc.Image(planes), fmt, srgb) for planes in _ref_levels(image)]
    offs, total = kc.bc_mip_layout(w, h, fmt)
    sizes = [lv.size for lv in levels]
    assert offs == [int(v) for v in np.cumsum([0] + sizes[:-1])] and total == sum(sizes)  # tightly packed, level 0 first
    flat = np.concatenate([lv.reshape(-1) for lv in levels])
    entry = ["host", "torch", "live"][rng.integers(3 if "lg" in src else 2)]
    if entry == "host":
        return [("BC%d chain host" % fmt, lambda: src["img"]().to_bc_mips(fmt, srgb, per_level=per_level), levels, (None, None))]

    def call():
        if entry == "torch":
            t, o = src["img"]().to_bc_mips_torch(fmt, srgb, per_level=per_level)
        else:
            t, o = src["lg"].buffer_bc_mips_torch(src["node"], src["slot"], fmt, srgb, per_level=per_level)
        return [t.cpu().numpy(), np.array(o, np.int64)]
    return [("BC%d chain %s" % (fmt, entry), call, [flat, np.array(offs, np.int64)], (None, None))]


def _flat_record(e):
    r = record(e)
    return [np.array([r["format"], r["channel_mask"], r["pixels"], r["undecoded_blocks"], e.flags], np.int64), np.array(r["sse"], np.uint64),
            np.array(r["max_abs"], np.int64), np.array(r["bc7_mode_blocks"], np.int64)]


def _want_record(r, flags):
    return [np.array([r["format"], r["channel_mask"], r["pixels"], r["undecoded_blocks"], flags], np.int64), np.array(r["sse"], np.uint64),
            np.array(r["max_abs"], np.int64), np.array(r["bc7_mode_blocks"], np.int64)]


def row_bc_error(kc, orc, torch, src, rng):
    image = src["image"]
    w, h = image.size
    fmt, srgb = ALL_FORMS[rng.integers(len(ALL_FORMS))]
    nblk = ((w + 3) // 4) * ((h + 3) // 4) * BLOCK_BYTES[fmt]
    n = _resident(src["keys"], READ_MASK[fmt])
    if fmt == BC6H:
        own = bc6h_ref.compare(image.planes, bc6h_ref.encode(image.planes))
    else:
        px = orc.to_u8(image, srgb)
        own = bc_decode_ref.error_record(px, _ref_blocks(orc, image, fmt, srgb), fmt)
    live = "lg" in src and bool(rng.integers(2))
    if live:
        call = lambda: _flat_record(src["lg"].buffer_bc_error(src["node"], src["slot"], fmt, srgb))  # noqa: E731
    else:
        call = lambda: _flat_record(src["img"]().bc_error(fmt, srgb))  # noqa: E731
    out = [("bc_error BC%d srgb=%s %s" % (fmt, srgb, "live" if live else "image"), call, _want_record(own, BC_SRGB if srgb else 0),
            (3, None if n is None else 2 * (nblk + 4 * w * h * n)))]
    # another encoder's blocks, every mode among them
    mfmt, msrgb = [(BC7, False), (BC7, True), (BC6H, False)][rng.integers(3)]
    blk = bc_modes_ref.random_image_blocks(mfmt, h, w, seed=5)
    want = bc_modes_ref.error_record(orc.to_u8(image, msrgb) if mfmt == BC7 else image.planes, blk, mfmt)
    m = _resident(src["keys"], READ_MASK[mfmt])

    def compare():
        t = torch.from_numpy(blk).cuda()
        return _flat_record(src["img"]().bc_error(mfmt, msrgb, blocks=t, all_modes=True))
    out.append(("bc_error blocks BC%d srgb=%s" % (mfmt, msrgb), compare, _want_record(want, BC_ALL_MODES | (BC_SRGB if msrgb else 0)),
                (2, None if m is None else blk.size + 4 * w * h * m)))
    return out


def _want_stats(orc, image, histogram, srgb):
    w, h = image.size
    lo_hi, nans = [], []
    for p in image.planes:
        lo, hi, k = key_range(p)
        lo_hi.append([-1, -1] if lo is None else [lo, hi])
        nans.append(k)
    out = [np.array([w * h, len(image.planes)], np.int64), np.array(lo_hi, np.int64), np.array(nans, np.int64)]
    if histogram:
        px = orc.to_u8(image, srgb)
        out.append(np.stack([np.bincount(px[:, :, c].reshape(-1), minlength=256) for c in range(len(image.planes))]).astype(np.int64))
    return out


def _flat_stats(st, histogram):
    lo_hi = [[-1, -1] if np.isnan(a) and np.isnan(b) else [int(np.float32(a).view(np.uint32)), int(np.float32(b).view(np.uint32))]
             for a, b in zip(st.min, st.max)]
    out = [np.array([st.pixels, len(st.min)], np.int64), np.array(lo_hi, np.int64), np.array(st.nan_count, np.int64)]
    if histogram:
        assert st.histogram.dtype == np.uint64
        out.append(st.histogram.astype(np.int64))
    else:
        assert st.histogram is None
    return out


def row_stats(kc, orc, torch, src, rng):
    image = src["image"]
    w, h = image.size
    modes = [(False, False), (True, False), (True, True)]
    order = [modes[i] for i in rng.permutation(3)]
    out = []
    for histogram, srgb in order:
        live = "lg" in src and bool(rng.integers(2))
        if src["keys"] is None:
            cost = (None, None)
        else:  # one slot per distinct resident plane and quantiser: alpha is binned linearly under srgb
            slots = len({(k, srgb and c < 3) for c, k in enumerate(src["keys"]) if k is not None})
            cost = (2, w * h * 4 * slots) if slots else (0, 0)
        if live:
            call = lambda hi=histogram, s=srgb: _flat_stats(src["lg"].buffer_channel_stats(src["node"], src["slot"], histogram=hi, srgb=s), hi)  # noqa: E731
        else:
            call = lambda hi=histogram, s=srgb: _flat_stats(src["img"]().channel_stats(histogram=hi, srgb=s), hi)  # noqa: E731
        out.append(("stats histogram=%s srgb=%s %s" % (histogram, srgb, "live" if live else "image"), call, _want_stats(orc, image, histogram, srgb), cost))
    return out


def _as_rgba(image):
    """the four channels every exporter sees: a Gray image is (v, v, v, 1)"""
    if image.is_rgba:
        return list(image.planes)
    p = image.planes[0]
    return [p, p, p, np.ones(p.shape, np.float32)]


def _half_bits(t, torch):
    """a float16 / bfloat16 tensor -> int32 bit patterns, every NaN as -1"""
    bits = t.view(torch.int16).numpy().astype(np.int32) & 0xffff
    return np.where(torch.isnan(t).numpy(), -1, bits)


def row_export(kc, orc, torch, src, rng):
    image = src["image"]
    w, h = image.size
    names = ["uint8", "uint8 srgb", "uint16", "float16", "bfloat16", "float32"]
    out = []
    for i in rng.choice(len(names), size=4, replace=False):
        name, layout, channels = names[i], ["hwc", "chw"][rng.integers(2)], int(rng.integers(1, 5))
        srgb = name == "uint8 srgb"
        dt = getattr(torch, name.split()[0])
        stacked = np.stack(_as_rgba(image)[:channels], 2 if layout == "hwc" else 0)
        if dt == torch.uint8:
            px = orc.to_u8(image, srgb)[:, :, :channels]
            want = px if layout == "hwc" else px.transpose(2, 0, 1)
        elif dt == torch.uint16:
            want = u16_formula(stacked)
        elif dt == torch.float32:
            want = stacked
        else:
            want = _half_bits(torch.from_numpy(stacked).to(dt), torch)
        live = "lg" in src and bool(rng.integers(2))

        def call(dt=dt, layout=layout, channels=channels, srgb=srgb, live=live):
            if live:
                t = src["lg"].buffer_torch(src["node"], src["slot"], dt, layout=layout, channels=channels, srgb=srgb)
            else:
                t = src["img"]().to_torch(dt, layout=layout, channels=channels, srgb=srgb)
            t = t.cpu()
            return _half_bits(t, torch) if dt in (torch.float16, torch.bfloat16) else t.numpy()
        out.append(("export %s %s %d %s" % (name, layout, channels, "live" if live else "image"), call, np.ascontiguousarray(want), (None, None)))
    return out


RULES = mip_states.FLAG_SETS[1:]  # the five flag sets of mips() that are not the plain rule


def _refusals(kc, src, calls):
    """The variant of a rule row on a Gray slot: every call is refused as the header documents, and nothing is launched."""
    def call():
        img = src["img"]()
        n0 = kc.stats()["kernel_launches"]
        for c in calls:
            with pytest.raises(kc.TexProError):
                c(img)
        assert kc.stats()["kernel_launches"] == n0
        return [np.array([len(calls)], np.int64)]
    return [("refused on a Gray image", call, [np.array([len(calls)], np.int64)], (0, 0))]


def _rule_cost(src, flags, per_level):
    """launches of mips(**flags) by test_gpu_mip_states.expected_mips_cost, residency from _provenance; None where ambiguous"""
    keys, image = src["keys"], src["image"]
    if keys is None:
        return None, None
    info = [(k is None, image.planes[ch].reshape(-1)[0], k) for ch, k in enumerate(keys)]
    return expected_mips_cost(flags, info, image.size[0], image.size[1], per_level)[1], None


def row_mips_rules(kc, orc, torch, src, rng):
    image = src["image"]
    if not image.is_rgba:
        return _refusals(kc, src, [lambda img, f=f, p=p: img.mips(per_level=p, **f) for f in RULES for p in (False, True)])
    out = []
    for i in rng.permutation(2 * len(RULES)):
        flags, per_level = RULES[i // 2], bool(i % 2)
        chains = mip_states.reference(image.planes, flags)
        want = [[c[k] for c in chains] for k in range(len(chains[0]))]
        out.append(("mips %s per_level=%s" % (mip_states.flag_id(flags), per_level),
                    lambda f=flags, p=per_level: [lv.planes() for lv in src["img"]().mips(per_level=p, **f)], want, _rule_cost(src, flags, per_level)))
    return out


def row_bc_mips_rules(kc, orc, torch, src, rng):
    """to_bc_mips under a rule encodes the chain mips builds under it; the blocks are the encoders' references of the reference levels"""
    image = src["image"]
    forms = [(flags,) + EXPORT[mip_states.flag_id(flags)] for flags in RULES]
    if not image.is_rgba:
        return _refusals(kc, src, [lambda img, f=f, fmt=fmt, pt=pt: img.to_bc_mips(fmt, punch_through=pt, **f) for f, fmt, pt in forms])
    out = []
    for i in rng.permutation(len(forms)):
        flags, fmt, punch = forms[i]
        ref = flags["coverage"] if punch else None
        chains = mip_states.reference(image.planes, flags)
        want = []
        for k in range(len(chains[0])):
            px = orc.to_u8(orc.Image([c[k] for c in chains]), False)
            want.append(bc1a_ref.encode(px, ref) if punch else bc_ref.encode(px, fmt))

        def call(flags=flags, fmt=fmt, punch=punch, ref=ref):
            img = src["img"]()
            got = img.to_bc_mips(fmt, punch_through=punch, **flags)
            _same(kc.levels_to_bc_mips(img.mips(**flags), fmt, punch_through=ref), got, "levels_to_bc_mips of mips(%s)" % mip_states.flag_id(flags))
            return got
        out.append(("BC%d chain %s" % (fmt, mip_states.flag_id(flags)), call, want, (None, None)))
    return out


ROW_FUNCTIONS = dict(bc=row_bc, bc7=row_bc7, bc6h=row_bc6h, mips=row_mips, bc_mips=row_bc_mips, bc_error=row_bc_error, stats=row_stats,
                     export=row_export, mips_rules=row_mips_rules, bc_mips_rules=row_bc_mips_rules)


# ------------------------------------------------------------------ the comparison and the driver
def _same(got, want, what):
    """equal in shape and bits; float32 under the suite's rule (any NaN equals any NaN); lists element by element"""
    if isinstance(want, (list, tuple)):
        assert isinstance(got, (list, tuple)) and len(got) == len(want), "%s: %d results, not %d" % (what, len(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, "%s [%d]" % (what, i))
        return
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, not %s" % (what, got.shape, want.shape)
    assert got.dtype == want.dtype, "%s: dtype %s, not %s" % (what, got.dtype, want.dtype)
    if want.dtype == np.float32:
        assert bit_equal(got, want), "%s: %d of %d values differ" % (
            what, int((~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))).sum()), want.size)
    else:
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s: %d of %d values differ, first at %s: %s, not %s" % (
            what, len(bad), want.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def _counted(kc, call):
    s0 = kc.stats()
    got = call()
    s1 = kc.stats()
    return got, s1["kernel_launches"] - s0["kernel_launches"], s1["algorithmic_bytes"] - s0["algorithmic_bytes"]


def _check_cost(launches, nbytes, cost, what):
    if cost[0] is not None:
        assert launches == cost[0], "%s: %d launches, not %d" % (what, launches, cost[0])
    if cost[1] is not None:
        assert nbytes == cost[1], "%s: %d algorithmic bytes, not %d" % (what, nbytes, cost[1])


def _consume(kc, orc, torch, row, make, rng, what):
    """One row against one freshly made source: the first variant forces the image, leaves it intact and repeats itself; the
    others follow on the forced image."""
    src = make()
    variants = ROW_FUNCTIONS[row](kc, orc, torch, src, rng)
    name, call, want, cost = variants[0]
    got = call()  # before anything else touches the image
    _same(got, want, "%s %s" % (what, name))
    img = src["img"]()
    assert img.is_rgba() == src["image"].is_rgba and tuple(img.size()) == src["image"].size, what
    assert_planes(img.planes(), src["image"].planes, what="%s: planes after %s" % (what, name))
    again, launches, nbytes = _counted(kc, call)
    _same(again, want, "%s %s, second call" % (what, name))
    _same(again, got, "%s %s, second call against the first" % (what, name))
    _check_cost(launches, nbytes, cost, "%s %s" % (what, name))
    for name, call, want, cost in variants[1:]:
        got, launches, nbytes = _counted(kc, call)
        _same(got, want, "%s %s" % (what, name))
        _check_cost(launches, nbytes, cost, "%s %s" % (what, name))
    assert_planes(img.planes(), src["image"].planes, what="%s: planes after every variant" % what)


def _graph_source(kc, orc, seed, plan):
    def make():
        lg, _, _ = _build(kc, orc, seed)  # a fresh graph per consumer: forcing may change the image in place
        lg.await_clean(plan["node"])
        return dict(image=plan["image"], keys=plan["keys"], lg=lg, node=plan["node"], slot=plan["slot"],
                    img=lambda: lg.slot_data(plan["node"], plan["slot"]).image)
    return make


def _run_seed(kc, orc, torch, seed, rows=None):
    plan = _plan(kc, orc, seed)
    if plan is None:
        return None
    for i, row in enumerate(plan["rows"] if rows is None else rows):
        _consume(kc, orc, torch, row, _graph_source(kc, orc, seed, plan), np.random.default_rng([seed, 2, ROWS.index(row)]),
                 "seed %#x node %d slot %d %s" % (seed, plan["node"], plan["slot"], sorted(plan["states"])))
    return plan


@pytest.mark.parametrize("seed", range(SEEDS))
def test_consumers_behind_a_random_graph(kc, orc, torch, seed):
    plan = _run_seed(kc, orc, torch, BASE + seed)
    _RAN[seed] = "skipped" if plan is None else "ran"
    if plan is not None:
        _TALLY.update((row, st) for row in plan["rows"] for st in plan["states"])


# ------------------------------------------------------------------ states _build cannot produce
def _gray_chain_as_rgba(kc, orc):
    h, w = 13, 18
    a, b = splitmix_plane(SEED_A, 0, h, w) * np.float32(1.4) - np.float32(0.2), splitmix_plane(SEED_A, 1, h, w)
    a[0, :4] = [np.nan, np.inf, -0.0, -np.inf]
    g = kc.mix_process(kc.SlotImage.from_planes([a]), kc.SlotImage.from_planes([b]), kc.MixType.Multiply).as_type(True)
    p = orc.mix_plane("Multiply", a, b)
    return dict(image=orc.Image([p, p, p, np.ones((h, w), np.float32)]), keys=["p", "p", "p", None], img=lambda: g)


def _wrapped_with_pool_planes(kc, orc):
    import torch
    from kanter_core_amd import _lib
    L = _lib.load()
    h, w, pitch_f = 19, 10, 20
    p = [splitmix_plane(SEED_A, 2 + c, h, w) * np.float32(1.2) - np.float32(0.1) for c in range(3)]
    p[0][1, :3] = [np.nan, np.inf, -0.0]
    t = torch.empty((h, pitch_f), dtype=torch.float32, device="cuda")
    t[:, :] = torch.tensor([float("nan"), -float("inf"), 1e30, -1e30], dtype=torch.float32).repeat(pitch_f // 4).cuda()
    t[:, :w] = torch.from_numpy(p[0]).cuda()
    torch.cuda.synchronize()
    plane, handle = C.c_void_p(), C.c_void_p()
    assert L.kc_plane_wrap(t.data_ptr(), w, h, pitch_f * 4, C.byref(plane)) == 0
    assert L.kc_image_gray(plane, C.byref(handle)) == 0
    L.kc_plane_release(plane)
    wrapped = kc.SlotImage(handle.value)
    img = kc.combine_rgba_process([wrapped, kc.SlotImage.from_planes([p[1]]), wrapped, kc.SlotImage.from_planes([p[2]])])
    return dict(image=orc.Image([p[0], p[1], p[0], p[2]]), keys=["wrapped", "pool 1", "wrapped", "pool 2"], img=lambda: img, keep=(t, wrapped))


def _nothing_connected(kc, orc):
    img = kc.combine_rgba_process([None, None, None, None])
    zero = np.zeros((1, 1), np.float32)
    return dict(image=orc.Image([zero, zero, zero, np.ones((1, 1), np.float32)]), keys=[None] * 4, img=lambda: img)


def _chain_longer_than_a_program(kc, orc):
    """test_gpu_chain_edges._long_chain's 150 steps over seven planes: the record limit cuts it, and it is pending here"""
    h, w = 24, 40
    planes = [splitmix_plane(SEED_A + i, 0, h, w) * np.float32(0.5) + np.float32(0.25) for i in range(7)]
    imgs = [kc.SlotImage.from_planes([p]) for p in planes]
    ops = ["Add", "Multiply", "Subtract", "Multiply", "Add"]
    x, want = imgs[0], planes[0]
    for i in range(150):
        k = 1 + (i * 5 + i // 7) % 6
        op = ops[i % len(ops)]
        if i % 3 == 0:
            x = kc.mix_process(imgs[k], x, kc.MixType.parse(op))
            want = orc.mix_plane(op, planes[k], want)
        else:
            x = kc.mix_process(x, imgs[k], kc.MixType.parse(op))
            want = orc.mix_plane(op, want, planes[k])
    return dict(image=orc.Image([want]), keys=["chain"], img=lambda: x)


HAND_STATES = {"gray chain as rgba": _gray_chain_as_rgba, "wrapped plane with pool planes": _wrapped_with_pool_planes,
               "nothing connected": _nothing_connected, "chain longer than a program": _chain_longer_than_a_program}


@pytest.mark.parametrize("row", ROWS)
@pytest.mark.parametrize("state", list(HAND_STATES))
def test_consumers_behind_hand_made_states(kc, orc, torch, state, row):
    _consume(kc, orc, torch, row, lambda: HAND_STATES[state](kc, orc), np.random.default_rng([len(state), ROWS.index(row)]), state)
    torch.cuda.synchronize()  # the wrapped tensor is freed after the library has read it
    kc.sync()


# ------------------------------------------------------------------ one count of resident planes for every exporter
def _export_states(kc, orc, w, h):
    """-> [(name, SlotImage, the oracle's image, the distinct resident planes among channels 0-3, among channels 0-1)]"""
    p = [splitmix_plane(SEED_A, 40 + c, h, w) * np.float32(1.2) - np.float32(0.1) for c in range(4)]
    p[0][0, :3] = [np.nan, np.inf, -0.0]
    zero, one = np.zeros((h, w), np.float32), np.ones((h, w), np.float32)
    g = kc.SlotImage.from_planes([p[0]])
    return [("four planes", kc.SlotImage.from_planes(p), orc.Image(p), 4, 2),
            ("one plane in four channels", kc.combine_rgba_process([g, g, g, g]), orc.Image([p[0]] * 4), 1, 1),
            ("one plane as R and A, G and B constant", kc.combine_rgba_process([g, None, None, g]), orc.Image([p[0], zero, zero, p[0]]), 1, 1),
            ("R and G constant, one plane as B and A", kc.combine_rgba_process([None, None, g, g]), orc.Image([zero, zero, p[0], p[0]]), 1, 0),
            ("gray", g, orc.Image([p[0]]), 1, 1),
            ("constant", kc.SlotImage.from_value((w, h), 0.25, True), orc.Image([one * np.float32(0.25)] * 3 + [one]), 0, 0)]


@pytest.mark.parametrize("w,h", [(12, 8), (7, 5)])
def test_exporters_count_distinct_resident_planes(kc, orc, torch, w, h):
    """to_u8, to_torch to U8 and the u8 pipe's download read an image as to_bc does: a plane that sits in several channels is
    loaded and counted once, a constant channel not at all.  On a forced image each call is one launch and
    4 * w * h * (distinct resident planes among the channels written) + (bytes written) algorithmic bytes -- also where no
    channel written is resident and the launch reads nothing -- and BC3, which reads all four channels, counts the same planes."""
    pipe = kc.U8Pipe(w, h, 4, depth=1)
    try:
        for name, img, image, d4, d2 in _export_states(kc, orc, w, h):
            def download(img=img):
                pipe.download(0, img)
                return pipe.wait_download(0).copy()
            px, px_srgb = orc.to_u8(image), orc.to_u8(image, True)
            calls = [("to_u8", lambda img=img: img.to_u8(), px, d4, 4),
                     ("to_u8 srgb", lambda img=img: img.to_u8(True), px_srgb, d4, 4),
                     ("to_torch 4 channels", lambda img=img: img.to_torch(torch.uint8, channels=4).cpu().numpy(), px, d4, 4),
                     ("to_torch 2 channels", lambda img=img: img.to_torch(torch.uint8, channels=2).cpu().numpy(), np.ascontiguousarray(px[:, :, :2]), d2, 2),
                     ("pipe download", download, px, d4, 4),
                     ("to_bc bc3", lambda img=img: img.to_bc("bc3"), _ref_blocks(orc, image, 3, False), d4, None)]
            for call_name, call, want, distinct, channels in calls:
                what = "%d x %d, %s, %s" % (w, h, name, call_name)
                _same(call(), want, what)  # nothing is left to force after it
                got, launches, nbytes = _counted(kc, call)
                _same(got, want, what + ", second call")
                written = ((w + 3) // 4) * ((h + 3) // 4) * BLOCK_BYTES[3] if channels is None else w * h * channels
                _check_cost(launches, nbytes, (1, 4 * w * h * distinct + written), what)
    finally:
        pipe.close()


# ------------------------------------------------------------------ the coverage
def test_every_row_met_every_state():
    """Runs after the seed tests of this file.  A condition, not a measurement: the seed base was chosen so that it holds under
    the oracle alone."""
    if len(_RAN) < SEEDS:
        pytest.skip("only meaningful after all %d seed tests of this module have run (%d did)" % (SEEDS, len(_RAN)))
    skipped = sum(v == "skipped" for v in _RAN.values())
    assert 4 * skipped <= SEEDS, "%d of %d seeds skipped: the reference refuses their requested nodes" % (skipped, SEEDS)
    missing = [(row, st) for row in ROWS for st in STATES if (row, st) not in _TALLY]
    assert not missing, "never reached: %s" % missing
