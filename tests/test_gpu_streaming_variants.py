"""GPU parity of every launch variant of the streaming kernels (csrc/h2n.hip, u8.hip, devimage.hip, stats.hip, mip.hip) at
the smallest sizes that select them: every case is ONE launch of the kernel under test, the counters of its family
(kc_stats_counter) show which form ran -- each case asserts the whole vector, 0 where it does not name a counter -- and the
result equals the reference bit for bit: the CPU oracle for HeightToNormal and the u8 boundary, numpy / torch-on-CPU
conversions for device images, numpy for the statistics, tests/mip_ref.py for the mip chains.

The forms are selected through the options a launch reads: cache_budget_mb = 0 marks the inputs and results of every launch
nontemporal (runtime.cpp, cache_policy_mask), tune_cap caps the grid of the grid-stride loops, h2n_tiled = 0 turns the tiled
HeightToNormal mapping off.  Options are process-wide: every case restores what it set, the module fixture restores them
again, and the last test reads them back."""
import contextlib
import ctypes as C
import json

import numpy as np
import pytest

from golden_graphs import G
from test_gpu_channel_stats import check as check_stats, edge_rgba
from test_gpu_device_image import edge_planes, expected_f32, rgba_rule, source_values, srgb_threshold_values, u16_formula
from test_gpu_mips import check_levels, plane_const, ref_chain, special_planes
from util import SEED_A, SEED_B, assert_planes, splitmix_plane, with_edge_cases

pytestmark = pytest.mark.gpu

OPTIONS = ["cache_budget_mb", "nt_force", "tune_cap", "h2n_tiled"]
H2N = ["h2n_launches", "h2n_plain", "h2n_tiled_q5", "h2n_tiled_q6", "h2n_tiled_q7", "h2n_band", "h2n_nt"]
U8 = ["to_u8_nt", "from_u8_nt"]
IMPORT = ["image_import_vec", "image_import_scalar", "image_import_nt"]
EXPORT = ["image_export_vec", "image_export_scalar", "image_export_nt"]
STATS = ["stats_nt"]
MIPS = ["mip_pyramid", "mip_level", "mip_nt"]
_SAVED = {}


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    _SAVED.update({n: kc.get_option(n) for n in OPTIONS})
    try:
        yield kc
    finally:
        for n, v in _SAVED.items():
            kc.set_option(n, v)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@contextlib.contextmanager
def options(kc, opts):
    saved = {n: kc.get_option(n) for n in opts}
    try:
        for n, v in opts.items():
            kc.set_option(n, v)
        yield
    finally:
        for n, v in saved.items():
            kc.set_option(n, v)


def counted(kc, names, opts, call):
    """call() under the options `opts`: (its result, the counters of `names` that moved, kernel launches)"""
    with options(kc, opts):
        before = {n: kc.stats_counter(n) for n in names}
        l0 = kc.stats()["kernel_launches"]
        out = call()
        launches = kc.stats()["kernel_launches"] - l0
        seen = {n: kc.stats_counter(n) - before[n] for n in names if kc.stats_counter(n) != before[n]}
    return out, seen, launches


def ones(names):
    return {n: 1 for n in names}


JUNK = np.float32(-7.25)  # no kernel here stores it: results lie in [0, 1] or are conversions of other data


def scrub_planes(kc, w, h):
    """Before a case whose result planes come from the pool: the pool's free lists match sizes exactly, so a launch would get
    back the planes of the previous case -- which hold this very result already, and a store that never happens would go
    unseen.  Afterwards the only free w x h planes hold JUNK."""
    kc.pool_trim()
    junk = np.full((h, w), JUNK, np.float32)
    img = kc.SlotImage.from_planes([junk, junk, junk, junk])
    img.materialize()
    del img


def scrub_staging(kc, junk_img):
    """The same for the staging block of to_u8 (w * h * 4 bytes, taken from the pool and freed by every call): afterwards it holds
    the bytes of `junk_img`, an image of the same size."""
    kc.pool_trim()
    junk_img.to_u8(False)


# ------------------------------------------------------------------ HeightToNormal
H2N_EDGE = [np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0, 1e-40]  # test_height_to_normal's
# (w, h) -> the tile width (log2 of its column quads) the launcher picks at default options, 0: the plain mapping
H2N_SHAPES = [((130, 13), 5), ((262, 7), 6), ((517, 5), 7), ((1024, 9), 5), ((2048, 3), 6), ((128, 1), 5), ((128, 2), 5),
              ((1, 3), 0), ((5, 1), 0)]
# (id, options, tiled?, nontemporal?)
H2N_OPTIONS = [("default", {}, True, False), ("plain", {"h2n_tiled": 0}, False, False), ("nt", {"cache_budget_mb": 0}, True, True),
               ("plain_cap2", {"h2n_tiled": 0, "tune_cap": 2}, False, False)]


def h2n_counters(tq, band=False, nt=False):
    names = ["h2n_launches", "h2n_tiled_q%d" % tq if tq else "h2n_plain"] + (["h2n_band"] if band else []) + (["h2n_nt"] if nt else [])
    return ones(names)


def height_plane(w, h):
    """Heights in [0, 1) with the IEEE edge values on a third of the crossings of the first and last quad's columns and the
    columns on both sides of every tile edge (32, 64, 128 quads) with the first and last rows and the rows on both sides of
    every row-group edge (2, 4, 8 rows)."""
    p = splitmix_plane(SEED_A, 2, h, w)
    cols = set(range(min(4, w))) | set(range(max(0, w - 4), w)) | {e + d for e in range(128, w, 128) for d in (-1, 0)}
    rows = {0, 1, h - 2, h - 1} | {e + d for e in range(2, h, 2) for d in (-1, 0)}
    k = 0
    for i, y in enumerate(sorted(r for r in rows if 0 <= r < h)):
        for j, x in enumerate(sorted(cols)):
            if (i + j) % 3 == 0:
                p[y, x] = H2N_EDGE[k % len(H2N_EDGE)]
                k += 1
    return p


_H2N_REF = {}


def h2n_ref(orc, key, plane):
    """orc.height_to_normal of a plane plus the ones plane, computed once per key and shared read-only"""
    if key not in _H2N_REF:
        ref = list(orc.height_to_normal(plane)) + [np.ones_like(plane)]
        for r in ref:
            r.setflags(write=False)
        _H2N_REF[key] = ref
    return _H2N_REF[key]


def assert_alpha_is_constant_one(img):
    from kanter_core_amd import _lib
    is_const, value, _ = plane_const(_lib.load(), img, 3)
    assert is_const and value == np.float32(1.0)


@pytest.mark.parametrize("shape,tq", H2N_SHAPES, ids=["%dx%d" % s for s, _ in H2N_SHAPES])
def test_h2n_mappings(kc, orc, shape, tq):
    w, h = shape
    p = height_plane(w, h)
    want = h2n_ref(orc, shape, p)
    src = kc.SlotImage.from_planes([p])
    for name, opts, tiled, nt in H2N_OPTIONS:
        scrub_planes(kc, w, h)
        got, seen, launches = counted(kc, H2N, opts, lambda: kc.height_to_normal_process(src))
        what = "h2n %dx%d %s" % (w, h, name)
        assert launches == 1 and seen == h2n_counters(tq if tiled else 0, nt=nt), "%s: %d launches, counters %s" % (what, launches, seen)
        assert_planes(got.planes(), want, ulp=0, what=what)
        assert_alpha_is_constant_one(got)


@pytest.mark.parametrize("shape,tq", [((130, 13), 5), ((517, 9), 7)], ids=["130x13", "517x9"])
def test_h2n_bands(kc, orc, shape, tq):
    """Row bands of a live graph (an embedded plane -> HeightToNormal): the BAND forms, tiled, plain stores and nontemporal."""
    w, h = shape
    p = height_plane(w, h)
    want = h2n_ref(orc, shape, p)
    g = G()
    e = g.add({"Embed": 0})
    sep = g.add("SeparateRgba")
    g.connect(e, sep, 0, 0)
    node = g.add("HeightToNormal")
    g.connect(sep, node, 0, 0)
    zero = np.zeros_like(p)
    for name, opts, nt in (("default", {}, False), ("nt", {"cache_budget_mb": 0}, True)):
        for y0, y1 in ((0, 5), (5, 6), (6, h)):
            tp = kc.TextureProcessor.new()
            lg = tp.new_live_graph()
            lg.set_node_graph(kc.NodeGraph.from_json(json.dumps(g.dict())))
            lg.embed_slot_data_with_id(kc.SlotData(0, 0, kc.SlotImage.from_planes([p, zero, zero, zero])), 0)
            scrub_planes(kc, w, y1 - y0)
            got, seen, launches = counted(kc, H2N, opts, lambda: lg.evaluate_band(node, y0, y1))
            what = "h2n band %d:%d of %dx%d %s" % (y0, y1, w, h, name)
            assert launches >= 1 and seen == h2n_counters(tq, band=True, nt=nt), "%s: counters %s" % (what, seen)
            assert_planes(got.planes(), [r[y0:y1] for r in want], ulp=0, what=what)


def test_h2n_wrapped_input_with_a_tight_pitch(kc, orc, torch):
    """A caller-owned plane 130 wide with rows 528 bytes apart: the last quad's 16-byte load reads the two floats of padding
    (NaN and 3e38 here), which must not reach a pixel inside the width, and the tensor is only read."""
    from kanter_core_amd import _lib
    L = _lib.load()
    w, h, pitch_f = 130, 13, 132
    p = height_plane(w, h)
    host = np.empty((h, pitch_f), np.float32)
    host[:, :w] = p
    host[:, w] = np.nan
    host[:, w + 1] = 3e38
    t = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    plane, img = C.c_void_p(), C.c_void_p()
    assert L.kc_plane_wrap(t.data_ptr(), w, h, pitch_f * 4, C.byref(plane)) == 0
    assert L.kc_image_gray(plane, C.byref(img)) == 0
    src = kc.SlotImage(img.value)
    want = h2n_ref(orc, (w, h), p)
    for name, opts, tiled, nt in H2N_OPTIONS:
        scrub_planes(kc, w, h)
        got, seen, launches = counted(kc, H2N, opts, lambda: kc.height_to_normal_process(src))
        assert launches == 1 and seen == h2n_counters(5 if tiled else 0, nt=nt), "wrapped %s: counters %s" % (name, seen)
        assert_planes(got.planes(), want, ulp=0, what="h2n wrapped %s" % name)
    kc.sync()
    assert np.array_equal(t.cpu().numpy().view(np.uint32), host.view(np.uint32))
    del src
    L.kc_plane_release(plane)


def exact_steps(n):
    """n height steps: 0, both bounds of the kernel's exact range (2^-40 and 2^7) and their neighbours outside it, each sign,
    eight of each in a row (a quad then holds no other step), then random mantissas at exponents -40 .. 7, and the special
    values again at the end (the last quads of a row)."""
    lo, hi = np.float32(2.0 ** -40), np.float32(2.0 ** 7)
    special = [np.float32(0), lo, -lo, np.nextafter(lo, np.float32(0)), -np.nextafter(lo, np.float32(0)), hi, -hi,
               np.nextafter(hi, np.float32(np.inf)), -np.nextafter(hi, np.float32(np.inf))]
    head = np.repeat(np.array(special, np.float32), 8)
    rng = np.random.default_rng(65535)
    m = rng.integers(0, 1 << 23, n).astype(np.uint32)
    e = rng.integers(-40, 8, n).astype(np.int64)
    s = rng.integers(0, 2, n).astype(np.uint32)
    steps = ((s << 31) | ((e + 127).astype(np.uint32) << 23) | m).view(np.float32)
    steps[:len(head)] = head
    steps[n - len(head):] = head[::-1]
    return steps


@pytest.mark.parametrize("shape,tq", [((65535, 3), 7), ((5, 65535), 0)], ids=["65535x3", "5x65535"])
def test_h2n_edge_of_the_exact_arithmetic(kc, orc, shape, tq):
    """h2n.hip's shared-denominator division and sqrt_normal are exact for extents up to 65535 and height steps of 0 or
    within [2^-40, 2^7]; outside that range a quad takes the general path.  Here the steps px - left and up - px ARE the
    chosen values (the plane alternates 0 and the step along the long axis, and repeats the line, 0, the line across the
    short one, so every difference is x - 0, 0 - x or x - x): both bounds, their neighbours outside, 0 and random mantissas
    at every exponent in between, with 1 / 65535 as the other component.  Only one extent can be extreme at a time in an
    image that fits a test: 65535 x 3 (tiled, 128-quad tiles) and 5 x 65535 (plain)."""
    w, h = shape
    n = max(w, h)
    line = np.zeros(n, np.float32)
    line[1::2] = exact_steps(n // 2)
    if w > h:
        p = np.stack([line, np.zeros(n, np.float32), line])
    else:
        z = np.zeros(n, np.float32)
        p = np.stack([line, z, line, z, line], axis=1)
    p = np.ascontiguousarray(p)
    assert p.shape == (h, w)
    lo, hi = np.float32(2.0 ** -40), np.float32(2.0 ** 7)
    tz, bz = p - np.roll(p, 1, axis=1), np.roll(p, 1, axis=0) - p
    line_steps = np.abs(line[1::2])
    for d in (tz, bz):  # both sides of both bounds, exactly, and exactly the chosen steps
        a = np.abs(d)
        for v in (np.float32(0), lo, np.nextafter(lo, np.float32(0)), hi, np.nextafter(hi, np.float32(np.inf))):
            assert (a == v).any(), v
        assert set(np.unique(a)) == set(np.unique(line_steps)) | {np.float32(0)}
    assert ((line_steps > np.float32(0)) & (line_steps < lo)).any() and (line_steps > hi).any()
    want = h2n_ref(orc, ("exact",) + shape, p)
    src = kc.SlotImage.from_planes([p])
    for name, opts, nt in (("default", {}, False), ("nt", {"cache_budget_mb": 0}, True)):
        scrub_planes(kc, w, h)
        got, seen, launches = counted(kc, H2N, opts, lambda: kc.height_to_normal_process(src))
        assert launches == 1 and seen == h2n_counters(tq, nt=nt), "exact %s: counters %s" % (name, seen)
        assert_planes(got.planes(), want, ulp=0, what="h2n exact range %dx%d %s" % (w, h, name))


# ------------------------------------------------------------------ the u8 boundary
# (id, options, nontemporal?)
U8_OPTIONS = [("default", {}, False), ("nt", {"cache_budget_mb": 0}, True), ("cap1", {"tune_cap": 1}, False),
              ("cap3_nt", {"tune_cap": 3, "cache_budget_mb": 0}, True)]


def u8_planes(h, w):
    """edge_planes, with as many of the sRGB threshold floats as half a small plane holds (another part of them per channel)"""
    planes = edge_planes(h, w)
    thr = srgb_threshold_values()
    for c in range(3):
        flat = planes[c].reshape(-1)
        if flat.size < 2 * len(thr):
            k = flat.size // 2
            flat[-k:] = np.roll(thr, 207 * c)[:k]
    return planes


# (64, 9): 144 quads, one workgroup with out-of-range threads at the sRGB barrier; (128, 33): 1056 quads, a grid of 3 loops;
# (13, 7): the scalar stores of a width that is no multiple of 4
@pytest.mark.parametrize("shape", [(64, 9), (128, 33), (13, 7)], ids=lambda s: "%dx%d" % s)
def test_to_u8_forms(kc, orc, shape):
    w, h = shape
    planes = u8_planes(h, w)
    one = np.ones((h, w), np.float32)
    half = np.full((h, w), 0.5, np.float32)
    junk_img = kc.SlotImage.from_planes([half, half, half, half])  # 127 in every byte, linear
    gray = [kc.SlotImage.from_planes([planes[c]]) for c in range(3)]
    images = [("rgba", kc.SlotImage.from_planes(planes), planes), ("gray", gray[0], planes[:1]),
              ("const_alpha", kc.combine_rgba_process(gray + [None]), planes[:3] + [one])]
    for kind, img, ref_planes in images:
        if kind == "const_alpha":
            assert_alpha_is_constant_one(img)
        for srgb in (False, True):
            want = orc.to_u8(orc.Image(ref_planes), srgb)
            for name, opts, nt in U8_OPTIONS:
                scrub_staging(kc, junk_img)
                got, seen, launches = counted(kc, U8, opts, lambda: img.to_u8(srgb))
                what = "to_u8 %dx%d %s srgb=%s %s" % (w, h, kind, srgb, name)
                assert launches == 1 and seen == (ones(["to_u8_nt"]) if nt else {}), "%s: %d launches, counters %s" % (what, launches, seen)
                assert np.array_equal(got, want), what


@pytest.mark.parametrize("shape", [(33, 17), (128, 33)], ids=lambda s: "%dx%d" % s)
def test_from_u8_forms(kc, orc, shape):
    w, h = shape
    for channels in (1, 2, 3, 4):
        px = np.random.default_rng([w, h, channels]).integers(0, 256, size=(h, w, channels), dtype=np.uint8)
        px.reshape(-1)[:4] = [0, 255, 1, 254]
        want = orc.deconstruct_u8(px)
        for name, opts, nt in U8_OPTIONS:
            scrub_planes(kc, w, h)
            got, seen, launches = counted(kc, U8, opts, lambda: kc.SlotImage.from_u8(px))
            what = "from_u8 %dx%d x%d %s" % (w, h, channels, name)
            assert launches == 1 and seen == (ones(["from_u8_nt"]) if nt else {}), "%s: %d launches, counters %s" % (what, launches, seen)
            assert_planes(got.planes(), want, what=what)


# ------------------------------------------------------------------ device images
DTYPES = ["uint8", "uint16", "float16", "bfloat16", "float32"]
ESIZE = {"uint8": 1, "uint16": 2, "float16": 2, "bfloat16": 2, "float32": 4}
BITS = {1: np.uint8, 2: np.uint16, 4: np.uint32}
DT_CODE = {"uint8": 0, "uint16": 1, "float16": 2, "bfloat16": 3, "float32": 4}
DEV_W, ALLOC_W = 70, 80  # every row ends in a partial quad; 80 elements keep every pitch a multiple of 16 bytes
# 9 rows: 162 quads, one workgroup; 33 rows: 594 quads, three workgroups, or two that loop under tune_cap = 2
DEV_HEIGHTS = [9, 33]
DEV_OPTIONS = [("default", {}, False), ("nt_cap2", {"cache_budget_mb": 0, "tune_cap": 2}, True)]


def geometry(name, layout, channels, h, aligned):
    """(offset, shape, strides, elements) of a DEV_W x h image inside a flat buffer, in elements.  aligned: rows of an
    allocation ALLOC_W pixels wide from its start -- every pitch a multiple of 16 bytes.  Otherwise the same rows one pixel
    in, which the access unit of the layout (devimage.cpp, devimage_args) does not divide -- or one ELEMENT in where a
    pixel is a whole unit (4-channel f32 pixels are 16 bytes)."""
    if layout == "hwc":
        shape, strides = (h, DEV_W, channels), (ALLOC_W * channels, channels, 1)
        offset = 0 if aligned else 1 if channels * ESIZE[name] % 16 == 0 else channels
    else:
        shape, strides = (channels, h, DEV_W), ((h + 1) * ALLOC_W, ALLOC_W, 1)  # a row of gap between the planes
        offset = 0 if aligned else 1
    need = offset + sum((n - 1) * s for n, s in zip(shape, strides)) + 1
    return offset, shape, strides, need + 19


def np_view(flat, geo):
    offset, shape, strides, _ = geo
    return np.lib.stride_tricks.as_strided(flat[offset:], shape, tuple(s * flat.itemsize for s in strides))


def is_nan_bits(name, bits):
    if name == "float16":
        return (bits & 0x7fff) > 0x7c00
    if name == "bfloat16":
        return (bits & 0x7fff) > 0x7f80
    return np.zeros(bits.shape, bool)  # integers have none; f32 is moved by its bits, payloads included


def bits_to_torch(torch, name, bits):
    """A flat array of bit patterns as a CPU tensor of the element type"""
    if name in ("uint8", "uint16"):
        return torch.from_numpy(bits)
    if name == "float32":
        return torch.from_numpy(bits.view(np.float32))
    return torch.from_numpy(bits.view(np.int16)).view(getattr(torch, name))


def torch_to_bits(torch, name, t):
    t = t.cpu()
    if name in ("uint8", "uint16"):
        return t.numpy()
    if name == "float32":
        return t.numpy().view(np.uint32)
    return t.view(torch.int16).numpy().view(np.uint16)


def by_hand(kc, torch, name, layout, channels, h, geo, flat, call):
    """The conversion through a kc_device_image filled in here from the flat buffer's address, not from a tensor view."""
    from kanter_core_amd import _lib
    offset, shape, strides, _ = geo
    e = ESIZE[name]
    row = (strides[0] if layout == "hwc" else strides[1]) * e
    chan = strides[0] * e if layout == "chw" else 0
    d = _lib.kc_device_image(flat.data_ptr() + offset * e, DEV_W, h, channels, DT_CODE[name], 0 if layout == "hwc" else 1, row, chan)
    torch.cuda.synchronize()  # no stream is handed over: the buffer is ready now, and read after kc.sync()
    out = call(_lib.load(), C.byref(d))
    kc.sync()
    return out


@pytest.mark.parametrize("name", DTYPES)
def test_device_import_forms(kc, orc, torch, name):
    """Every import form of one element type: layout x channels x aligned / misaligned descriptor x plain / nontemporal with
    a capped grid.  The counters say which access path ran, and both paths give the same planes."""
    for layout, channels, h in [(l, c, h) for l in ("hwc", "chw") for c in (1, 2, 3, 4) for h in DEV_HEIGHTS]:
        rng = np.random.default_rng([ESIZE[name], len(name), channels, h, layout == "hwc"])
        planes_of = {}
        for aligned in (True, False):
            geo = geometry(name, layout, channels, h, aligned)
            offset, shape, strides, n = geo
            src = rng.integers(0, 256, n, dtype=np.uint8) if name == "uint8" else source_values(torch, name, (n,), rng)
            host = torch.from_numpy(src) if name == "uint8" else src
            hview = torch.as_strided(host, shape, strides, offset)
            if aligned:
                first = hview.clone()  # the misaligned case holds the same pixels
            else:
                hview.copy_(first)
            chans = [(hview[:, :, c] if layout == "hwc" else hview[c]).contiguous() for c in range(channels)]
            if name == "uint8":
                want = orc.deconstruct_u8(np.stack([c.numpy() for c in chans], 2))
            else:
                want = rgba_rule([expected_f32(torch, name, c) for c in chans], h, DEV_W)
            dev = host.cuda()
            dview = torch.as_strided(dev, shape, strides, offset)
            hand = not aligned and layout == "hwc" and channels * ESIZE[name] % 16 == 0  # no tensor view breaks that alignment

            def run():
                if not hand:
                    return kc.SlotImage.from_torch(dview, layout=layout)
                out = C.c_void_p()
                assert by_hand(kc, torch, name, layout, channels, h, geo, dev, lambda L, d: L.kc_image_from_device(d, 0, None, C.byref(out))) == 0
                return kc.SlotImage(out.value)

            for oname, opts, nt in DEV_OPTIONS:
                scrub_planes(kc, DEV_W, h)
                img, seen, launches = counted(kc, IMPORT, opts, run)
                what = "import %s %s x%d h=%d %s %s" % (name, layout, channels, h, "aligned" if aligned else "misaligned", oname)
                expect = ones(["image_import_vec" if aligned else "image_import_scalar"] + (["image_import_nt"] if nt else []))
                assert launches == 1 and seen == expect, "%s: %d launches, counters %s" % (what, launches, seen)
                got = img.planes()
                if name == "float32":  # the bits as they are
                    for c in range(4):
                        assert np.array_equal(got[c].view(np.uint32), want[c].view(np.uint32)), (what, c)
                else:
                    assert_planes(got, want, what=what)
                planes_of[(aligned, oname)] = got
        for oname, _, _ in DEV_OPTIONS:
            for c in range(4):
                assert np.array_equal(planes_of[(True, oname)][c].view(np.uint32), planes_of[(False, oname)][c].view(np.uint32))


_EXPORT_SRC = {}


def export_source(kc, h):
    """(planes, RGBA image, gray image of plane 0) of the export cases, built once per height"""
    if h not in _EXPORT_SRC:
        planes = edge_planes(h, DEV_W)
        planes[0].reshape(-1)[100:104] = [65504.0, 65520.0, 1e-8, 3.0e38]  # f16 overflow / rounding, bf16 range
        _EXPORT_SRC[h] = (planes, kc.SlotImage.from_planes(planes), kc.SlotImage.from_planes([planes[0]]))
    return _EXPORT_SRC[h]


def export_bits(orc, torch, name, planes, srgb):
    """What an export of the 4 planes holds, as (h, w, 4) bit patterns"""
    if name == "uint8":
        return orc.to_u8(orc.Image(list(planes)), srgb)  # alpha stays linear
    ref = np.stack(planes, 2)
    if name == "uint16":
        return u16_formula(ref)
    if name == "float32":
        return ref.view(np.uint32)
    return torch.from_numpy(ref).to(getattr(torch, name)).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("name", DTYPES)
def test_device_export_forms(kc, orc, torch, name):
    """Every export form of one element type, into a buffer of sentinel bytes: only the described elements change -- not the
    row padding, not the gap between planes, not the bytes before a misaligned start."""
    e = ESIZE[name]
    cases = [(layout, channels, h, False) for layout in ("hwc", "chw") for channels in (1, 2, 3, 4) for h in DEV_HEIGHTS]
    cases.append(("hwc", 4, DEV_HEIGHTS[0], True))  # a Gray image, once: (v, v, v, 1)
    for layout, channels, h, gray in cases:
        planes, rgba, gimg = export_source(kc, h)
        img = gimg if gray else rgba
        ref_planes = [planes[0], planes[0], planes[0], np.ones_like(planes[0])] if gray else planes
        for srgb in ((False, True) if name == "uint8" else (False,)):
            full = export_bits(orc, torch, name, ref_planes, srgb)[:, :, :channels]
            want = full if layout == "hwc" else full.transpose(2, 0, 1)
            for aligned in (True, False):
                geo = geometry(name, layout, channels, h, aligned)
                offset, shape, strides, n = geo
                expect_flat = np.full(n, 0x47, np.uint8).repeat(e).view(BITS[e]).copy()
                sentinel = expect_flat.copy()
                np_view(expect_flat, geo)[...] = want
                hand = not aligned and layout == "hwc" and channels * e % 16 == 0  # no tensor view breaks that alignment
                for oname, opts, nt in DEV_OPTIONS:
                    dev = bits_to_torch(torch, name, sentinel.copy()).cuda()
                    dview = torch.as_strided(dev, shape, strides, offset)

                    def run():
                        if not hand:
                            return img.to_torch(layout=layout, srgb=srgb, out=dview)
                        flags = kc.DEVICE_SRGB if srgb else 0
                        assert by_hand(kc, torch, name, layout, channels, h, geo, dev, lambda L, d: L.kc_image_to_device(img._h, d, flags, None)) == 0

                    _, seen, launches = counted(kc, EXPORT, opts, run)
                    what = "export %s %s x%d h=%d%s srgb=%s %s %s" % (name, layout, channels, h, " gray" if gray else "", srgb,
                                                                    "aligned" if aligned else "misaligned", oname)
                    expect = ones(["image_export_vec" if aligned else "image_export_scalar"] + (["image_export_nt"] if nt else []))
                    assert launches == 1 and seen == expect, "%s: %d launches, counters %s" % (what, launches, seen)
                    got = torch_to_bits(torch, name, dev)
                    gn, wn = is_nan_bits(name, got), is_nan_bits(name, expect_flat)
                    assert np.array_equal(gn, wn), what
                    assert np.array_equal(got[~gn], expect_flat[~wn]), what


# ------------------------------------------------------------------ statistics and mips
@pytest.mark.parametrize("rgba", [False, True], ids=["gray", "rgba"])
@pytest.mark.parametrize("mode", ["minmax", "hist", "srgb"])
def test_channel_stats_forms(kc, orc, mode, rgba):
    h, w = 33, 4097  # test_gpu_channel_stats.py's ragged size and inputs
    planes = edge_rgba(h, w) if rgba else [with_edge_cases(splitmix_plane(SEED_B, 0, h, w) * 1.5 - 0.2, shift=3)]
    img = kc.SlotImage.from_planes(planes)
    # nontemporal loads; two workgroups that loop some 66 times each.  No counter shows the loop: the cap2 leg is pinned by the
    # numpy comparison alone (min, max, NaN counts and bins of the whole plane).  check_stats also calls to_u8 for its bins, inside
    # the window: it moves none of STATS.
    for name, opts, nt in (("nt", {"cache_budget_mb": 0}, True), ("cap2", {"tune_cap": 2}, False)):
        _, seen, _ = counted(kc, STATS, opts, lambda: check_stats(kc, orc, img, planes, histogram=mode != "minmax", srgb=mode == "srgb"))
        assert seen == (ones(STATS) if nt else {}), "stats %s %s: counters %s" % (mode, name, seen)


@pytest.mark.parametrize("shape", [(130, 70), (320, 192), (1, 5)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("n", [1, 4], ids=["gray", "rgba"])
def test_mip_forms(kc, shape, n):
    w, h = shape
    planes = special_planes(w, h, n)
    refs = [ref_chain((("special", w, h), c), p) for c, p in enumerate(planes)]
    img = kc.SlotImage.from_planes(planes)
    levels = len(refs[0])
    for per_level in (False, True):
        for name, opts, nt in (("nt", {"cache_budget_mb": 0}, True), ("default", {}, False)):
            got, seen, launches = counted(kc, MIPS, opts, lambda: img.mips(per_level=per_level))
            what = "mips %dx%d x%d per_level=%s %s" % (w, h, n, per_level, name)
            forms = seen.get("mip_pyramid", 0) + seen.get("mip_level", 0)
            assert launches == forms > 0 and seen.get("mip_nt", 0) == (launches if nt else 0), "%s: %d launches, counters %s" % (what, launches, seen)
            if per_level:
                assert seen == dict(mip_level=levels - 1, **({"mip_nt": levels - 1} if nt else {})), (what, seen)
            else:
                assert ("mip_pyramid" in seen) == (min(w, h) >= 2), (what, seen)
            check_levels(got, refs, what)


# ------------------------------------------------------------------ the options are as they were
def test_options_are_back_at_their_defaults(kc):
    assert {n: kc.get_option(n) for n in OPTIONS} == _SAVED
    import os
    if not any("KC_" + n.upper() in os.environ for n in OPTIONS):
        assert _SAVED == {"cache_budget_mb": 208, "nt_force": -1, "tune_cap": 0, "h2n_tiled": -1}
