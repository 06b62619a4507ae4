"""Previews on the device (kc_image_previews and its forms, csrc/preview.*): the bytes of every request equal the CPU oracle's
to_u8 of tests/mip_ref.py's level, cut to the rect, byte for byte -- and every other byte of the 0xA5-filled output buffer stays
0xA5.  The sizes are those at which each part of the kernel can go wrong: one tile, partial tiles with odd levels, rects off the
origin at every x % 4, a second pass through the f32 scratch (one and two tiles wide), the levels after one extent has reached 1
(the fallback through the chain), a batch of mixed images and levels in one launch.  Gray and RGBA, constant and aliased planes,
a pending Mix chain, a wrapped tensor with a tight pitch, IEEE special values, sRGB; the device, live-graph and SlotImage forms;
launch and byte counts; the refusals."""
import ctypes as C
import json

import numpy as np
import pytest

import mip_ref
from util import SEED_A, SEED_B, synthetic_rgba, wrapped_image

pytestmark = pytest.mark.gpu

KC_ERR_NO_SLOT_DATA, KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 10, 102, 104
PREVIEW_SRGB = 1
FLT_MAX = np.finfo(np.float32).max
SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 5.877e-39, 1.1754942e-38, FLT_MAX, -FLT_MAX, 3e38],
                    np.float32)


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    return kc


@pytest.fixture(scope="module")
def L():
    from kanter_core_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def random_planes(w, h, n, seed=SEED_A):
    return synthetic_rgba(seed, h, w)[:n]  # [0, 1)


def special_plane(w, h, seed):
    """test_gpu_mips.py's generator: random data with special values scattered over a tenth of the texels and filling whole
    aligned 2 x 2 quads and 4 x 4 blocks (so that they survive, unmixed, into levels 1 and 2)."""
    rng = np.random.default_rng([seed, w, h])
    p = rng.random((h, w), dtype=np.float32)
    hit = rng.random((h, w)) < 0.1
    p[hit] = SPECIALS[rng.integers(0, len(SPECIALS), size=int(hit.sum()))]
    for i in range(min(64, (h // 2) * (w // 2))):
        y, x = 2 * int(rng.integers(0, h // 2)), 2 * int(rng.integers(0, w // 2))
        p[y:y + 2, x:x + 2] = SPECIALS[i % len(SPECIALS)]
    for i in range(min(24, (h // 4) * (w // 4))):
        y, x = 4 * int(rng.integers(0, h // 4)), 4 * int(rng.integers(0, w // 4))
        p[y:y + 4, x:x + 4] = SPECIALS[(5 * i + 1) % len(SPECIALS)]
    return p


def const_fold(c, k):
    c = np.float32(c)
    with np.errstate(all="ignore"):
        for _ in range(k):
            c = ((c + c) + (c + c)) * np.float32(0.25)
    return c


class Src:
    """An image on the device and what its channels hold (a plane, or a float for a constant channel): the reference of any
    level, computed once and shared."""

    def __init__(self, img, channels, size=None):
        self.img, self.channels = img, channels
        self.w, self.h = size if size else channels[0].shape[::-1]
        self.planes = sum(1 for c in channels if isinstance(c, np.ndarray))  # before aliases are counted once
        self._chain, self._want = {}, {}

    def levels(self):
        return mip_ref.level_count(self.w, self.h)

    def level_planes(self, k):
        lw, lh = mip_ref.level_size(self.w, self.h, k)
        out = []
        for i, c in enumerate(self.channels):
            if isinstance(c, np.ndarray):
                if i not in self._chain:
                    self._chain[i] = mip_ref.chain(c)
                out.append(self._chain[i][k])
            else:
                out.append(np.full((lh, lw), const_fold(c, k), np.float32))
        return out

    def want(self, orc, k, srgb, rect=None):
        if (k, srgb) not in self._want:
            full = orc.to_u8(orc.Image(self.level_planes(k)), srgb)
            full.setflags(write=False)
            self._want[(k, srgb)] = full
        full = self._want[(k, srgb)]
        if rect is None:
            return full
        x, y, w, h = rect
        return full[y:y + h, x:x + w]


def rgba_src(kc, w, h, seed=SEED_A, special=False):
    planes = [special_plane(w, h, 7 + c) for c in range(4)] if special else random_planes(w, h, 4, seed)
    return Src(kc.SlotImage.from_planes(planes), planes)


def gray_src(kc, w, h, seed=SEED_A, special=False):
    planes = [special_plane(w, h, 11)] if special else random_planes(w, h, 1, seed)
    return Src(kc.SlotImage.from_planes(planes), planes)


def whole(src, k):
    return (0, 0) + mip_ref.level_size(src.w, src.h, k)


def layout(items, gap=0, pitch_extra=0):
    """-> (kc_preview_request array, total bytes): the rects one after the other, `gap` bytes between them, rows pitch_extra
    bytes wider than the rect (an int, or one per item)."""
    from kanter_core_amd import _lib
    reqs = (_lib.kc_preview_request * len(items))()
    at = 0
    for i, (src, level, rect) in enumerate(items):
        x, y, w, h = rect if rect is not None else whole(src, level)
        extra = pitch_extra[i] if isinstance(pitch_extra, (list, tuple)) else pitch_extra
        pitch = 4 * w + extra
        reqs[i] = _lib.kc_preview_request(src.img._h if src.img is not None else None, level, x, y, w, h, at, pitch)
        at += pitch * (h - 1) + 4 * w + gap
    return reqs, at


def check_bytes(orc, items, reqs, buf, srgb):
    """Every request's bytes are the reference cut; everything else in `buf` is still 0xA5."""
    mask = np.zeros(buf.size, bool)
    for i, (src, level, rect) in enumerate(items):
        q = reqs[i]
        want = src.want(orc, level, srgb, (q.x, q.y, q.width, q.height))
        for row in range(q.height):
            o = q.offset_bytes + row * q.row_pitch_bytes
            got = buf[o:o + 4 * q.width].reshape(q.width, 4)
            assert np.array_equal(got, want[row]), "request %d (%dx%d level %d rect %s) row %d: %d texels differ" % (
                i, src.w, src.h, level, (q.x, q.y, q.width, q.height), row, int((got != want[row]).any(axis=1).sum()))
            mask[o:o + 4 * q.width] = True
    assert (buf[~mask] == 0xA5).all(), "%d bytes outside the rects were written" % int((buf[~mask] != 0xA5).sum())


def run(L, orc, items, srgb=False, gap=12, pitch_extra=0):
    reqs, total = layout(items, gap, pitch_extra)
    buf = np.full(total + 64, 0xA5, np.uint8)
    status = L.kc_image_previews(reqs, len(items), PREVIEW_SRGB if srgb else 0, buf.ctypes.data, buf.nbytes)
    assert status == 0, (status, L.kc_last_error())
    check_bytes(orc, items, reqs, buf, srgb)


def counters(kc):
    st = kc.stats()
    return dict(launches=st["kernel_launches"], bytes=st["algorithmic_bytes"], preview=kc.stats_counter("preview_launches"),
                fallback=kc.stats_counter("preview_fallback"))


def delta(kc, before):
    now = counters(kc)
    return {k: now[k] - before[k] for k in now}


# ------------------------------------------------------------------ the bits, by size
_SRC = {}


def shared(kc, key, make):
    if key not in _SRC:
        _SRC[key] = make()
    return _SRC[key]


@pytest.mark.parametrize("level", range(7))
def test_one_tile(kc, L, orc, level):
    src = shared(kc, "64x64", lambda: rgba_src(kc, 64, 64))
    lw, lh = mip_ref.level_size(64, 64, level)
    items = [(src, level, None)]
    if lw > 1:
        items.append((src, level, (1, 1, lw - 1, lh - 1)))
    c0 = counters(kc)
    run(L, orc, items)
    assert delta(kc, c0)["preview"] == 1 and delta(kc, c0)["fallback"] == 0


@pytest.mark.parametrize("level", range(7))
def test_partial_tiles_and_odd_levels(kc, L, orc, level):
    src = shared(kc, "130x70", lambda: rgba_src(kc, 130, 70))
    lw, lh = mip_ref.level_size(130, 70, level)  # 130x70, 65x35, 32x17, 16x8, 8x4, 4x2, 2x1
    items = [(src, level, None), (src, level, (lw - min(lw, 5), lh - min(lh, 3), min(lw, 5), min(lh, 3)))]  # ends on the last column and row
    for x in (1, 2, 3):
        for wd in (1, 3, 5):
            if x + wd <= lw and lh >= 2:
                items.append((src, level, (x, 1, wd, min(3, lh - 1))))
    if lw > 70:
        items.append((src, level, (61, 33, lw - 66, lh - 38)))  # across the tile boundary, off the origin
    extra = [8 if i % 2 else 0 for i in range(len(items))]  # every other request: rows wider than 4 * width
    c0 = counters(kc)
    run(L, orc, items, pitch_extra=extra)
    assert delta(kc, c0)["preview"] == 1 and delta(kc, c0)["fallback"] == 0


def test_second_pass(kc, L, orc):
    src = shared(kc, "256x256", lambda: rgba_src(kc, 256, 256, SEED_B))
    src.img.materialize()  # nothing pending: the launches below are the batch's own
    c0 = counters(kc)
    run(L, orc, [(src, 7, None), (src, 7, (1, 1, 1, 1)), (src, 8, None), (src, 7, (1, 0, 1, 2))], pitch_extra=[0, 4, 0, 0])
    d = delta(kc, c0)
    assert d["preview"] == 2 and d["launches"] == 2 and d["fallback"] == 0


def test_second_pass_two_tiles_wide(kc, L, orc):
    src = shared(kc, "8192x128", lambda: gray_src(kc, 8192, 128))
    c0 = counters(kc)
    run(L, orc, [(src, 7, (1, 0, 63, 1)), (src, 7, None)])  # level 7 is 64 x 1; the level-6 scratch 126 x 2 and 128 x 2
    assert delta(kc, c0)["preview"] == 2
    run(L, orc, [(src, 6, (3, 1, 120, 1)), (src, 1, (4000, 60, 96, 4)), (src, 0, (8101, 120, 91, 8))])


@pytest.mark.parametrize("w,h", [(1, 1), (1, 5), (5, 1), (64, 2)])
def test_fallback_after_an_extent_has_reached_one(kc, L, orc, w, h):
    """Every level of the shapes whose chains leave the fused ground, H = how often both extents halve: the requests with
    level > H take the fallback, one "preview_fallback" each, and the bytes are the reference's.  1 x 1 has level 0 alone, which is
    not past H = 0 and is read as it is; 64 x 2 is past H = 1 from level 2 on."""
    src = gray_src(kc, w, h) if w == 1 else rgba_src(kc, w, h)
    H = min(w.bit_length(), h.bit_length()) - 1
    items = [(src, k, None) for k in range(src.levels())]
    if (w, h) == (64, 2):
        items.append((src, 2, (5, 0, 7, 1)))
    src.img.materialize()
    c0 = counters(kc)
    src.img.mips()
    chain = delta(kc, c0)["launches"]  # what one chain of this image launches
    c0 = counters(kc)
    run(L, orc, items)
    d = delta(kc, c0)
    want = sum(1 for _, k, _ in items if k > H)  # 1 x 1 has level 0 alone, which is read as it is
    assert d["launches"] == (chain if want else 0) + 1  # one chain for the image, however many requests need it, and the batch
    assert d["fallback"] == want and (want > 0 or (w, h) == (1, 1))
    assert (w, h) != (64, 2) or want == 6  # levels 2 .. 6, and the rect of level 2


# ------------------------------------------------------------------ one batch, one launch
def tile_texels(size, level, rect):
    """The source texels a fused request reads per plane: its tiles, clipped to the image (level 0: the rect)."""
    (w, h), (x, y, rw, rh) = size, rect
    if level == 0:
        return rw * rh
    span = 64 >> level
    x0, x1, y0, y1 = x // span * 64, ((x + rw - 1) // span + 1) * 64, y // span * 64, ((y + rh - 1) // span + 1) * 64
    return (min(x1, w) - x0) * (min(y1, h) - y0)


def batch_bytes(items, distinct):
    """kc_stats_algorithmic_bytes of a batch of fused single-pass requests: 4 bytes per source texel read per distinct resident
    plane, 4 per texel written"""
    total = 0
    for (src, level, rect), n in zip(items, distinct):
        rect = rect if rect is not None else whole(src, level)
        total += 4 * n * tile_texels((src.w, src.h), level, rect) + 4 * rect[2] * rect[3]
    return total


@pytest.fixture(scope="module")
def mixed(kc, torch):
    """(items, distinct resident planes per item, the wrapped image): at least eight requests at mixed levels 0 .. 6"""
    w, h = 130, 70
    gray = gray_src(kc, 200, 100)
    p = random_planes(w, h, 3, SEED_B)
    const_alpha = Src(kc.combine_rgba_process([kc.SlotImage.from_planes([p[0]]), kc.SlotImage.from_planes([p[1]]), kc.SlotImage.from_planes([p[2]]),
                                               kc.SlotImage.from_value(kc.Size(w, h), 0.6, False)]), [p[0], p[1], p[2], 0.6])
    const = Src(kc.SlotImage.from_value(kc.Size(37, 21), 0.25, True), [0.25, 0.25, 0.25, 1.0], size=(37, 21))
    q = random_planes(64, 64, 1, SEED_B)[0]
    alias = Src(kc.SlotImage.from_planes([q]).materialize().as_type(True), [q, q, q, 1.0])  # [p, p, p, ones]
    wrapped = wrapped_image(kc, torch, [special_plane(100, 37, 3)], "tight", guard=np.nan)
    wsrc = Src(wrapped.image, wrapped.planes)
    wrapped4 = wrapped_image(kc, torch, random_planes(67, 45, 4), ["tight", "pad48", "offset", ("const", 0.5)], guard=7.0)
    w4src = Src(wrapped4.image, wrapped4.planes[:3] + [0.5])
    items = [(gray, 0, (3, 5, 150, 40)), (gray, 3, None), (const_alpha, 1, None), (const_alpha, 6, None), (const, 2, None), (const, 0, (2, 1, 30, 3)),
             (alias, 4, None), (alias, 0, (1, 1, 5, 5)), (wsrc, 0, None), (wsrc, 2, (1, 1, 23, 7)), (wsrc, 5, None), (w4src, 1, (1, 0, 31, 22)),
             (w4src, 0, (62, 40, 5, 5))]
    distinct = [1, 1, 3, 3, 0, 0, 1, 1, 1, 1, 1, 3, 3]
    return items, distinct, (wrapped, wrapped4)


def test_one_batch_is_one_launch(kc, L, orc, mixed):
    items, distinct, wrapped = mixed
    c0 = counters(kc)
    run(L, orc, items)
    d = delta(kc, c0)
    assert (d["preview"], d["launches"], d["fallback"]) == (1, 1, 0)
    assert d["bytes"] == batch_bytes(items, distinct)
    for wimg in wrapped:
        wimg.assert_untouched()


def test_aliased_planes_are_read_once_and_constants_not_at_all(kc, L, orc, mixed):
    items, distinct, _ = mixed
    alias = [it for it, n in zip(items, distinct) if it[0].planes == 3 and n == 1]
    const = [it for it, n in zip(items, distinct) if n == 0]
    assert len(alias) == 2 and len(const) == 2
    c0 = counters(kc)
    run(L, orc, alias)
    d = delta(kc, c0)
    assert d["bytes"] == batch_bytes(alias, [1, 1]) == 4 * 64 * 64 + 4 * 16 + 4 * 25 + 4 * 25 and d["launches"] == 1
    c0 = counters(kc)
    run(L, orc, const)
    d = delta(kc, c0)
    assert d["bytes"] == 4 * (9 * 5 + 30 * 3) and d["launches"] == 1  # the bytes written: nothing is read


def test_pending_mix_chain_runs_first(kc, L, orc, mixed):
    items, _, _ = mixed
    w, h = 130, 70
    a, b = random_planes(w, h, 4), random_planes(w, h, 4, SEED_B)
    m = kc.mix_process(kc.SlotImage.from_planes(a), kc.SlotImage.from_planes(b), kc.MixType.Multiply)  # not evaluated yet
    c0 = counters(kc)
    reqs, total = layout([(Src(m, a), 2, None)] + items[:8])
    buf = np.full(total + 64, 0xA5, np.uint8)
    assert L.kc_image_previews(reqs, 9, 0, buf.ctypes.data, buf.nbytes) == 0
    assert delta(kc, c0)["preview"] == 1
    msrc = Src(m, m.planes())  # the reference from the product's planes: Multiply has its own tests
    check_bytes(orc, [(msrc, 2, None)] + items[:8], reqs, buf, False)


def test_a_deeper_level_adds_a_launch(kc, L, orc, mixed):
    items, _, _ = mixed
    deep = shared(kc, "256x256", lambda: rgba_src(kc, 256, 256, SEED_B))
    deep.img.materialize()
    c0 = counters(kc)
    run(L, orc, items + [(deep, 8, None)])
    d = delta(kc, c0)
    assert (d["preview"], d["launches"]) == (2, 2)


@pytest.mark.parametrize("n", [1, 4], ids=["gray", "rgba"])
def test_srgb(kc, L, orc, n):
    w, h = 130, 70
    src = gray_src(kc, w, h, SEED_B) if n == 1 else rgba_src(kc, w, h, SEED_B)
    run(L, orc, [(src, 0, (1, 3, 101, 50)), (src, 1, None), (src, 3, (2, 1, 9, 5)), (src, 6, None)], srgb=True)
    deep = shared(kc, "256x256", lambda: rgba_src(kc, 256, 256, SEED_B))
    run(L, orc, [(deep, 7, None), (src, 2, None)], srgb=True)


@pytest.mark.parametrize("n", [1, 4], ids=["gray", "rgba"])
def test_special_values(kc, L, orc, n):
    w, h = 130, 70
    src = gray_src(kc, w, h, special=True) if n == 1 else rgba_src(kc, w, h, special=True)
    for srgb in (False, True):
        run(L, orc, [(src, k, None) for k in range(4)] + [(src, 1, (1, 1, 33, 17)), (src, 2, (3, 2, 5, 9))], srgb=srgb)
    big = Src(kc.SlotImage.from_planes([special_plane(256, 256, 5)]), [special_plane(256, 256, 5)])
    run(L, orc, [(big, 7, None), (big, 2, None)])
    # constants the fold changes: very large and denormal values
    for c in (3e38, -3e38, 1e-45, 4.2e-45, float("inf"), -0.0, float("nan")):
        csrc = Src(kc.SlotImage.from_value(kc.Size(37, 21), c, False), [c], size=(37, 21))
        run(L, orc, [(csrc, k, None) for k in range(6)])


# ------------------------------------------------------------------ the other forms
def test_device_form_on_a_stream(kc, L, orc, torch):
    src = shared(kc, "130x70", lambda: rgba_src(kc, 130, 70))
    deep = shared(kc, "256x256", lambda: rgba_src(kc, 256, 256, SEED_B))
    items = [(src, 0, (1, 1, 77, 30)), (src, 2, None), (deep, 7, None), (src, 5, None)]
    reqs, total = layout(items, gap=8, pitch_extra=[0, 12, 0, 4])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        assert L.kc_image_previews_device(reqs, len(items), 0, C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(stream.cuda_stream)) == 0
        got = t.cpu().numpy()  # on the same stream: ordered behind the launches
    check_bytes(orc, items, reqs, got, False)
    # the torch wrapper: tightly packed, on torch's current stream
    with torch.cuda.stream(stream):
        out, offs = kc.previews_torch([(s.img, k, r) for s, k, r in items], srgb=True)
        host = out.cpu().numpy()
    for (s, k, r), o in zip(items, offs):
        want = s.want(orc, k, True, r)
        assert np.array_equal(host[o:o + want.size].reshape(want.shape), want)
    # refusals: a host pointer, a size below the extent, an unaligned pointer; nothing is launched or written
    t = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    host = np.full(total + 64, 0xA5, np.uint8)
    n0 = kc.stats()["kernel_launches"]
    assert L.kc_image_previews_device(reqs, len(items), 0, C.c_void_p(host.ctypes.data), host.nbytes, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_previews_device(reqs, len(items), 0, C.c_void_p(t.data_ptr()), total - 9, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_previews_device(reqs, len(items), 0, C.c_void_p(t.data_ptr() + 2), total, None) == KC_ERR_INVALID_ARG
    assert kc.stats()["kernel_launches"] == n0
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == 0xA5).all() and (host == 0xA5).all()


def test_python_previews_are_views_of_one_buffer(kc, orc):
    src = shared(kc, "130x70", lambda: rgba_src(kc, 130, 70))
    got = kc.previews([(src.img, 1, None), (src.img, 0, (3, 1, 9, 2)), (src.img, 7, None)])
    assert [g.shape for g in got] == [(35, 65, 4), (2, 9, 4), (1, 1, 4)] and got[1].base is got[0].base
    for g, (k, r) in zip(got, [(1, None), (0, (3, 1, 9, 2)), (7, None)]):
        assert np.array_equal(g, src.want(orc, k, False, r))
    assert kc.previews([]) == []


def test_slot_image_preview(kc, orc):
    src = shared(kc, "1024x512", lambda: rgba_src(kc, 1024, 512))
    assert kc.preview_level(1024, 512, 128) == (3, 128, 64)
    for srgb in (False, True):
        got = src.img.preview(128, srgb)
        assert got.shape == (64, 128, 4) and np.array_equal(got, src.want(orc, 3, srgb))


def test_live_graph_form(kc, L, orc):
    import os
    from golden_graphs import HEART_256, INPUTS, G
    g = G()
    img = g.add({"Image": HEART_256})
    sep = g.add("SeparateRgba")
    out = g.add({"OutputGray": "out"})
    g.connect(img, sep, 0, 0)
    g.connect(sep, out, 1, 0)
    tp = kc.TextureProcessor.new()
    lg = tp.new_live_graph()
    lg.use_cache = True  # every node keeps its slots
    lg.set_base_dir(INPUTS)
    lg.set_node_graph(kc.NodeGraph.from_json(json.dumps(g.dict())))
    lg.await_clean(out)
    rgba = Src(None, lg.slot_data(img, 0).image.planes())
    green = Src(None, lg.slot_data(sep, 1).image.planes())
    assert (rgba.w, rgba.h, len(rgba.channels), len(green.channels)) == (256, 256, 4, 1)
    spec = [(img, 0, 1, None, rgba), (sep, 1, 3, (1, 1, 30, 17), green), (img, 0, 7, None, rgba), (sep, 1, 0, (101, 7, 50, 50), green)]
    for srgb in (False, True):
        c0 = counters(kc)
        got = lg.buffer_previews([s[:4] for s in spec], srgb)
        assert delta(kc, c0)["preview"] == 2
        for g_, (_, _, k, rect, src) in zip(got, spec):
            assert np.array_equal(g_, src.want(orc, k, srgb, rect))
    with pytest.raises(kc.TexProError) as e:
        lg.buffer_previews([(img, 0, 1, None), (sep, 9, 0, (0, 0, 4, 4))])  # no such slot
    assert e.value.code == KC_ERR_NO_SLOT_DATA
    # the C form with pitches and gaps; the image field is ignored
    items = [(s[4], s[2], s[3]) for s in spec]
    reqs, total = layout(items, gap=20, pitch_extra=[0, 8, 4, 0])
    buf = np.full(total + 64, 0xA5, np.uint8)
    nodes, slots = (C.c_uint32 * 4)(*[s[0] for s in spec]), (C.c_uint32 * 4)(*[s[1] for s in spec])
    assert L.kc_live_graph_buffer_previews(lg._h, nodes, slots, reqs, 4, 0, buf.ctypes.data, buf.nbytes) == 0
    check_bytes(orc, items, reqs, buf, False)


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_buffer_untouched(kc, L):
    from kanter_core_amd import _lib
    Req = _lib.kc_preview_request
    src = shared(kc, "130x70", lambda: rgba_src(kc, 130, 70))  # 8 levels; level 1 is 65 x 35
    src.img.materialize()
    h = src.img._h
    buf = np.full(4096, 0xA5, np.uint8)

    def call(reqs, count=None, flags=0, size=4096):
        arr = (Req * len(reqs))(*reqs)
        return L.kc_image_previews(arr, len(reqs) if count is None else count, flags, buf.ctypes.data, size)

    good = Req(h, 1, 0, 0, 8, 8, 0, 32)
    n0 = kc.stats()["kernel_launches"]
    assert call([good, Req(h, 8, 0, 0, 1, 1, 512, 4)]) == KC_ERR_INVALID_ARG   # a level at L
    assert call([good, Req(h, 200, 0, 0, 1, 1, 512, 4)]) == KC_ERR_INVALID_ARG
    assert call([good, Req(h, 1, 58, 0, 8, 8, 512, 32)]) == KC_ERR_INVALID_ARG  # one texel past the last column
    assert call([good, Req(h, 1, 0, 28, 8, 8, 512, 32)]) == KC_ERR_INVALID_ARG  # one texel past the last row
    assert call([good, Req(h, 1, 65, 0, 1, 1, 512, 4)]) == KC_ERR_INVALID_ARG
    assert call([good, Req(h, 1, 0, 0, 8, 8, 512, 28)]) == KC_ERR_INVALID_ARG   # a pitch below 4 * width
    assert call([good, Req(h, 1, 0, 0, 8, 8, 514, 32)]) == KC_ERR_INVALID_ARG   # an unaligned offset
    assert call([good, Req(h, 1, 0, 0, 8, 8, 512, 34)]) == KC_ERR_INVALID_ARG
    assert call([good, Req(h, 1, 0, 0, 0, 8, 512, 32)]) == KC_ERR_INVALID_ARG   # an empty rect
    assert call([good, Req(None, 1, 0, 0, 8, 8, 512, 32)]) == KC_ERR_INVALID_ARG
    assert call([good, Req(h, 1, 0, 0, 8, 8, 4096 - 255, 32)]) == KC_ERR_INVALID_ARG  # the last byte lies past the buffer
    assert call([good], size=255) == KC_ERR_INVALID_ARG
    for flags in (2, 3, 0x100):
        assert call([good], flags=flags) == KC_ERR_UNSUPPORTED
    assert call([Req(h, 0, 0, 0, 1, 1, 0, 4)] * 4097) == KC_ERR_INVALID_ARG
    assert kc.stats()["kernel_launches"] == n0
    assert (buf == 0xA5).all()
    assert call([good], count=0) == 0 and kc.stats()["kernel_launches"] == n0 and (buf == 0xA5).all()
    assert call([good, Req(h, 1, 57, 27, 8, 8, 4096 - 256, 32)]) == 0  # the last column and row, the buffer's last byte
    assert kc.stats()["kernel_launches"] == n0 + 1
