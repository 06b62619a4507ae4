"""Packed copies of chain inputs (csrc/chain_pack.cpp, chain_pack.h) on the device.  Every case evaluates the same program with
pack_sources = 2 (every eligible input is packed at its first sighting, whatever the size) and with pack_sources = 0 (the f32
path) and compares both with each other and with the CPU oracle, bit for bit, NaN == NaN.

Unit counts (float4 per plane) straddle the lane and workgroup edges of both kernel forms: one float4 per lane (nt_force 0)
on 4 x 1 and on 255 / 256 / 257 quads, two per lane (nt_force 0x101, "_q2") on 511 / 512 / 513 quads.  Which form a launch
took is read from kc_stats_counter: "packed_launches", "packed_planes", "pack_rejected", "packed_bytes"."""
import numpy as np
import pytest

from util import SEED_A, SEED_B, assert_planes, splitmix_plane, wrapped_image

pytestmark = pytest.mark.gpu

ONE_QUAD = [(4, 1), (1020, 1), (1024, 1), (1028, 1)]
TWO_QUADS = [(2044, 1), (2048, 1), (2052, 1)]
SHAPES = [(s, 0) for s in ONE_QUAD] + [(s, 0x101) for s in TWO_QUADS]  # (shape, nt_force)


def inv(op, right, k, c):
    """One record "c - (acc op input k)" (right: "c - (input k op acc)") as two Mix nodes."""
    return [(op, right, ("p", k)), ("Subtract", True, ("c", c))]


# every {+, -, *, *_INV} code once, input 0 the start value and input 1 the operand of each
ALL_CODES = ([("Add", False, ("p", 1)), ("Subtract", False, ("p", 1)), ("Subtract", True, ("p", 1)), ("Multiply", False, ("p", 1))] +
             inv("Add", False, 1, 1.5) + inv("Subtract", False, 1, 0.75) + inv("Subtract", True, 1, -0.375) + inv("Multiply", False, 1, 1.0))
PASS_THROUGH = [("Add", False, ("c", 0.0)), ("Multiply", False, ("c", 1.0))]  # x + 0.0, * 1.0: x itself for x >= +0.0


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    saved = {n: kc.get_option(n) for n in ("nt_force", "chain1", "cache_budget_mb", "replay")}
    spec, pack, budget = kc.get_specialize(), kc.get_pack_sources(), kc.get_pack_budget_mb()
    kc.set_option("chain1", 0)  # a one-record program goes to its compiled kernel, not to chain1.hip
    kc.set_specialize(2)        # compile at first sight and wait
    kc.set_pack_sources(2)
    yield kc
    for n, v in saved.items():
        kc.set_option(n, v)
    kc.set_specialize(spec)
    kc.set_pack_sources(pack)
    kc.set_pack_budget_mb(budget)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


def plane_of(kind, w, h, seed=SEED_A):
    """fix24: k * 2^-24; u8: k / 255.0f; f32: full mantissas with negatives (fits no tier)."""
    u = splitmix_plane(seed, 0, h, w)
    if kind == "fix24":
        return u
    if kind == "u8":
        return np.floor(u * np.float32(256.0)).astype(np.float32) / np.float32(255.0)
    assert kind == "f32"
    return u * np.float32(3.7) - np.float32(1.1)


def run_oracle(orc, planes, start, steps):
    h, w = planes[0].shape
    full = lambda v: np.full((h, w), v, np.float32)  # noqa: E731
    want = planes[start[1]] if start[0] == "p" else full(start[1])
    for op, right, (kind, v) in steps:
        x = planes[v] if kind == "p" else full(v)
        want = orc.mix_plane(op, x, want) if right else orc.mix_plane(op, want, x)
    return want


def run_device(kc, imgs, start, steps):
    """The program on SlotImages (Gray or RGBA); the images stay the caller's, so every input plane has a second holder."""
    mix, mt = kc.mix_process, kc.MixType.parse
    s = imgs[0].size()
    const = lambda v: kc.SlotImage.from_value((s.width, s.height), v, imgs[0].is_rgba())  # noqa: E731
    acc = imgs[start[1]] if start[0] == "p" else const(start[1])
    for op, right, (kind, v) in steps:
        x = imgs[v] if kind == "p" else const(v)
        acc = mix(x, acc, mt(op)) if right else mix(acc, x, mt(op))
    return acc.planes()


COUNTERS = ("packed_launches", "packed_planes", "pack_rejected")


def counted(kc, run):
    before = {n: kc.stats_counter(n) for n in COUNTERS}
    got = run()
    return got, {n: kc.stats_counter(n) - before[n] for n in COUNTERS}


def both_ways(kc, imgs, start, steps):
    """(packed result, its counter deltas, f32 result): pack_sources 2, then 0 on the same images."""
    kc.set_pack_sources(2)
    got, d = counted(kc, lambda: run_device(kc, imgs, start, steps))
    kc.set_pack_sources(0)
    plain, d0 = counted(kc, lambda: run_device(kc, imgs, start, steps))
    kc.set_pack_sources(2)
    assert d0 == {n: 0 for n in COUNTERS}, d0
    return got, d, plain


TIER_PAIRS = [("fix24", "f32"), ("f32", "fix24"), ("fix24", "fix24"), ("u8", "f32"), ("fix24", "u8"), ("u8", "u8")]


@pytest.mark.parametrize("kinds", TIER_PAIRS, ids=["%s-%s" % k for k in TIER_PAIRS])
def test_every_code_with_packed_start_and_operand(kc, orc, kinds):
    for (w, h), force in SHAPES:
        kc.set_option("nt_force", force)
        planes = [plane_of(kinds[0], w, h, SEED_A), plane_of(kinds[1], w, h, SEED_B)]
        imgs = [kc.SlotImage.from_planes([p]) for p in planes]
        got, d, plain = both_ways(kc, imgs, ("p", 0), ALL_CODES)
        what = "%s %dx%d nt %x" % (kinds, w, h, force)
        n_packed = sum(k != "f32" for k in kinds)
        assert d == {"packed_launches": 1, "packed_planes": n_packed, "pack_rejected": 2 - n_packed}, (what, d)
        assert_planes(got, plain, what=what + " packed vs f32")
        assert_planes(got, [run_oracle(orc, planes, ("p", 0), ALL_CODES)], what=what + " vs oracle")
        # the shadows are there now: the next evaluation launches the packed form without another pass
        _, d2 = counted(kc, lambda: run_device(kc, imgs, ("p", 0), ALL_CODES))
        assert d2 == {"packed_launches": 1, "packed_planes": 0, "pack_rejected": 0}, (what, d2)


def test_rgba_and_constant_start(kc, orc):
    kc.set_option("nt_force", 0x102)
    w, h = 2052, 1
    chans = [[splitmix_plane(SEED_A + i, c, h, w) for c in range(4)] for i in range(2)]
    imgs = [kc.SlotImage.from_planes(p) for p in chans]
    steps = inv("Add", False, 0, 0.375) + [("Subtract", True, ("p", 1)), ("Multiply", False, ("p", 0))]
    got, d, plain = both_ways(kc, imgs, ("c", 1.5), steps)
    assert d["packed_launches"] >= 1 and d["packed_planes"] in (6, 8) and d["pack_rejected"] == 0, d  # (alpha: Mix's own rule)
    assert_planes(got, plain, what="rgba packed vs f32")
    for c in range(3):
        assert_planes([got[c]], [run_oracle(orc, [chans[0][c], chans[1][c]], ("c", 1.5), steps)], what="rgba channel %d vs oracle" % c)


def test_u8_decode_of_all_256_values(kc):
    kc.set_option("nt_force", 0)
    host = np.arange(256, dtype=np.float32) / np.float32(255.0)  # k / 255.0f, correctly rounded
    img = kc.SlotImage.from_planes([host.reshape(1, 256)])
    got, d, plain = both_ways(kc, [img], ("p", 0), PASS_THROUGH)
    assert d == {"packed_launches": 1, "packed_planes": 1, "pack_rejected": 0}, d
    assert_planes(got, [host.reshape(1, 256)], what="u8 decode vs k / 255.0f on the host")
    assert_planes(got, plain, what="u8 decode vs f32")


NEAR = [-0.0, 1.0, 2.0 ** -25, 3 * 2.0 ** -26, np.nan, np.inf, -(2.0 ** -24), 1e-30]


@pytest.mark.parametrize("value", NEAR, ids=[repr(float(v)) for v in NEAR])
def test_fix24_near_misses_stay_f32(kc, orc, value):
    kc.set_option("nt_force", 0)
    w, h = 1028, 1
    other = plane_of("fix24", w, h, SEED_B)
    for pos in (0, w // 2 + 1, w - 1):
        p = plane_of("fix24", w, h, SEED_A).copy()
        p[0, pos] = np.float32(value)
        imgs = [kc.SlotImage.from_planes([p]), kc.SlotImage.from_planes([other])]
        what = "near miss %r at %d" % (value, pos)
        got, d, plain = both_ways(kc, imgs[:1], ("p", 0), PASS_THROUGH)
        assert d == {"packed_launches": 0, "packed_planes": 0, "pack_rejected": 1}, (what, d)  # refused: the launch stays f32
        assert_planes(got, plain, what=what + " vs f32")
        assert_planes(got, [run_oracle(orc, [p], ("p", 0), PASS_THROUGH)], what=what + " vs oracle")
        # marked: never tried again; beside a clean operand that is packed the plane is still read as f32
        got, d, plain = both_ways(kc, imgs, ("p", 0), ALL_CODES[:4])
        assert d == {"packed_launches": 1, "packed_planes": 1, "pack_rejected": 0}, (what, d)
        assert_planes(got, plain, what=what + " beside a packed operand vs f32")
        assert_planes(got, [run_oracle(orc, [p, other], ("p", 0), ALL_CODES[:4])], what=what + " beside a packed operand vs oracle")


def test_u8_plane_with_one_off_grid_value_stays_f32(kc, orc):
    kc.set_option("nt_force", 0)
    p = plane_of("u8", 1024, 1).copy()
    p[0, 517] = np.float32(0.5)  # on the FIX24 grid, but the other samples are not
    img = kc.SlotImage.from_planes([p])
    got, d, plain = both_ways(kc, [img], ("p", 0), PASS_THROUGH)
    assert d == {"packed_launches": 0, "packed_planes": 0, "pack_rejected": 1}, d
    assert_planes(got, plain, what="u8 near miss vs f32")
    assert_planes(got, [run_oracle(orc, [p], ("p", 0), PASS_THROUGH)], what="u8 near miss vs oracle")


def test_channel_mismatch_keeps_the_slot_f32(kc, orc):
    kc.set_option("nt_force", 0)
    w, h = 1028, 1
    chans = [plane_of("fix24", w, h, SEED_A), plane_of("f32", w, h, SEED_A + 1), plane_of("fix24", w, h, SEED_A + 2), plane_of("fix24", w, h, SEED_A + 3)]
    img = kc.SlotImage.from_planes(chans)
    got, d, plain = both_ways(kc, [img], ("p", 0), PASS_THROUGH)
    assert d["packed_launches"] == 0 and d["packed_planes"] == 0 and d["pack_rejected"] >= 1, d
    assert_planes(got, plain, what="channel mismatch vs f32")
    for c in range(3):
        assert_planes([got[c]], [run_oracle(orc, [chans[c]], ("p", 0), PASS_THROUGH)], what="channel mismatch, channel %d vs oracle" % c)


def test_ineligible_planes_are_never_packed(kc, orc):
    import torch
    kc.set_option("nt_force", 0)
    # a width that is no whole number of float4
    p = plane_of("fix24", 1022, 1)
    got, d, plain = both_ways(kc, [kc.SlotImage.from_planes([p])], ("p", 0), PASS_THROUGH)
    assert d == {n: 0 for n in COUNTERS}, d
    assert_planes(got, plain)
    # rows padded to the pool's pitch (1028 x 3: the pitch is not the width)
    p = plane_of("fix24", 1028, 3)
    got, d, plain = both_ways(kc, [kc.SlotImage.from_planes([p])], ("p", 0), PASS_THROUGH)
    assert d == {n: 0 for n in COUNTERS}, d
    assert_planes(got, plain)
    # a caller-owned plane: its owner may write it
    p = plane_of("fix24", 1024, 1)
    wi = wrapped_image(kc, torch, [p], "tight", 77.0)
    got, d, plain = both_ways(kc, [wi.image], ("p", 0), PASS_THROUGH)
    assert d == {n: 0 for n in COUNTERS}, d
    assert_planes(got, plain)
    assert_planes(got, [run_oracle(orc, [p], ("p", 0), PASS_THROUGH)])


def test_band_views_are_never_packed(kc):
    kc.set_option("nt_force", 0)
    w, h = 64, 8  # dense rows: the planes themselves are eligible, their row-band views are not
    host = [[splitmix_plane(SEED_A + i, c, h, w) for c in range(4)] for i in range(2)]
    tp = kc.TextureProcessor.new()
    lg = tp.new_live_graph()
    for i in range(2):
        lg.embed_slot_data_with_id(kc.SlotData(0, 0, kc.SlotImage.from_planes(host[i])), i)
    na, nb = (lg.add_node(kc.Node.new(kc.NodeType.Embed(i))) for i in range(2))
    prev = na
    for op in (kc.MixType.Add, kc.MixType.Multiply, kc.MixType.Subtract):
        n = lg.add_node(kc.Node.new(kc.NodeType.Mix(op)))
        lg.connect(prev, n, 0, 0)
        lg.connect(nb, n, 0, 1)
        prev = n
    band, d = counted(kc, lambda: lg.evaluate_band(prev, 2, 6).planes())
    assert d == {n: 0 for n in COUNTERS}, d
    kc.set_pack_sources(0)
    plain = lg.evaluate_band(prev, 2, 6).planes()
    kc.set_pack_sources(2)
    assert_planes(band, plain, what="band vs f32")


def test_shadows_leave_with_their_planes(kc):
    kc.set_option("nt_force", 0)
    kc.sync()
    in_use0, bytes0 = kc.stats()["bytes_in_use"], kc.stats_counter("packed_bytes")
    p = plane_of("fix24", 1024, 1)
    img = kc.SlotImage.from_planes([p])
    got, d = counted(kc, lambda: run_device(kc, [img], ("p", 0), PASS_THROUGH))
    assert d["packed_planes"] == 1
    assert kc.stats_counter("packed_bytes") == bytes0 + 1024 * 3  # 256 quads of 12 bytes (a multiple of the pool's 256)
    del img, got
    import gc
    gc.collect()
    assert kc.stats_counter("packed_bytes") == bytes0
    assert kc.stats()["bytes_in_use"] == in_use0


def test_in_place_writers_leave_no_stale_shadow(kc, orc):
    import ctypes as C
    from kanter_core_amd import _lib
    L = _lib.load()
    kc.set_option("nt_force", 0)
    w, h = 1024, 1
    first, second = plane_of("fix24", w, h, SEED_A), plane_of("fix24", w, h, SEED_B)
    img = kc.SlotImage.from_planes([first])
    got, d = counted(kc, lambda: run_device(kc, [img], ("p", 0), PASS_THROUGH))
    assert d["packed_planes"] == 1 and d["packed_launches"] == 1
    assert_planes(got, [first])
    # kc_plane_upload_f32 writes into the plane: the shadow goes, and the plane is packed again from its new pixels
    hnd = img.plane_handles()[0]
    assert L.kc_plane_upload_f32(hnd, second.ctypes.data, w * 4) == 0
    got, d = counted(kc, lambda: run_device(kc, [img], ("p", 0), PASS_THROUGH))
    assert d["packed_planes"] == 1 and d["packed_launches"] == 1, d
    assert_planes(got, [second], what="after an upload in place")
    # kc_plane_device_ptr hands the pointer out: no packed copy from then on, whatever is written through it
    ptr, pitch = C.c_void_p(), C.c_size_t()
    assert L.kc_plane_device_ptr(hnd, C.byref(ptr), C.byref(pitch)) == 0
    got, d = counted(kc, lambda: run_device(kc, [img], ("p", 0), PASS_THROUGH))
    assert d == {n: 0 for n in COUNTERS}, d
    assert_planes(got, [second], what="after the pointer left the library")
    L.kc_plane_release(hnd)


def test_budget_just_under_one_shadow_packs_nothing(kc):
    kc.set_option("nt_force", 0)
    w, h = 1024, 1024  # a U8 shadow is exactly 1 MiB
    p = plane_of("u8", w, h)
    held = kc.stats_counter("packed_bytes")
    assert held < (1 << 20)  # (nothing of the other tests is alive)
    img = kc.SlotImage.from_planes([p])
    kc.set_pack_budget_mb(0)
    try:
        got, d, plain = both_ways(kc, [img], ("p", 0), PASS_THROUGH)
        assert d == {n: 0 for n in COUNTERS}, d
        assert_planes(got, plain)
        kc.set_pack_budget_mb(1 if held == 0 else 2)
        got, d = counted(kc, lambda: run_device(kc, [img], ("p", 0), PASS_THROUGH))
        assert d == {"packed_launches": 1, "packed_planes": 1, "pack_rejected": 0}, d
        assert_planes(got, plain)
    finally:
        kc.set_pack_budget_mb(4096)


@pytest.mark.parametrize("replay", [1, 0], ids=["replay", "walk"])
def test_adoption_by_a_live_graph(kc, replay):
    """pack_sources = 1 with a cache budget of 0 (every launch counts as HBM-bound): f32 at the first sighting, the pass at the
    second, packed launches from then on; the same pixels every time.  With the default budget the same graph never packs."""
    kc.set_option("nt_force", -1)
    kc.set_option("replay", replay)
    w, h = 1028, 1
    host = [[splitmix_plane(SEED_A + i, c, h, w) for c in range(4)] for i in range(2)]

    def graph():
        tp = kc.TextureProcessor.new()
        lg = tp.new_live_graph()
        for i in range(2):
            lg.embed_slot_data_with_id(kc.SlotData(0, 0, kc.SlotImage.from_planes(host[i])), i)
        na, nb = (lg.add_node(kc.Node.new(kc.NodeType.Embed(i))) for i in range(2))
        prev, first = na, None
        for op in (kc.MixType.Add, kc.MixType.Multiply, kc.MixType.Subtract, kc.MixType.Add):
            n = lg.add_node(kc.Node.new(kc.NodeType.Mix(op)))
            lg.connect(prev, n, 0, 0)
            lg.connect(nb, n, 0, 1)
            first = first if first is not None else n
            prev = n
        return tp, lg, na, first, prev

    def evaluate(g):
        _, lg, na, first, last = g
        lg.connect(na, first, 0, 0)
        lg.await_clean(last)
        return lg.slot_data(last, 0).image.planes()

    try:
        kc.set_pack_sources(1)
        g = graph()
        small = [counted(kc, lambda: evaluate(g)) for _ in range(3)]
        assert all(d == {n: 0 for n in COUNTERS} for _, d in small), [d for _, d in small]  # a small graph never packs
        kc.set_option("cache_budget_mb", 0)
        g = graph()
        runs = [counted(kc, lambda: evaluate(g)) for _ in range(5)]
        deltas = [d for _, d in runs]
        assert deltas[0] == {n: 0 for n in COUNTERS}, deltas
        n = deltas[1]["packed_launches"]
        assert deltas[1]["packed_planes"] in (6, 8) and n >= 1 and deltas[1]["pack_rejected"] == 0, deltas  # R, G, B (and alpha) of both sources
        assert all(d == {"packed_launches": n, "packed_planes": 0, "pack_rejected": 0} for d in deltas[2:]), deltas
        for got, _ in runs + small:
            assert_planes(got, small[0][0], what="replay %d" % replay)
    finally:
        kc.set_pack_sources(2)
        kc.set_option("cache_budget_mb", 208)
        kc.set_option("replay", 1)
