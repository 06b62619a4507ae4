"""Per-channel statistics on the device (kc_image_channel_stats / kc_live_graph_buffer_channel_stats, csrc/stats.*): min and max
in the total order of the floats, NaN counts and the u8 histograms, bit for bit against numpy -- the ranges from the same integer
keys, the bins as np.bincount of the oracle's to_u8 and of the library's own kc_image_to_u8 bytes -- over edge-case planes,
ragged widths, constant and shared planes, pending chains, padded caller planes and a live graph."""
import ctypes as C
import json

import numpy as np
import pytest

from util import SEED_A, SEED_B, key_range, splitmix_plane, synthetic_rgba, with_edge_cases

pytestmark = pytest.mark.gpu

KC_ERR_INVALID_ARG, KC_ERR_NO_SLOT_DATA, KC_ERR_UNSUPPORTED = 102, 10, 104


@pytest.fixture(scope="module")
def kc():
    import kanter_core_amd as kc
    kc.init(0)
    return kc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


def launches(kc):
    return kc.stats()["kernel_launches"]


def counted(kc, img, **kw):
    """(launches, algorithmic bytes) of one channel_stats call"""
    l0, b0 = launches(kc), kc.stats()["algorithmic_bytes"]
    img.channel_stats(**kw)
    return launches(kc) - l0, kc.stats()["algorithmic_bytes"] - b0


def bits(x):
    return int(np.float32(x).view(np.uint32))


def check(kc, orc, img, planes, histogram=True, srgb=False):
    """img.channel_stats against numpy of `planes` (the image's own channels)."""
    st = img.channel_stats(histogram=histogram, srgb=srgb)
    n = len(planes)
    h, w = planes[0].shape
    assert st.pixels == h * w and len(st.min) == n and len(st.max) == n and len(st.nan_count) == n
    for c, p in enumerate(planes):
        lo, hi, nans = key_range(p)
        assert int(st.nan_count[c]) == nans, c
        if lo is None:
            assert np.isnan(st.min[c]) and np.isnan(st.max[c]), c
        else:
            assert (bits(st.min[c]), bits(st.max[c])) == (lo, hi), (c, st.min[c], st.max[c])
    if not histogram:
        assert st.histogram is None
        return st
    assert st.histogram.shape == (n, 256) and st.histogram.dtype == np.uint64
    want = orc.to_u8(orc.Image(list(planes)), srgb)
    own = img.to_u8(srgb)
    for c in range(n):
        assert np.array_equal(st.histogram[c], np.bincount(want[:, :, c].reshape(-1), minlength=256)), c
        assert np.array_equal(st.histogram[c], np.bincount(own[:, :, c].reshape(-1), minlength=256)), c
    return st


def edge_rgba(h, w, seed=SEED_A):
    return [with_edge_cases(p * 1.2 - 0.1, shift=c) for c, p in enumerate(synthetic_rgba(seed, h, w))]


# (h, w): 1x1, 3x5, widths 4k+1 .. 4k+3, 4097 x 33
SIZES = [(1, 1), (3, 5), (7, 9), (6, 10), (5, 11), (33, 4097)]


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("rgba", [False, True])
@pytest.mark.parametrize("mode", ["minmax", "hist", "srgb"])
def test_sizes_edge_cases(kc, orc, hw, rgba, mode):
    h, w = hw
    planes = edge_rgba(h, w) if rgba else [with_edge_cases(splitmix_plane(SEED_B, 0, h, w) * 1.5 - 0.2, shift=3)]
    check(kc, orc, kc.SlotImage.from_planes(planes), planes, histogram=mode != "minmax", srgb=mode == "srgb")


def contract_planes(h, w):
    rng = np.random.default_rng(7)
    zeros = np.where(rng.random((h, w)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    infs = np.where(rng.random((h, w)) < 0.5, np.float32(-np.inf), np.float32(np.inf)).astype(np.float32)
    denorm = (rng.integers(1, 1 << 23, (h, w)).astype(np.uint32) | (rng.integers(0, 2, (h, w)).astype(np.uint32) << 31)).view(np.float32)
    far = (rng.standard_normal((h, w)) * 1e6).astype(np.float32)
    allnan = np.full((h, w), np.nan, np.float32)
    allnan.reshape(-1).view(np.uint32)[::3] = 0xffc00001  # other payloads, negative sign
    hot = np.zeros((h, w), np.float32)
    hot.reshape(-1)[::997] = 0.5
    ones = np.full((h, w), 1.0, np.float32)
    ones.reshape(-1)[5::11] = 7.0  # clamps to the same bin
    return zeros, infs, denorm, far, allnan, hot, ones


@pytest.mark.parametrize("hw", [(3, 5), (31, 45), (64, 129)])
@pytest.mark.parametrize("srgb", [False, True])
def test_contract_planes(kc, orc, hw, srgb):
    h, w = hw
    zeros, infs, denorm, far, allnan, hot, ones = contract_planes(h, w)
    for planes in ([zeros, infs, denorm, allnan], [far, hot, ones, zeros]):
        check(kc, orc, kc.SlotImage.from_planes(planes), planes, srgb=srgb)
    for p in (zeros, infs, denorm, far, allnan, hot, ones):
        check(kc, orc, kc.SlotImage.from_planes([p]), [p], srgb=srgb)
    st = kc.SlotImage.from_planes([zeros]).channel_stats()
    assert bits(st.min[0]) == 0x80000000 and bits(st.max[0]) == 0  # -0.0 < +0.0
    st = kc.SlotImage.from_planes([allnan]).channel_stats(histogram=True)
    assert np.isnan(st.min[0]) and int(st.nan_count[0]) == h * w and int(st.histogram[0][255]) == h * w


def test_full_size_srgb_and_one_bin(kc, orc):
    n = 4096
    planes = edge_rgba(n, n, SEED_B)
    check(kc, orc, kc.SlotImage.from_planes(planes), planes, srgb=True)
    hot = np.zeros((n, n), np.float32)
    hot[::512, ::7] = 0.75
    check(kc, orc, kc.SlotImage.from_planes([hot]), [hot])


@pytest.mark.parametrize("v", [0.3, -0.0, 0.0, float("nan"), 7.0, -float("inf"), 1.0, 0.5])
@pytest.mark.parametrize("rgba", [False, True])
@pytest.mark.parametrize("srgb", [False, True])
def test_constant_images_launch_nothing(kc, orc, v, rgba, srgb):
    img = kc.SlotImage.from_value((13, 6), v, rgba)
    planes = [np.full((6, 13), v if (not rgba or c < 3) else 1.0, np.float32) for c in range(4 if rgba else 1)]
    assert counted(kc, img, histogram=True, srgb=srgb) == (0, 0)  # constant channels are answered on the host
    st = check(kc, orc, img, planes, srgb=srgb)
    assert int(st.histogram.sum()) == len(planes) * 13 * 6


def test_combine_with_missing_inputs(kc, orc):
    h, w = 21, 18
    g = splitmix_plane(SEED_A, 1, h, w)
    gray = kc.SlotImage.from_planes([g])
    img = kc.combine_rgba_process([None, gray, None, None])  # R, B: the shared zero plane, A: ones
    planes = [np.zeros((h, w), np.float32), g, np.zeros((h, w), np.float32), np.ones((h, w), np.float32)]
    # the stats kernel and its combine, for the one resident plane
    assert counted(kc, img) == (2, h * w * 4)
    assert counted(kc, img, histogram=True, srgb=True) == (2, h * w * 4)
    check(kc, orc, img, planes, histogram=False)
    check(kc, orc, img, planes, srgb=True)
    all_const = kc.combine_rgba_process([None, None, None, None])
    assert counted(kc, all_const, histogram=True) == (0, 0)
    check(kc, orc, all_const, [np.zeros((1, 1), np.float32)] * 3 + [np.ones((1, 1), np.float32)])


@pytest.mark.parametrize("srgb", [False, True])
def test_gray_as_rgba_reads_one_plane(kc, orc, srgb):
    h, w = 37, 41
    g = with_edge_cases(splitmix_plane(SEED_B, 2, h, w) * 1.3 - 0.1)
    img = kc.SlotImage.from_planes([g]).as_type(True)  # [p, p, p, ones]
    assert counted(kc, img, histogram=True, srgb=srgb) == (2, h * w * 4)
    check(kc, orc, img, [g, g, g, np.ones((h, w), np.float32)], srgb=srgb)


def test_pending_mix_chain(kc, orc):
    h, w = 45, 67
    a, b = edge_rgba(h, w, SEED_A), edge_rgba(h, w, SEED_B)
    m = kc.mix_process(kc.SlotImage.from_planes(a), kc.SlotImage.from_planes(b), kc.MixType.Multiply)
    st = m.channel_stats(histogram=True, srgb=True)  # forces the chain first
    planes = m.planes()
    want = check(kc, orc, m, planes, srgb=True)
    for f in ("min", "max"):
        assert np.array_equal(getattr(st, f).view(np.uint32), getattr(want, f).view(np.uint32))
    assert np.array_equal(st.nan_count, want.nan_count) and np.array_equal(st.histogram, want.histogram)


@pytest.mark.parametrize("w", [9, 10, 11, 12])
def test_wrapped_plane_padding_is_not_counted(kc, orc, w):
    import torch
    from kanter_core_amd import _lib
    L = _lib.load()
    h, pitch_f = 19, 20
    p = with_edge_cases(splitmix_plane(SEED_A, 3, h, w) * 0.8 + 0.1, shift=2)
    t = torch.empty((h, pitch_f), dtype=torch.float32, device="cuda")
    pad = torch.tensor([float("nan"), -float("inf"), 1e30, -1e30], dtype=torch.float32)
    t[:, :] = pad.repeat(pitch_f // 4).cuda()
    t[:, :w] = torch.from_numpy(p).cuda()
    torch.cuda.synchronize()
    plane, img = C.c_void_p(), C.c_void_p()
    assert L.kc_plane_wrap(t.data_ptr(), w, h, pitch_f * 4, C.byref(plane)) == 0
    assert L.kc_image_gray(plane, C.byref(img)) == 0
    L.kc_plane_release(plane)
    src = kc.SlotImage(img.value)
    for srgb in (False, True):
        check(kc, orc, src, [p], srgb=srgb)
    del src
    torch.cuda.synchronize()


def test_live_graph_invert(kc):
    import os
    from golden_graphs import HEART_256, INPUTS, G
    with open(os.path.join(INPUTS, "invert_graph.json")) as f:
        inner = json.load(f)
    inp = next(n["node_id"] for n in inner["nodes"] if n["node_type"] == {"InputGray": "in"})
    outn = next(n["node_id"] for n in inner["nodes"] if n["node_type"] == {"OutputGray": "out"})
    g = G()
    src = g.add({"Image": HEART_256})
    sep = g.add("SeparateRgba")
    gn = g.add({"Graph": inner})
    out = g.add({"OutputGray": "out"})
    g.connect(src, sep, 0, 0)
    g.connect(sep, gn, 0, inp)
    g.connect(gn, out, outn, 0)
    tp = kc.TextureProcessor.new()
    lg = tp.new_live_graph()
    lg.set_base_dir(INPUTS)
    lg.set_node_graph(kc.NodeGraph.from_json(json.dumps(g.dict())))
    lg.await_clean(out)
    for srgb in (False, True):
        st = lg.buffer_channel_stats(out, 0, histogram=True, srgb=srgb)
        px = lg.buffer_rgba(out, 0, srgb)
        assert st.pixels == 256 * 256 and len(st.min) == 1
        assert np.array_equal(st.histogram[0], np.bincount(px[:, :, 0].reshape(-1), minlength=256))
    plane = lg.slot_data(out, 0).image.planes()[0]
    lo, hi, nans = key_range(plane)
    st = lg.buffer_channel_stats(out, 0)
    assert (bits(st.min[0]), bits(st.max[0]), int(st.nan_count[0])) == (lo, hi, nans)
    assert st.histogram is None
    with pytest.raises(kc.TexProError) as e:
        lg.buffer_channel_stats(out, 5)  # no such slot
    assert e.value.code == KC_ERR_NO_SLOT_DATA
    with pytest.raises(kc.TexProError) as e:
        lg.buffer_channel_stats(gn + 100, 0)
    assert e.value.code == KC_ERR_NO_SLOT_DATA


def test_refusals_leave_out_untouched(kc):
    from kanter_core_amd import _lib
    L = _lib.load()
    img = kc.SlotImage.from_planes([splitmix_plane(SEED_A, 0, 4, 4)])
    s = _lib.kc_channel_stats()
    s.channels = 0xdead
    before = launches(kc)
    assert L.kc_image_channel_stats(img._h, 4, C.byref(s)) == KC_ERR_UNSUPPORTED
    assert L.kc_image_channel_stats(img._h, 2, C.byref(s)) == KC_ERR_INVALID_ARG
    assert s.channels == 0xdead and launches(kc) == before
    with pytest.raises(ValueError):
        img.channel_stats(srgb=True)
