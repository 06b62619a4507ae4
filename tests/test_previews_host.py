"""kc_image_previews without a device: kc_preview_plan -- the host function the entry points plan with -- against a small
restatement of the pass rule in Python (passes, workgroups per pass, the fallback flag, the scratch extents), the refusals that
are arithmetic (checked before kc_init), and the Python names."""
import ctypes as C

import pytest

import mip_ref

KC_OK, KC_ERR_NO_DEVICE, KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 0, 101, 102, 104
PREVIEW_SRGB = 1


@pytest.fixture(scope="module")
def L():
    from kanter_core_amd import _lib
    return _lib.load()


def ceil_div(a, b):
    return (a + b - 1) // b


def want_plan(w, h, level, rect):
    """The pass rule of the header: (passes, fallback, [n], [workgroups], [(scratch w, h)], [scratch bytes per plane])."""
    x, y, rw, rh = rect
    H = min(w.bit_length(), h.bit_length()) - 1
    if level > H:  # one extent has reached 1: the chain, then the rect of levels[level] at relative level 0
        return 1, True, [0], [ceil_div(ceil_div(rw, 4) * rh, 256)], [(0, 0)], [0]
    ns, wgs, scratch, sbytes = [], [], [], []
    left = level
    while True:
        if left > 6:
            up = left - 6
            fx, fy, fw, fh = x << up, y << up, rw << up, rh << up  # the footprint at level 6 of this pass's source: one tile each
            ns.append(6)
            wgs.append(fw * fh)
            scratch.append((fw, fh))
            sbytes.append(ceil_div(fw, 64) * 64 * fh * 4)
            x, y, left = 0, 0, up  # the next pass reads the scratch as an image of its own, the rect at its origin
        else:
            ns.append(left)
            if left == 0:
                wgs.append(ceil_div(ceil_div(rw, 4) * rh, 256))
            else:
                span = 64 >> left  # texels of the stored level per 64 x 64 source tile
                wgs.append(((x + rw - 1) // span - x // span + 1) * ((y + rh - 1) // span - y // span + 1))
            scratch.append((0, 0))
            sbytes.append(0)
            return len(ns), False, ns, wgs, scratch, sbytes


def rects_of(lw, lh):
    out = [(0, 0, lw, lh)]
    for x in range(4):
        for wd in (1, 2, 3, 5):
            if x + wd <= lw and lh >= 2:
                out.append((x, 1, wd, min(3, lh - 1)))
    out.append((lw - min(lw, 5), lh - min(lh, 3), min(lw, 5), min(lh, 3)))
    if lw > 70 and lh > 40:
        out.append((61, 33, lw - 66, lh - 38))
    return out


SIZES = [(1, 1), (1, 5), (5, 1), (64, 2), (64, 64), (130, 70), (256, 256), (8192, 128), (4096, 4096), (16384, 8192)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_plan_against_the_restated_rule(size):
    from kanter_core_amd import api
    w, h = size
    for level in range(mip_ref.level_count(w, h)):
        lw, lh = mip_ref.level_size(w, h, level)
        for rect in rects_of(lw, lh):
            p = api.preview_plan(w, h, level, rect)
            got = (p.passes, p.fallback, p.levels, p.workgroups, p.scratch_sizes, p.scratch_bytes)
            assert got == want_plan(w, h, level, rect), (w, h, level, rect, got)
            assert p.level_size == (lw, lh)
            assert p.passes == (1 if p.fallback else max(1, ceil_div(level, 6)))
        assert api.preview_plan(w, h, level) == api.preview_plan(w, h, level, (0, 0, lw, lh))  # None: the whole level


def test_plan_examples():
    from kanter_core_amd import api
    p = api.preview_plan(4096, 4096, 5)  # a 128 x 128 thumbnail: one pass, one workgroup per source tile
    assert (p.passes, p.fallback, p.levels, p.workgroups) == (1, False, [5], [64 * 64])
    p = api.preview_plan(8192, 128, 7, (1, 0, 63, 1))  # the level-6 scratch is 126 x 2 of the 128 x 2 level: pass 2 spans two tiles
    assert (p.passes, p.levels, p.workgroups, p.scratch_sizes) == (2, [6, 1], [126 * 2, 2], [(126, 2), (0, 0)])
    p = api.preview_plan(8192, 128, 7)
    assert (p.workgroups, p.scratch_sizes, p.scratch_bytes) == ([256, 2], [(128, 2), (0, 0)], [128 * 2 * 4, 0])
    p = api.preview_plan(16384, 8192, 13)  # three passes
    assert (p.passes, p.levels, p.level_size) == (3, [6, 6, 1], (2, 1))
    assert api.preview_plan(64, 2, 2).fallback and not api.preview_plan(64, 2, 1).fallback
    assert api.preview_plan(4096, 4096, 0, (0, 0, 512, 512)).workgroups == [128 * 512 // 256]


def test_plan_refusals_write_nothing(L):
    from kanter_core_amd import _lib
    info = _lib.kc_preview_plan_info()
    info.passes = 77
    bad = [(0, 8, 0, 0, 0, 1, 1), (8, 0, 0, 0, 0, 1, 1),  # a zero size
           (8, 8, 4, 0, 0, 1, 1), (130, 70, 8, 0, 0, 1, 1),  # a level at or above L
           (8, 8, 1, 0, 0, 0, 1), (8, 8, 1, 0, 0, 1, 0),  # an empty rect
           (8, 8, 1, 4, 0, 1, 1), (8, 8, 1, 0, 4, 1, 1), (8, 8, 1, 3, 0, 2, 1), (8, 8, 1, 0, 3, 1, 2),  # one texel outside the level
           (8, 8, 0, 0xffffffff, 0, 2, 1)]  # x + width wraps in 32 bits
    for args in bad:
        assert L.kc_preview_plan(*args, C.byref(info)) == KC_ERR_INVALID_ARG, args
    assert L.kc_preview_plan(8, 8, 1, 0, 0, 4, 4, None) == KC_ERR_INVALID_ARG
    assert info.passes == 77
    assert L.kc_preview_plan(8, 8, 1, 0, 0, 4, 4, C.byref(info)) == KC_OK and info.passes == 1


def test_entries_check_arguments_then_the_device(L):
    from kanter_core_amd import _lib
    Req = _lib.kc_preview_request
    img = C.c_void_p(1 << 20)  # never looked at: every call below is refused before it would be
    buf = (C.c_uint8 * 256)(*([0xA5] * 256))
    ids = (C.c_uint32 * 1)(0)
    lg = C.c_void_p(1 << 21)

    def one(level=0, x=0, y=0, w=4, h=4, off=0, pitch=16, image=img):
        return (Req * 1)(Req(image, level, x, y, w, h, off, pitch))

    ok = one()
    # 1. unknown flag bits
    for flags in (2, 4, 0x80000001):
        assert L.kc_image_previews(ok, 1, flags, buf, 256) == KC_ERR_UNSUPPORTED
        assert L.kc_image_previews_device(ok, 1, flags, buf, 256, None) == KC_ERR_UNSUPPORTED
        assert L.kc_live_graph_buffer_previews(lg, ids, ids, ok, 1, flags, buf, 256) == KC_ERR_UNSUPPORTED
    # 2. NULL arguments, the count, and everything a request says without its image
    assert L.kc_image_previews(None, 1, 0, buf, 256) == KC_ERR_INVALID_ARG
    assert L.kc_image_previews(ok, 1, 0, None, 256) == KC_ERR_INVALID_ARG
    assert L.kc_image_previews(None, 0, 0, None, 0) == KC_ERR_INVALID_ARG  # also with count == 0
    assert L.kc_image_previews_device(ok, 1, PREVIEW_SRGB, None, 256, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_previews_device(ok, 1, 0, C.c_void_p((1 << 20) + 2), 256, None) == KC_ERR_INVALID_ARG  # not a multiple of 4
    assert L.kc_live_graph_buffer_previews(None, ids, ids, ok, 1, 0, buf, 256) == KC_ERR_INVALID_ARG
    assert L.kc_live_graph_buffer_previews(lg, None, ids, ok, 1, 0, buf, 256) == KC_ERR_INVALID_ARG
    assert L.kc_live_graph_buffer_previews(lg, ids, None, ok, 1, 0, buf, 256) == KC_ERR_INVALID_ARG
    many = (Req * 4097)(*([Req(img, 0, 0, 0, 1, 1, 0, 4)] * 4097))
    assert L.kc_image_previews(many, 4097, 0, buf, 256) == KC_ERR_INVALID_ARG
    assert L.kc_image_previews_device(many, 4097, 0, buf, 256, None) == KC_ERR_INVALID_ARG
    for r in (one(image=None), one(w=0), one(h=0), one(pitch=12), one(pitch=18), one(off=2), one(off=196),  # 196 + 3 * 16 + 16 > 256
              one(off=(1 << 64) - 4), one(h=1 << 31, pitch=1 << 40)):
        assert L.kc_image_previews(r, 1, PREVIEW_SRGB, buf, 256) == KC_ERR_INVALID_ARG
        assert L.kc_image_previews_device(r, 1, 0, buf, 256, None) == KC_ERR_INVALID_ARG
    for r in (one(w=0), one(pitch=12), one(off=2), one(off=196)):  # the live-graph form ignores the image field, not the rest
        assert L.kc_live_graph_buffer_previews(lg, ids, ids, r, 1, 0, buf, 256) == KC_ERR_INVALID_ARG
    # count == 0 is KC_OK and needs no device
    assert L.kc_image_previews(ok, 0, 0, buf, 256) == KC_OK
    assert L.kc_image_previews_device(ok, 0, PREVIEW_SRGB, buf, 256, None) == KC_OK
    # 3. then the device (this suite also runs where another test has initialised one: the fake image stays untouched there)
    if not L.kc_is_initialized():
        assert L.kc_image_previews(ok, 1, 0, buf, 256) == KC_ERR_NO_DEVICE
        assert L.kc_image_previews(one(off=192), 1, PREVIEW_SRGB, buf, 256) == KC_ERR_NO_DEVICE  # the last byte is the buffer's last
        assert L.kc_image_previews_device(ok, 1, 0, C.c_void_p(1 << 20), 256, None) == KC_ERR_NO_DEVICE
        assert L.kc_live_graph_buffer_previews(lg, ids, ids, one(image=None), 1, 0, buf, 256) == KC_ERR_NO_DEVICE
    assert bytes(buf) == b"\xa5" * 256  # nothing was written


def test_python_names():
    import kanter_core_amd as kc
    from kanter_core_amd import _lib, api
    for name in ("kc_image_previews", "kc_image_previews_device", "kc_live_graph_buffer_previews", "kc_preview_plan"):
        assert name in _lib.SIGNATURES
    for name in ("previews", "previews_torch", "preview_plan", "PreviewPlan", "PREVIEW_SRGB"):
        assert getattr(kc, name) is getattr(api, name)
    assert callable(kc.SlotImage.preview) and callable(kc.LiveGraph.buffer_previews)
    assert kc.PREVIEW_SRGB == 1
    with pytest.raises(kc.TexProError) as e:
        api.preview_plan(8, 8, 4)
    assert e.value.code == KC_ERR_INVALID_ARG
