"""Device-memory image descriptors without a device: kc_device_image_validate's arithmetic (exact extents, refusals) and the
pure tensor -> descriptor mapping of the Python API (device_image_desc), on CPU tensors.  Nothing here dereferences a pointer:
the addresses are made up."""
import ctypes as C

import pytest

from kanter_core_amd import _lib

KC_ERR_INVALID_ARG, KC_ERR_NO_DEVICE = 102, 101
U8, U16, F16, BF16, F32 = range(5)
HWC, CHW = 0, 1
BASE = 0x7f0000000000  # a made-up, 256-byte aligned address


def desc(w, h, c, dtype, layout, row, chan=0, ptr=BASE):
    return _lib.kc_device_image(ptr, w, h, c, dtype, layout, row, chan)


def validate(d):
    """-> (status, extent or None when the call left it untouched)"""
    L = _lib.load()
    ext = C.c_size_t(0xdeadbeef)
    s = L.kc_device_image_validate(C.byref(d), C.byref(ext))
    return s, (None if ext.value == 0xdeadbeef else ext.value)


def arith_ok_status():
    # the arithmetic passed: without kc_init the device check cannot run (NoDevice); once initialised (a GPU suite in the same
    # process), a made-up address is not device memory (InvalidArgument) -- the extent is written either way
    return KC_ERR_INVALID_ARG if _lib.load().kc_is_initialized() else KC_ERR_NO_DEVICE


@pytest.mark.parametrize("d, extent", [
    (desc(33, 17, 4, U8, HWC, 33 * 4), 17 * 33 * 4),
    (desc(33, 17, 3, U8, HWC, 128), 16 * 128 + 33 * 3),                       # padded rows
    (desc(5, 1, 1, U16, HWC, 10), 10),
    (desc(5, 7, 2, F16, HWC, 64), 6 * 64 + 5 * 2 * 2),
    (desc(100, 9, 4, BF16, HWC, 100 * 8), 9 * 100 * 8),
    (desc(100, 9, 4, F32, HWC, 2048), 8 * 2048 + 100 * 16),
    (desc(33, 17, 4, F32, CHW, 33 * 4, 17 * 33 * 4), 3 * 17 * 33 * 4 + 16 * 33 * 4 + 33 * 4),
    (desc(33, 17, 3, F16, CHW, 128, 17 * 128 + 512), 2 * (17 * 128 + 512) + 16 * 128 + 66),  # padded rows, gaps between planes
    (desc(8, 8, 1, U8, CHW, 8, 0), 7 * 8 + 8),                                # one plane: the channel pitch is not used
    (desc(1, 1, 2, U16, CHW, 2, 2), 2 + 2),
])
def test_extent_is_exact_before_init(d, extent):
    s, ext = validate(d)
    assert s == arith_ok_status(), _lib.load().kc_last_error()
    assert ext == extent


@pytest.mark.parametrize("d, why", [
    (desc(4, 4, 0, U8, HWC, 16), "channels 0"),
    (desc(4, 4, 5, U8, HWC, 20), "channels 5"),
    (desc(4, 4, 4, 5, HWC, 64), "unknown dtype"),
    (desc(4, 4, 4, -1, HWC, 64), "negative dtype"),
    (desc(4, 4, 4, U8, 2, 16), "unknown layout"),
    (desc(4, 4, 1, U16, HWC, 8, ptr=BASE + 1), "misaligned pointer"),
    (desc(4, 4, 1, F32, HWC, 16, ptr=BASE + 2), "misaligned pointer (f32)"),
    (desc(4, 4, 1, F16, HWC, 9), "misaligned row pitch"),
    (desc(4, 4, 2, F32, CHW, 16, 66), "misaligned channel pitch"),
    (desc(4, 4, 4, U8, HWC, 15), "row pitch too small (hwc)"),
    (desc(4, 4, 3, F32, HWC, 44), "row pitch too small (hwc f32)"),
    (desc(4, 4, 2, F16, CHW, 6, 64), "row pitch too small (chw)"),
    (desc(4, 4, 2, F32, CHW, 16, 60), "overlapping planes"),
    (desc(4, 4, 3, U8, CHW, 8, 31), "overlapping planes (padded rows)"),
    (desc(0, 4, 1, U8, HWC, 4), "zero width"),
    (desc(4, 0, 1, U8, HWC, 4), "zero height"),
    (desc(4, 4, 1, U8, HWC, 4, ptr=0), "NULL pointer"),
    (desc(4, 1 << 20, 1, U8, HWC, 1 << 60), "extent overflows"),
])
def test_arithmetic_refusals(d, why):
    s, ext = validate(d)
    assert s == KC_ERR_INVALID_ARG, why
    assert ext is None, why  # refused before any extent
    assert _lib.load().kc_last_error()


def test_null_descriptor():
    assert _lib.load().kc_device_image_validate(None, None) == KC_ERR_INVALID_ARG


def test_extent_is_optional():
    assert _lib.load().kc_device_image_validate(C.byref(desc(4, 4, 4, U8, HWC, 16)), None) == arith_ok_status()


# ---- tensor -> descriptor (pure: CPU tensors, no library call)
torch = pytest.importorskip("torch")
from kanter_core_amd.api import device_image_desc  # noqa: E402

DTYPES = [(torch.uint8, U8, 1), (torch.uint16, U16, 2), (torch.float16, F16, 2), (torch.bfloat16, BF16, 2), (torch.float32, F32, 4)]


def fields(d):
    return (d.ptr, d.width, d.height, d.channels, d.dtype, d.layout, d.row_pitch_bytes, d.channel_pitch_bytes)


@pytest.mark.parametrize("tdt, code, e", DTYPES)
def test_mapping_contiguous(tdt, code, e):
    t = torch.zeros((7, 9, 3), dtype=tdt)
    assert fields(device_image_desc(t)) == (t.data_ptr(), 9, 7, 3, code, HWC, 9 * 3 * e, 0)
    t = torch.zeros((2, 7, 9), dtype=tdt)
    assert fields(device_image_desc(t, "chw")) == (t.data_ptr(), 9, 7, 2, code, CHW, 9 * e, 7 * 9 * e)
    t = torch.zeros((7, 9), dtype=tdt)
    assert fields(device_image_desc(t)) == (t.data_ptr(), 9, 7, 1, code, HWC, 9 * e, 0)
    assert fields(device_image_desc(t, "chw")) == (t.data_ptr(), 9, 7, 1, code, CHW, 9 * e, 7 * 9 * e)


@pytest.mark.parametrize("tdt, code, e", DTYPES)
def test_mapping_strided_views(tdt, code, e):
    big = torch.zeros((20, 30, 4), dtype=tdt)
    v = big[3:10, 5:17, :]  # padded rows, offset pointer
    assert fields(device_image_desc(v)) == (big.data_ptr() + (3 * 30 * 4 + 5 * 4) * e, 12, 7, 4, code, HWC, 30 * 4 * e, 0)
    planes = torch.zeros((6, 20, 32), dtype=tdt)
    v = planes[1:6:2, 2:9, 3:19]  # gaps between the planes and inside the rows
    assert fields(device_image_desc(v, "chw")) == (planes.data_ptr() + (20 * 32 + 2 * 32 + 3) * e, 16, 7, 3, code, CHW, 32 * e,
                                                   2 * 20 * 32 * e)
    col = big[:, :, 1:2]  # one channel out of four is not packed
    with pytest.raises(ValueError, match="packed"):
        device_image_desc(col)


def test_mapping_size_one_dims_take_any_stride():
    t = torch.zeros((1, 4, 2), dtype=torch.uint8).expand(1, 4, 2)
    assert fields(device_image_desc(t))[6] == 8
    t = torch.zeros((3, 5, 8), dtype=torch.float32)[:, 2:3, :]  # one row per plane
    d = device_image_desc(t, "chw")
    assert (d.height, d.row_pitch_bytes, d.channel_pitch_bytes) == (1, 32, 5 * 8 * 4)


def test_mapping_refusals():
    with pytest.raises(ValueError, match="packed"):
        device_image_desc(torch.zeros((4, 5, 3), dtype=torch.uint8).permute(1, 0, 2))  # columns not contiguous
    with pytest.raises(ValueError, match="packed"):
        device_image_desc(torch.zeros((3, 4, 5), dtype=torch.uint8).permute(1, 2, 0))  # HWC view of CHW memory
    with pytest.raises(ValueError, match="unit stride"):
        device_image_desc(torch.zeros((3, 4, 10), dtype=torch.float32)[:, :, ::2], "chw")
    with pytest.raises(ValueError, match="unit stride"):
        device_image_desc(torch.zeros((4, 3), dtype=torch.float32).t(), "chw")
    with pytest.raises(ValueError, match="dtype"):
        device_image_desc(torch.zeros((4, 4, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="dtype"):
        device_image_desc(torch.zeros((4, 4, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="channels"):
        device_image_desc(torch.zeros((4, 4, 5), dtype=torch.uint8))
    with pytest.raises(ValueError, match="channels"):
        device_image_desc(torch.zeros((5, 4, 4), dtype=torch.uint8), "chw")
    with pytest.raises(ValueError, match="shape"):
        device_image_desc(torch.zeros((2, 4, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="empty"):
        device_image_desc(torch.zeros((0, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="layout"):
        device_image_desc(torch.zeros((4, 4, 4), dtype=torch.uint8), "nhwc")


def test_mapping_feeds_validation():
    """What the mapping makes of a strided view passes the arithmetic with the view's own extent."""
    big = torch.zeros((20, 30, 4), dtype=torch.float16)
    v = big[3:10, 5:17, :]
    s, ext = validate(device_image_desc(v))
    assert s == arith_ok_status()
    assert ext == (6 * 30 * 4 + 12 * 4) * 2


def test_api_import_leaves_torch_alone():
    import os
    import subprocess
    import sys
    code = "import sys, kanter_core_amd.api; assert 'torch' not in sys.modules"
    subprocess.check_call([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
