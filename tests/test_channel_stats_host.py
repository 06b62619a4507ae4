"""kc_image_channel_stats / kc_live_graph_buffer_channel_stats without a device: the symbols are exported, the ctypes struct has the
header's layout (checked against a C program compiled from the header), the Rust binding declares it, and the argument checks
return their codes before the device check."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from kanter_core_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KC_OK, KC_ERR_NO_DEVICE, KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 0, 101, 102, 104
HIST, SRGB = 1, 2


def test_symbols_exported():
    L = _lib.load()
    for name in ("kc_image_channel_stats", "kc_live_graph_buffer_channel_stats"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES


def test_struct_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    src = tmp_path / "layout.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "kanter_core_amd.h"
#define F(m) printf(#m " %zu\\n", offsetof(kc_channel_stats, m))
int main(void)
{
    printf("sizeof %zu\\n", sizeof(kc_channel_stats));
    F(channels); F(flags); F(pixels); F(min); F(max); F(nan_count); F(histogram);
    printf("KC_STATS_HISTOGRAM %u\\nKC_STATS_SRGB %u\\n", KC_STATS_HISTOGRAM, KC_STATS_SRGB);
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    S = _lib.kc_channel_stats
    assert int(got["sizeof"]) == C.sizeof(S) == 8 + 8 + 16 + 16 + 32 + 4 * 256 * 8
    for f, _ in S._fields_:
        assert int(got[f]) == getattr(S, f).offset, f
    assert int(got["KC_STATS_HISTOGRAM"]) == HIST and int(got["KC_STATS_SRGB"]) == SRGB


def test_rust_binding_declares_the_struct():
    rs = open(os.path.join(ROOT, "bindings", "rust", "kanter_core_amd_sys.rs")).read()
    m = re.search(r"pub struct KcChannelStats \{(.*?)\}", rs, re.S)
    assert m, "KcChannelStats missing"
    fields = re.findall(r"pub (\w+): ([^,]+),", m.group(1))
    assert fields == [("channels", "u32"), ("flags", "u32"), ("pixels", "u64"), ("min", "[f32; 4]"), ("max", "[f32; 4]"),
                      ("nan_count", "[u64; 4]"), ("histogram", "[[u64; 256]; 4]")]
    assert "pub const KC_STATS_HISTOGRAM: u32 = 1;" in rs and "pub const KC_STATS_SRGB: u32 = 2;" in rs
    assert re.search(r"pub fn kc_image_channel_stats\(img: \*mut KcImage, flags: u32, out: \*mut KcChannelStats\) -> i32;", rs)
    assert re.search(r"pub fn kc_live_graph_buffer_channel_stats\(lg: \*mut KcLiveGraph, node_id: u32, slot_id: u32, flags: u32, "
                     r"out: \*mut KcChannelStats\) -> i32;", rs)
    backend = open(os.path.join(ROOT, "bindings", "rust", "device_backend.rs")).read()
    assert "kc_image_channel_stats(" in backend


@pytest.fixture
def const_image():
    """A constant Gray image: creating it needs no device (kc_image_from_value keeps the value as a scalar)."""
    L = _lib.load()
    img = C.c_void_p()
    assert L.kc_image_from_value(_lib.kc_size(5, 3), C.c_float(0.25), 0, C.byref(img)) == KC_OK
    yield img
    L.kc_image_release(img)


def sentinel():
    s = _lib.kc_channel_stats()
    s.channels, s.pixels = 0xdead, 0xbeef
    return s


def untouched(s):
    return s.channels == 0xdead and s.pixels == 0xbeef


def test_argument_checks_before_the_device(const_image):
    L = _lib.load()
    s = sentinel()
    assert L.kc_image_channel_stats(None, 0, C.byref(s)) == KC_ERR_INVALID_ARG
    assert L.kc_image_channel_stats(const_image, 0, None) == KC_ERR_INVALID_ARG
    for bad in (4, 8, 0x80000000, HIST | 4):
        assert L.kc_image_channel_stats(const_image, bad, C.byref(s)) == KC_ERR_UNSUPPORTED, bad
    assert L.kc_image_channel_stats(const_image, SRGB, C.byref(s)) == KC_ERR_INVALID_ARG
    assert untouched(s)
    assert L.kc_live_graph_buffer_channel_stats(None, 0, 0, 0, C.byref(s)) == KC_ERR_INVALID_ARG
    assert untouched(s)


@pytest.mark.parametrize("flags", [0, HIST, HIST | SRGB])
def test_valid_flags_reach_the_device_check(const_image, flags):
    L = _lib.load()
    s = sentinel()
    st = L.kc_image_channel_stats(const_image, flags, C.byref(s))
    if L.kc_is_initialized():  # a GPU suite in the same process: a constant image is answered without a launch
        assert st == KC_OK
        assert s.channels == 1 and s.pixels == 15 and s.min[0] == 0.25 and s.max[0] == 0.25
    else:
        assert st == KC_ERR_NO_DEVICE
        assert untouched(s)
