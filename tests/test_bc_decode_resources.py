"""Build-time guard for the decode and compare kernels (csrc/bc_decode.hip): every instantiation is in the cross-compile's
resource remarks with zero scratch, and each family stays under the VGPR count of the occupancy step just above what the
compiler reports (gfx950: 512 VGPRs a SIMD in steps of 8, so 128 is four waves, 168 three, 256 two).

    kernel                               reported     budget
    bc_decode_kernel  BC1 BC3 BC4 BC5    34 39 36 39  64   (eight waves)
    bc_decode_kernel  BC7                111 / 115    128  (four waves; 115 with the count)
    bc_compare_kernel BC4 / BC5          53 / 69      64 / 72  (eight and seven waves)
    bc_compare_kernel BC1                89 / 90      96   (five waves; 90 with sRGB)
    bc_compare_kernel BC3                115 / 116    128  (four waves; 116 with sRGB)
    bc_compare_kernel BC7                198 / 199    256  (two waves: the 32 source words, the 16 decoded words and the
                                                            three modes' fields together; see DESIGN)
"""
import re

import pytest

from util import kernel_resource_usage

BC7 = 98
DECODE_BUDGET = {1: 64, 3: 64, 4: 64, 5: 64, BC7: 128}
COMPARE_BUDGET = {1: 96, 3: 128, 4: 64, 5: 72, BC7: 256}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    from kanter_core_amd import build as kbuild
    assert "bc_decode.cpp" in kbuild.SOURCES
    return kernel_resource_usage("bc_decode.hip", tmp_path_factory.mktemp("bc_decode_res"))


def instances(usage, kernel):
    """{(fmt, flag, flag): usage} of kernel<FMT, bool, bool>"""
    out = {}
    for k, v in usage.items():
        m = re.search(kernel + r"ILi(\d+)ELb(\d)ELb(\d)E", k)
        if m:
            out[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = v
    return out


def test_every_decode_instantiation(usage):
    # bc_decode_kernel<FMT, NT, COUNT>: every format in both cache policies, BC7 also with the count
    got = instances(usage, "bc_decode_kernel")
    want = {(f, nt, 0) for f in (1, 3, 4, 5, BC7) for nt in (0, 1)} | {(BC7, nt, 1) for nt in (0, 1)}
    assert set(got) == want
    for (fmt, _, _), u in got.items():
        assert u.get("ScratchSize", 0) == 0, (fmt, u)
        assert u["VGPRs"] <= DECODE_BUDGET[fmt], (fmt, u)


def test_every_compare_instantiation(usage):
    # bc_compare_kernel<FMT, SRGB, NT>: sRGB for the formats with colour
    got = instances(usage, "bc_compare_kernel")
    want = {(f, s, nt) for f in (1, 3, BC7) for s in (0, 1) for nt in (0, 1)} | {(f, 0, nt) for f in (4, 5) for nt in (0, 1)}
    assert set(got) == want
    for (fmt, _, _), u in got.items():
        assert u.get("ScratchSize", 0) == 0, (fmt, u)
        assert u["VGPRs"] <= COMPARE_BUDGET[fmt], (fmt, u)


def test_the_combine_kernel(usage):
    got = [v for k, v in usage.items() if "bc_combine_kernel" in k]
    assert len(got) == 1 and got[0].get("ScratchSize", 0) == 0 and got[0]["VGPRs"] <= 32
