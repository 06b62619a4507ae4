"""Build-time guard for the punch-through BC1 unit (csrc/bc1a.hip): every instantiation of bc1a_encode_kernel and
bc1a_compare_kernel -- linear and sRGB, each in both cache policies -- is there and keeps zero scratch, within the register step
(gfx950 allocates VGPRs in steps of 8) just above what the compiler reports: 127 VGPRs for the four encoders (budget 128, four
waves a SIMD; capped at 96 or 80 the sRGB forms spill, see DESIGN), 101 (linear) and 102 (sRGB) for the comparisons (budget 104)."""
import re

import pytest

from util import kernel_resource_usage


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return kernel_resource_usage("bc1a.hip", tmp_path_factory.mktemp("bc1a_res"))


def forms(usage, kernel):
    """{(srgb, nt): usage} of the instantiations of a kernel template <bool SRGB, bool NT>"""
    out = {}
    for name, u in usage.items():
        m = re.search(kernel + r"ILb([01])ELb([01])E", name)
        if m:
            out[(int(m.group(1)), int(m.group(2)))] = u
    return out


@pytest.mark.parametrize("kernel,budget", [("bc1a_encode_kernel", 128), ("bc1a_compare_kernel", 104)])
def test_every_instantiation_without_scratch_and_within_budget(usage, kernel, budget):
    got = forms(usage, kernel)
    assert sorted(got) == [(0, 0), (0, 1), (1, 0), (1, 1)], sorted(got)
    for form, u in got.items():
        assert u.get("ScratchSize", 0) == 0, (kernel, form, u)
        assert u["VGPRs"] <= budget, (kernel, form, u)


def test_the_unit_holds_no_other_kernel(usage):
    assert all("bc1a_encode_kernel" in k or "bc1a_compare_kernel" in k for k in usage), sorted(usage)
    assert not any("bc_encode_kernel" in k or "bc_compare_kernel" in k for k in usage)  # the guards of bc.hip and bc_decode.hip count those
