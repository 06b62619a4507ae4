"""Build-time guard for the BC7 kernel (csrc/bc7.hip): the four instantiations of bc7_encode_kernel -- linear and sRGB, each in
both cache policies -- keep zero scratch and stay within 128 VGPRs, four waves per SIMD.  The kernel holds 32 packed texel
words and up to 32 search keys through the encoder; the cross-compile reports 125 (see DESIGN)."""
import re

import pytest

from util import kernel_resource_usage

VGPR_BUDGET = 128


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return {k: v for k, v in kernel_resource_usage("bc7.hip", tmp_path_factory.mktemp("bc7_res")).items() if "bc7_encode_kernel" in k}


def test_every_instantiation_is_there(usage):
    # bc7_encode_kernel<SRGB, NT>: ILb0ELb0E, ILb0ELb1E, ILb1ELb0E, ILb1ELb1E
    assert sorted(re.search(r"bc7_encode_kernelILb(\d)ELb(\d)E", k).groups() for k in usage) == [
        ("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")]


def test_no_scratch_and_register_budget(usage):
    assert len(usage) == 4
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0, (name, u)
        assert u["VGPRs"] <= VGPR_BUDGET, (name, u)
