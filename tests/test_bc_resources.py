"""Build-time guard for the block-compression kernel (csrc/bc.hip): every instantiation of bc_encode_kernel -- BC1 and BC3 linear
and sRGB, BC4 and BC5, each in both cache policies -- keeps zero scratch.  BC4 and BC5 stay within 64 VGPRs like the other
streaming exporters; BC1 and BC3 hold 32 packed texel words through the encoder and are pinned at their spill-free counts (capped
at 64 they spill to scratch, see DESIGN)."""
import re

import pytest

from util import kernel_resource_usage


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return kernel_resource_usage("bc.hip", tmp_path_factory.mktemp("bc_res"))


def test_every_instantiation_is_there(usage):
    assert len([k for k in usage if "bc_encode_kernel" in k]) == (2 + 2 + 1 + 1) * 2  # (BC1, BC3) x sRGB, BC4, BC5 x policy


def fmt_of(name):
    return int(re.search(r"bc_encode_kernelILi(\d)E", name).group(1))


def test_no_scratch_and_register_budget(usage):
    budget = {1: 72, 3: 96, 4: 64, 5: 64}
    seen = 0
    for name, u in usage.items():
        if "bc_encode_kernel" not in name:
            continue
        seen += 1
        assert u.get("ScratchSize", 0) == 0, (name, u)
        assert u["VGPRs"] <= budget[fmt_of(name)], (name, u)
    assert seen == 12
