"""Build-time guard for the BC6H kernels (csrc/bc6h.hip): every instantiation keeps zero scratch; the encoder, in both cache
policies, stays within 128 VGPRs, four waves per SIMD and BC7's budget (it holds 32 texel words and 32 words of the search; the
cross-compile reports 111); the decoder (43, 47 with the count) stays within 64, eight waves, and the comparison (87) within 96,
five waves: the occupancy step above what the cross-compile reports (see DESIGN)."""
import re

import pytest

from util import kernel_resource_usage

VGPR_BUDGET = {"bc6h_encode_kernel": 128, "bc6h_decode_kernel": 64, "bc6h_compare_kernel": 96}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return {k: v for k, v in kernel_resource_usage("bc6h.hip", tmp_path_factory.mktemp("bc6h_res")).items() if "bc6h_" in k}


def test_every_instantiation_is_there(usage):
    # bc6h_encode_kernel<NT>, bc6h_decode_kernel<NT, COUNT>, bc6h_compare_kernel<NT>
    found = sorted((m.group(1), tuple(re.findall(r"Lb(\d)E", m.group(2)))) for m in
                   (re.search(r"(bc6h_\w+_kernel)I((?:Lb\dE)+)E", k) for k in usage))
    assert found == [("bc6h_compare_kernel", ("0",)), ("bc6h_compare_kernel", ("1",)),
                     ("bc6h_decode_kernel", ("0", "0")), ("bc6h_decode_kernel", ("0", "1")),
                     ("bc6h_decode_kernel", ("1", "0")), ("bc6h_decode_kernel", ("1", "1")),
                     ("bc6h_encode_kernel", ("0",)), ("bc6h_encode_kernel", ("1",))]


def test_no_scratch_and_register_budgets(usage):
    assert len(usage) == 8
    for name, u in usage.items():
        kernel = re.search(r"bc6h_\w+_kernel", name).group(0)
        assert u.get("ScratchSize", 0) == 0, (name, u)
        assert u["VGPRs"] <= VGPR_BUDGET[kernel], (name, u)
