"""Build-time guard for the all-modes decode and compare kernels (csrc/bc_modes.hip): every instantiation is in the
cross-compile's resource remarks with zero scratch, and each kernel stays under the VGPR count of the occupancy step just above
what the compiler reports (gfx950: 512 VGPRs a SIMD in steps of 8, so 80 is six waves, 128 four, 168 three).

    kernel                                   reported     budget
    bc7_modes_decode_kernel   <NT>           109          128  (four waves, the step of bc_decode_kernel's BC7 form at 111 / 115)
    bc6h_modes_decode_kernel  <NT>           77           80   (six waves; bc6h_decode_kernel: 43 / 47)
    bc7_modes_compare_kernel  <SRGB, NT>     151 / 153    168  (three waves; 153 with sRGB.  bc_compare_kernel's BC7 form holds
                                                                sixteen decoded words beside the 32 source words and sits at
                                                                198 / 199, two waves)
    bc6h_modes_compare_kernel <NT>           110          128  (four waves; bc6h_compare_kernel: 87, five waves)

Zero scratch is a condition of its own: the decoders keep a block's state in a struct and pick words of it by per-lane
positions, and a conditional between two members compiled to a choice of addresses once, which put the whole state in scratch
(bc_modes.h reads the members into values first).
"""
import re

import pytest

from util import kernel_resource_usage

BUDGET = {"bc7_modes_decode_kernel": 128, "bc6h_modes_decode_kernel": 80, "bc7_modes_compare_kernel": 168, "bc6h_modes_compare_kernel": 128}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    from kanter_core_amd import build as kbuild
    assert "bc_modes.hip" in kbuild.SOURCES and "bc_modes.h" in kbuild.HEADERS
    return kernel_resource_usage("bc_modes.hip", tmp_path_factory.mktemp("bc_modes_res"))


def test_every_instantiation_is_there_without_scratch_and_within_its_step(usage):
    found = {}
    for name, u in usage.items():
        m = re.search(r"(bc7|bc6h)_modes_(decode|compare)_kernelI((?:Lb\dE)+)E", name)
        if m:
            kernel = "%s_modes_%s_kernel" % (m.group(1), m.group(2))
            found[(kernel, tuple(int(v) for v in re.findall(r"Lb(\d)E", m.group(3))))] = u
    want = {("bc7_modes_decode_kernel", (nt,)) for nt in (0, 1)} | {("bc6h_modes_decode_kernel", (nt,)) for nt in (0, 1)}
    want |= {("bc7_modes_compare_kernel", (s, nt)) for s in (0, 1) for nt in (0, 1)} | {("bc6h_modes_compare_kernel", (nt,)) for nt in (0, 1)}
    assert set(found) == want
    assert len([k for k in usage if "_modes_" in k]) == len(want)  # and nothing else of the family
    for (kernel, args), u in found.items():
        assert u.get("ScratchSize", 0) == 0, (kernel, args, u)
        assert u["VGPRs"] <= BUDGET[kernel], (kernel, args, u)
