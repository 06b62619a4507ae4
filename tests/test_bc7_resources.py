"""Build-time guard for the BC7 kernel (csrc/bc7.hip): the four instantiations of bc7_encode_kernel -- linear and sRGB, each in
both cache policies -- keep zero scratch and stay within 128 VGPRs, four waves per SIMD.  The kernel holds 32 packed texel
words and up to 32 search keys through the encoder; the cross-compile reports 125 (see DESIGN)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VGPR_BUDGET = 128


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    from kanter_core_amd import build as kbuild
    hipcc = kbuild._hipcc()
    if shutil.which(hipcc) is None and not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    assert "bc7.hip" in kbuild.SOURCES and "bc_blocks.h" in kbuild.HEADERS
    tmp = tmp_path_factory.mktemp("bc7_res")
    src = os.path.join(ROOT, "kanter_core_amd", "csrc", "bc7.hip")
    cmd = [hipcc] + kbuild.FLAGS + kbuild.DEVICE_FLAGS + ["-x", "hip", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                                                          "-o", str(tmp / "bc7.o")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    table, name = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            table[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            table[name][m.group(1).split()[0]] = int(m.group(2))
    return {k: v for k, v in table.items() if "bc7_encode_kernel" in k}


def test_every_instantiation_is_there(usage):
    # bc7_encode_kernel<SRGB, NT>: ILb0ELb0E, ILb0ELb1E, ILb1ELb0E, ILb1ELb1E
    assert sorted(re.search(r"bc7_encode_kernelILb(\d)ELb(\d)E", k).groups() for k in usage) == [
        ("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")]


def test_no_scratch_and_register_budget(usage):
    assert len(usage) == 4
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0, (name, u)
        assert u["VGPRs"] <= VGPR_BUDGET, (name, u)
