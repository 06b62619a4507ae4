"""Build-time guard for the mip kernels (csrc/mip.hip): both instantiations (cache policies) of mip_pyramid_kernel and of
mip_level_kernel are there, keep zero scratch and stay within 64 VGPRs like the other streaming exporters."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    from kanter_core_amd import build as kbuild
    hipcc = kbuild._hipcc()
    if shutil.which(hipcc) is None and not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("mip_res")
    src = os.path.join(ROOT, "kanter_core_amd", "csrc", "mip.hip")
    cmd = [hipcc] + kbuild.FLAGS + kbuild.DEVICE_FLAGS + ["-x", "hip", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                                                          "-o", str(tmp / "mip.o")]
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
    return table


def test_the_unit_is_part_of_the_build():
    from kanter_core_amd import build as kbuild
    assert "mip.hip" in kbuild.SOURCES and "mip.cpp" in kbuild.SOURCES and "mip_export.cpp" in kbuild.SOURCES


@pytest.mark.parametrize("kernel", ["mip_pyramid_kernel", "mip_level_kernel"])
def test_every_instantiation_is_there(usage, kernel):
    names = [k for k in usage if kernel in k]
    assert len(names) == 2, names  # NT = false, true
    assert {re.search(kernel + r"ILb(\d)E", n).group(1) for n in names} == {"0", "1"}


def test_no_scratch_and_register_budget(usage):
    seen = 0
    for name, u in usage.items():
        if "mip_pyramid_kernel" not in name and "mip_level_kernel" not in name:
            continue
        seen += 1
        assert u.get("ScratchSize", 0) == 0, (name, u)
        assert u["VGPRs"] <= 64, (name, u)
    assert seen == 4
