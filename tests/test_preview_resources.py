"""Build-time guard for the preview kernel (csrc/preview.hip): the four instantiations (sRGB x cache policy) of preview_kernel are
there, keep zero scratch memory and stay within the 64 VGPRs at which a 256-thread workgroup still reaches the occupancy of
mip_pyramid_kernel (8 waves per SIMD), like the other streaming exporters."""
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
    tmp = tmp_path_factory.mktemp("preview_res")
    src = os.path.join(ROOT, "kanter_core_amd", "csrc", "preview.hip")
    cmd = [hipcc] + kbuild.FLAGS + kbuild.DEVICE_FLAGS + ["-x", "hip", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                                                          "-o", str(tmp / "preview.o")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    table, name = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            table[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            table[name][m.group(1).split()[0]] = int(m.group(2))
    return table


def test_the_unit_is_part_of_the_build():
    from kanter_core_amd import build as kbuild
    assert "preview.hip" in kbuild.SOURCES and "preview.cpp" in kbuild.SOURCES and "preview_walk.h" in kbuild.HEADERS
    assert kbuild.object_name("preview.hip") != kbuild.object_name("preview.cpp")


def test_every_instantiation_is_there(usage):
    names = [k for k in usage if "preview_kernel" in k]
    assert len(names) == 4, names  # SRGB x NT
    assert {re.search(r"preview_kernelILb(\d)ELb(\d)E", n).groups() for n in names} == {("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")}


def test_no_scratch_and_register_budget(usage):
    seen = 0
    for name, u in usage.items():
        if "preview_kernel" not in name:
            continue
        seen += 1
        assert u.get("ScratchSize", 0) == 0, (name, u)
        assert u["VGPRs"] <= 64, (name, u)
        assert u["Occupancy"] == 8, (name, u)
    assert seen == 4
