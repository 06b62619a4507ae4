"""Build-time guard for the alpha-weighted chain kernels (csrc/mip_alpha.hip): all four instantiations (cache policy, first launch
or state planes) of alpha_pull_pyramid_kernel and of alpha_pull_level_kernel and the one alpha_push_kernel are there, keep zero
scratch, and stay within their register budgets: 128 VGPRs for the pull -- four channels of four 16-byte rows are 64 VGPRs of
tile, so the step of eight waves (64) is out of reach with all sixteen loads up front -- and 64 for the push, which holds a quad
of weights and a few indices and should run eight waves per SIMD to hide its dependent loads."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PULL = ["alpha_pull_pyramid_kernel", "alpha_pull_level_kernel"]
PUSH = "alpha_push_kernel"


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    from kanter_core_amd import build as kbuild
    hipcc = kbuild._hipcc()
    if shutil.which(hipcc) is None and not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("mip_alpha_res")
    src = os.path.join(ROOT, "kanter_core_amd", "csrc", "mip_alpha.hip")
    cmd = [hipcc] + kbuild.FLAGS + kbuild.DEVICE_FLAGS + ["-x", "hip", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                                                          "-o", str(tmp / "mip_alpha.o")]
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
    assert "mip_alpha.hip" in kbuild.SOURCES and "mip_steps.h" in kbuild.HEADERS


def test_the_names_stay_apart_from_the_other_mip_kernels(usage):
    assert not [k for k in usage if "mip_pyramid_kernel" in k or "mip_level_kernel" in k or "normal_" in k or "roughness_" in k or "coverage_" in k]
    assert len(usage) == 9, sorted(usage)


@pytest.mark.parametrize("kernel", PULL)
def test_every_instantiation_is_there(usage, kernel):
    names = [k for k in usage if kernel in k]
    assert len(names) == 4, names  # NT, FIRST = false, true
    assert {re.search(kernel + r"ILb(\d)ELb(\d)E", n).groups() for n in names} == {("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")}


def test_the_push_is_one_kernel(usage):
    assert len([k for k in usage if PUSH in k]) == 1


def test_no_scratch_and_register_budgets(usage):
    seen = 0
    for name, u in usage.items():
        seen += 1
        print(name, u)
        assert u.get("ScratchSize", 0) == 0, (name, u)
        assert u["VGPRs"] <= (64 if PUSH in name else 128), (name, u)
    assert seen == 9
