"""Build-time guard for the alpha-coverage kernels (csrc/mip_coverage.hip): the unit is part of the build, its three kernels --
the count pass of the radix select, the pick between the passes and the scale -- are there, keep zero scratch (the job table in
the launch's arguments is indexed without a private copy) and stay within 64 VGPRs, the occupancy step of eight waves per SIMD."""
import pytest

from util import kernel_resource_usage

KERNELS = ["coverage_count_kernel", "coverage_pick_kernel", "coverage_scale_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return kernel_resource_usage("mip_coverage.hip", tmp_path_factory.mktemp("mip_coverage_res"))


def test_the_unit_is_part_of_the_build():
    from kanter_core_amd import build as kbuild
    assert "mip_coverage.hip" in kbuild.SOURCES and "mip.cpp" in kbuild.SOURCES and "mip_export.cpp" in kbuild.SOURCES
    assert "streaming.h" in kbuild.HEADERS  # hist_add, which the count pass shares with stats.hip


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_kernel_is_there_once(usage, kernel):
    assert len([k for k in usage if kernel in k]) == 1, sorted(usage)


def test_no_scratch_and_register_budget(usage):
    seen = 0
    for name, u in usage.items():
        if not any(k in name for k in KERNELS):
            continue
        seen += 1
        assert u.get("ScratchSize", 0) == 0, (name, u)
        assert u["VGPRs"] <= 64, (name, u)
    assert seen == 3
