"""Build-time guard for the blur kernels (csrc/blur.hip): the four instantiations (cache policy, wrap) of blur_rows_kernel and of
blur_columns_kernel are there and nothing else, every one keeps zero scratch -- a lane's two windows of four taps and its four
sums stay registers because the loop over the pairs shifts them by name, never by index -- and stays on the occupancy step the
compiler put it on.

The compiler reports 33 to 40 VGPRs for blur_rows_kernel (40 with wrap and plain loads: the modulo of the halo staging) and 58 for
every blur_columns_kernel (two windows of four quads, four quads of sums): all on the step that ends at 64 VGPRs, eight waves
per SIMD; the bound is 64.  LDS: blur_rows_kernel 6656 bytes per workgroup (4 rows of four sub-arrays of 104 floats);
blur_columns_kernel (64 + 2 R) rows of 256 bytes, sized by the launch: 16896 bytes at R = 1, 49152 at R = 64, three workgroups
per CU."""
import re

import pytest

from util import kernel_resource_usage

KERNELS = {"blur_rows_kernel": 64, "blur_columns_kernel": 64}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return kernel_resource_usage("blur.hip", tmp_path_factory.mktemp("blur_res"))


def test_the_units_are_part_of_the_build():
    from kanter_core_amd import build as kbuild
    assert "blur.hip" in kbuild.SOURCES and "blur.cpp" in kbuild.SOURCES and "streaming.h" in kbuild.HEADERS
    assert kbuild.object_name("blur.hip") != kbuild.object_name("blur.cpp")


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_every_instantiation_is_there(usage, kernel):
    names = [k for k in usage if kernel in k]
    assert len(names) == 4, names  # NT, WRAP = false, true
    assert {re.search(kernel + r"ILb(\d)ELb(\d)E", n).groups() for n in names} == {("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")}


def test_and_no_others(usage):
    assert len(usage) == 8 and all(any(k in n for k in KERNELS) for n in usage), sorted(usage)


def test_no_scratch_and_register_budgets(usage):
    for name, u in usage.items():
        print(name, u)
        assert u.get("ScratchSize", 0) == 0, (name, u)
        assert u["VGPRs"] <= next(b for k, b in KERNELS.items() if k in name), (name, u)
