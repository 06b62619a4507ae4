"""Build-time guard for the distance-field kernels (csrc/sdf.hip): the four instantiations (cache policy, wrap) of
sdf_columns_kernel and of sdf_rows_kernel are there and nothing else, every one keeps zero scratch -- the columns kernel holds a
band's classes as a 64-bit mask and the down sweep's 64 distances as bytes in 16 registers, which stay registers only while every
index is static -- and stays on the occupancy step the compiler put it on.

The compiler reports 90 VGPRs for sdf_columns_kernel (all 64 row loads of a band are in flight at once, one register each):
five waves per SIMD, the step that ends at 96 VGPRs; the bound is 96.  sdf_rows_kernel takes 55 VGPRs with wrap (the modulo of the
staging) and fewer without: eight waves per SIMD, the step that ends at 64; the bound is 64.  Its LDS is 12224 bytes per
workgroup (4 rows, two images each, of 256 + 2 * 254 words), far from limiting eight waves."""
import re

import pytest

from util import kernel_resource_usage

KERNELS = {"sdf_columns_kernel": 96, "sdf_rows_kernel": 64}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return kernel_resource_usage("sdf.hip", tmp_path_factory.mktemp("sdf_res"))


def test_the_units_are_part_of_the_build():
    from kanter_core_amd import build as kbuild
    assert "sdf.hip" in kbuild.SOURCES and "sdf.cpp" in kbuild.SOURCES and "streaming.h" in kbuild.HEADERS
    assert kbuild.object_name("sdf.hip") != kbuild.object_name("sdf.cpp")


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
