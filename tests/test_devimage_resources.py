"""Build-time guard for the device-memory image kernels (csrc/devimage.hip): every instantiation of image_import_kernel and
image_export_kernel -- five element types, two layouts, both cache policies, sRGB for U8 -- keeps zero scratch and at most
64 VGPRs (8 waves per SIMD: they are HBM-bound streams and need the loads in flight)."""
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
    tmp = tmp_path_factory.mktemp("devimage_res")
    src = os.path.join(ROOT, "kanter_core_amd", "csrc", "devimage.hip")
    cmd = [hipcc] + kbuild.FLAGS + kbuild.DEVICE_FLAGS + ["-x", "hip", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                                                          "-o", str(tmp / "devimage.o")]
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


def test_every_instantiation_is_there(usage):
    imports = [k for k in usage if "image_import_kernel" in k]
    exports = [k for k in usage if "image_export_kernel" in k]
    assert len(imports) == 5 * 2 * 2  # dtype x layout x cache policy
    assert len(exports) == (5 * 2 + 2) * 2  # dtype x layout (+ sRGB U8 in both layouts) x cache policy


def test_no_scratch_and_full_occupancy(usage):
    seen = 0
    for name, u in usage.items():
        if "image_import_kernel" not in name and "image_export_kernel" not in name:
            continue
        seen += 1
        assert u.get("ScratchSize", 0) == 0, (name, u)
        assert u["VGPRs"] <= 64, (name, u)
    assert seen == 44
