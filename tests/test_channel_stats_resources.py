"""Build-time guard for the channel statistics kernels (csrc/stats.hip): every instantiation of channel_stats_kernel -- min / max
only, with the histogram, with the sRGB histogram, each in both cache policies -- and the combine kernel keep zero scratch and
at most 64 VGPRs (they are HBM-bound streams and need the loads in flight)."""
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
    tmp = tmp_path_factory.mktemp("stats_res")
    src = os.path.join(ROOT, "kanter_core_amd", "csrc", "stats.hip")
    cmd = [hipcc] + kbuild.FLAGS + kbuild.DEVICE_FLAGS + ["-x", "hip", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                                                          "-o", str(tmp / "stats.o")]
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
    mains = [k for k in usage if "channel_stats_kernel" in k]
    assert len(mains) == 3 * 2  # (plain, histogram, sRGB histogram) x cache policy
    assert len([k for k in usage if "channel_stats_combine_kernel" in k]) == 1


def test_no_scratch_and_full_occupancy(usage):
    seen = 0
    for name, u in usage.items():
        if "channel_stats" not in name:
            continue
        seen += 1
        assert u.get("ScratchSize", 0) == 0, (name, u)
        assert u["VGPRs"] <= 64, (name, u)
    assert seen == 7
