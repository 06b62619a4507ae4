"""tests/host/preview_walk_check.cpp -- every workgroup and thread of every pass of kc_image_previews walked on the CPU with the
library's own planner and index functions (csrc/preview_walk.h), real loads and stores on buffers of exact size -- built with
the ROCm clang++ under the address and undefined-behaviour sanitizers and run as a child process of its own, in the
environment as it is.  Exit status 0 and
no sanitizer report: no address the device would form leaves a plane, the scratch or a rect, every byte of a rect is written
exactly once with the reference value and nothing else is touched.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clangxx():
    for cand in (os.environ.get("KC_CLANGXX"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cand and os.path.exists(cand):
            return cand
    return shutil.which("amdclang++")


def test_the_walk_is_clean_under_the_sanitizers(tmp_path):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("the ROCm clang++ is not available")
    exe = str(tmp_path / "preview_walk_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "kanter_core_amd", "csrc"), os.path.join(ROOT, "tests", "host", "preview_walk_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")  # the program is linked with its sanitizer runtime
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    assert "0 failures" in r.stdout, r.stdout[-3000:]
