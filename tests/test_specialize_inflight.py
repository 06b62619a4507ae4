"""The compiled chain kernels with more than one float4 per lane (csrc/chain_codegen.cpp, chain_quads_for / emit_quads),
without a GPU.  A flat {+, -, *} program whose cache-policy mask leaves an input plain beside a nontemporal stream gets
QUADS float4 per lane if it has at most 16 records: every load of the lane is issued before the first step, then one quad after the other runs the
program, and the stores follow the last body.  Its listing for gfx950 is counted the way tests/test_specialize_isa.py counts the one-quad form; every signature
outside the rule must generate exactly the one-quad text; and the generator's host code runs under AddressSanitizer and
UndefinedBehaviorSanitizer in a stand-alone program (tests/c_host/specialize_generate_check.cpp)."""
import os
import re
import shutil
import subprocess

import pytest

import kanter_core_amd as kc
from test_specialize_isa import ADD, ADD_INV, DIV_L, MUL, MUL_INV, POW_L, SUB_R, UNPACKED, assert_no_scratch, count, listing, packed, valu, word

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUADS = 2  # kQuadsWarm: what the rule picks (profiles/chain_inflight_times.txt)
HEADLINE = [word(ADD_INV if i % 2 == 0 else MUL_INV, 1) for i in range(16)]  # the 32-node BASELINE graph, as in test_specialize_isa


@pytest.fixture
def quads():
    """Sets chain_quads for one test; the rule's own choice comes back afterwards."""
    yield kc.set_chain_quads
    kc.set_chain_quads(0)


def kernel_lines(text):
    lines = text.split("\n")
    start = [i for i, l in enumerate(lines) if re.match(r"^kc_chain_[0-9a-f]{8}:", l)]
    assert len(start) == 1
    out = []
    for l in lines[start[0] + 1:]:
        t = l.strip()
        if re.match(r"^[a-z]", t) and not t.endswith(":"):
            out.append(t)
        if "s_endpgm" in t:
            break
    return out


@pytest.mark.parametrize("setting, per_lane", [(0, QUADS), (2, 2), (4, 4)])
def test_headline_program_with_a_resident_input(tmp_path, quads, setting, per_lane):
    quads(setting)
    assert kc.get_chain_quads() == setting
    text = listing(kc.specialize_compile_check_mask(HEADLINE, n_in=2, nt_mask=0x101), tmp_path)
    hist, meta = count(text)
    print("chain_quads=%d: %d vector instructions, %s, %s" % (setting, valu(hist), dict(hist.most_common(8)), meta))
    assert packed(hist) == per_lane * 64  # straight-line: one body per quad
    assert not any(hist[k] for k in UNPACKED), hist
    assert hist["global_load_dwordx4"] == 2 * per_lane
    ops = [l.split()[0] for l in kernel_lines(text)]
    first_packed = min(i for i, op in enumerate(ops) if op.startswith("v_pk_"))
    assert all(i < first_packed for i, op in enumerate(ops) if op.startswith("global_load")), "a load behind the first step"
    assert_no_scratch(hist, meta)
    assert meta["vgpr_count"] <= 64  # 8 waves per SIMD remain


def test_a_setting_of_one_is_the_one_quad_kernel(tmp_path, quads):
    quads(1)
    hist, meta = count(listing(kc.specialize_compile_check_mask(HEADLINE, n_in=2, nt_mask=0x101), tmp_path))
    assert packed(hist) == 64 and hist["global_load_dwordx4"] == 2 and hist["global_store_dwordx4"] == 1
    assert valu(hist) <= 90


INELIGIBLE = [
    ("mask_0", HEADLINE, 2, 0x000, True),
    ("every_input_marked", HEADLINE, 2, 0x103, True),
    ("every_input_marked_result_plain", HEADLINE, 2, 0x003, True),
    ("divide", HEADLINE[:4] + [word(DIV_L, 1)] + HEADLINE[4:8], 2, 0x101, True),
    ("pow", [word(ADD, 1), word(POW_L, -1), word(MUL, 0)], 2, 0x101, True),
    ("pitched", HEADLINE, 2, 0x101, False),
    ("seventeen_records", HEADLINE + HEADLINE[:1], 2, 0x101, True),
    ("no_input_plane", [word(ADD, -1), word(SUB_R, -1)], 0, 0x100, True),
]


@pytest.mark.parametrize("case", INELIGIBLE, ids=[c[0] for c in INELIGIBLE])
def test_signatures_outside_the_rule_keep_the_one_quad_text(quads, case):
    _, words, n_in, mask, flat = case
    start = 0 if n_in else -1
    quads(1)
    one = kc.specialize_compile_check_mask(words, n_in=n_in, nt_mask=mask, start_src=start, flat=flat)
    for setting in (0, 2, 4):
        quads(setting)
        assert kc.specialize_compile_check_mask(words, n_in=n_in, nt_mask=mask, start_src=start, flat=flat) == one, setting
    if mask == 0:  # and everything kc_specialize_compile_check returns
        assert kc.specialize_compile_check(words, n_in=n_in, start_src=start, flat=flat) == one


def test_an_eligible_mask_changes_the_text_and_the_kernel_name(quads):
    quads(1)
    one = kc.specialize_compile_check_mask(HEADLINE, n_in=2, nt_mask=0x101)
    names = {re.search(r"kc_chain_[0-9a-f]{8}", one).group(0)}
    for setting in (2, 4):
        quads(setting)
        text = kc.specialize_compile_check_mask(HEADLINE, n_in=2, nt_mask=0x101)
        assert text != one
        names.add(re.search(r"kc_chain_[0-9a-f]{8}", text).group(0))
    assert len(names) == 3  # the form is part of the signature: never one kernel under the grid of another


def test_refused_settings(quads):
    for bad in (-1, 3, 5, 8):
        with pytest.raises(kc.TexProError):
            quads(bad)
    assert kc.get_chain_quads() == 0


def test_generator_host_code_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/chain_codegen.cpp and the check program alone: the generator needs no HIP runtime, no context and no other unit.
    The program's output -- its sweep's verdict and one digest per group of generated texts -- is pinned in
    tests/golden/chain_kernel_texts.txt.  After an intended change of the generator, from the repository's root:
    hipcc -x c++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -Ikanter_core_amd/csrc kanter_core_amd/csrc/chain_codegen.cpp tests/c_host/specialize_generate_check.cpp -o /tmp/kc_texts && /tmp/kc_texts > tests/golden/chain_kernel_texts.txt"""
    from kanter_core_amd import build as kbuild
    hipcc = shutil.which(kbuild._hipcc()) or kbuild._hipcc()
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))  # <rocm>/bin/hipcc
    csrc = os.path.join(ROOT, "kanter_core_amd", "csrc")
    exe = str(tmp_path / "specialize_generate_check")
    cmd = [hipcc, "-x", "c++", "-O1", "-g", "-std=c++17", "-fno-fast-math", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(csrc, "chain_codegen.cpp"),
           os.path.join(ROOT, "tests", "c_host", "specialize_generate_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), r.stdout
    with open(os.path.join(ROOT, "tests", "golden", "chain_kernel_texts.txt")) as f:
        assert r.stdout == f.read()
