"""Device code of the chain kernels generated at run time (csrc/specialize.cpp), without a GPU: the text that
kc.specialize_compile_check returns is compiled for gfx950 with the generator's own options to an assembly listing, and the
listing is counted.  Every {+, -, *} step must be packed f32 instructions, two per float4 (v_pk_add_f32 / v_pk_mul_f32; a
subtraction is a packed add with the negate modifier on the subtrahend), four for a "c - (acc op x)" record; no unpacked f32
add, subtract or multiply may remain.  The 16-record headline program had 103 vector instructions per wave before (64 of
them v_sub_f32) and is held to 90 here."""
import collections
import re
import subprocess

import pytest

import kanter_core_amd as kc
from kanter_core_amd import build as kbuild

ADD, SUB_L, SUB_R, MUL, DIV_L, DIV_R, POW_L, POW_R = range(8)
ADD_INV, SUBL_INV, SUBR_INV, MUL_INV = 10, 11, 12, 13
SAVE_LOAD = 14
SAVED = 254  # operand source index of the saved value (word bits 8-15 = 255)

# the options of kCompileOpts (csrc/specialize.cpp); hiprtc supplies the HIP built-ins that the header supplies here
OPTS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt"]
UNPACKED = ("v_add_f32", "v_sub_f32", "v_subrev_f32", "v_mul_f32")


def word(code, src):
    return code | ((src + 1) << 8)


def listing(src, tmp_path):
    hip, out = tmp_path / "kernel.hip", tmp_path / "kernel.s"
    hip.write_text(src)
    cmd = [kbuild._hipcc()] + OPTS + ["-x", "hip", "-include", "hip/hip_runtime.h", "--cuda-device-only", "-S", str(hip), "-o", str(out)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    return out.read_text()


def count(text):
    """(histogram of the one kernel's instructions by mnemonic without its encoding suffix, its metadata as a dict)."""
    lines = text.split("\n")
    start = [i for i, l in enumerate(lines) if re.match(r"^kc_chain_[0-9a-f]{8}:", l)]
    assert len(start) == 1
    hist = collections.Counter()
    for l in lines[start[0] + 1:]:
        t = l.strip()
        if re.match(r"^[a-z]", t) and not t.endswith(":"):
            op = re.sub(r"_e(32|64)$|_dpp$|_sdwa$", "", t.split()[0])
            # "idx / P.row_units" of the pitched form: the compiler's unsigned division scales its reciprocal estimate by
            # 0x4f7ffffe with one v_mul_f32.  Addressing, not a step of the program (the parent has it too): counted apart.
            hist["udiv_scale" if op == "v_mul_f32" and "0x4f7ffffe" in t else op] += 1
        if "s_endpgm" in t:
            break
    meta = {k: int(v) for k, v in re.findall(r"^\s+\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", text, re.M)}
    assert set(meta) == {"vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"}, meta
    return hist, meta


def packed(hist):
    return hist["v_pk_add_f32"] + hist["v_pk_mul_f32"]


def valu(hist):
    return sum(n for k, n in hist.items() if k.startswith("v_") or k == "udiv_scale")


def assert_no_scratch(hist, meta):
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, meta
    assert not any(k.startswith("scratch_") for k in hist), hist


def test_headline_program_is_four_packed_instructions_a_record(tmp_path):
    # the 32-node BASELINE graph: 16 records "c - (acc op B)", op alternating +, *, on input plane 1
    words = [word(ADD_INV if i % 2 == 0 else MUL_INV, 1) for i in range(16)]
    hist, meta = count(listing(kc.specialize_compile_check(words, n_in=2, start_src=0, flat=True), tmp_path))
    print("headline: %d vector instructions, %s, %s" % (valu(hist), dict(hist.most_common(8)), meta))
    assert packed(hist) == 64
    assert not any(hist[k] for k in UNPACKED), hist
    assert valu(hist) <= 90
    assert_no_scratch(hist, meta)
    assert meta["vgpr_count"] <= 64


@pytest.mark.parametrize("flat", [True, False])
def test_every_add_subtract_multiply_step_is_packed(tmp_path, flat):
    plain, inv = [ADD, SUB_L, SUB_R, MUL], [ADD_INV, SUBL_INV, SUBR_INV, MUL_INV]
    words = [word(c, 1 + i % 2) for i, c in enumerate(plain + inv)]              # on a plane
    words += [word(c, -1) for c in plain]                                        # on the record's constant, either side
    words += [word(SAVE_LOAD, 1)] + [word(c, SAVED) for c in plain + inv]        # on a saved value
    steps = 3 * len(plain) + 2 * len(inv)
    hist, meta = count(listing(kc.specialize_compile_check(words, n_in=3, start_src=0, flat=flat), tmp_path))
    print("flat=%s: %d vector instructions, %s, %s" % (flat, valu(hist), dict(hist.most_common(8)), meta))
    assert packed(hist) == 2 * (steps + 2 * len(inv))  # two per step, four per "c - (acc op x)" record
    assert not any(hist[k] for k in UNPACKED), hist
    assert hist["udiv_scale"] == (0 if flat else 1)
    assert_no_scratch(hist, meta)


def test_divide_and_pow_programs_still_compile(tmp_path):
    for code in (DIV_L, DIV_R, POW_L, POW_R):
        words = [word(ADD_INV, 1), word(code, 1), word(SUB_R, -1), word(code, -1), word(MUL, 0)]
        src = kc.specialize_compile_check(words, n_in=2, start_src=0, flat=False)
        hist, meta = count(listing(src, tmp_path))
        assert packed(hist) >= 8, hist  # the {+, -, *} steps beside them: c - (acc + x), c - acc, acc * x
