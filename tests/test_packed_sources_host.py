"""Packed copies of chain inputs without a device: the kernel the headline launches once its sources are packed (csrc/chain_pack.h,
csrc/chain_codegen.cpp), cross-compiled by hiprtc and read back as ISA, and the optional "in_tiers" field of the manifest of
pre-compiled programs."""
import json
import os
import shutil
import struct
import subprocess

import pytest

import kanter_core_amd as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANIFEST = os.path.join(ROOT, "kanter_core_amd", "baseline_programs.jsonl")
FIX24_BOTH = 0b0101  # inputs 0 and 1 in tier FIX24


def entries():
    return [json.loads(line) for line in open(MANIFEST) if line.strip()]


def headline():
    """The 16-record program of the 32-node graph with input 0 and the result nontemporal, two float4 per lane."""
    e = [e for e in entries() if e["n_in"] == 2 and len(e["words"]) == 16 and e["nt_mask"] == 0x101 and not e.get("in_tiers")]
    assert len(e) == 1
    return e[0]


def objdump():
    for cand in ("/opt/rocm/llvm/bin/llvm-objdump", shutil.which("llvm-objdump")):
        if cand and os.path.exists(cand):
            return cand
    pytest.skip("no llvm-objdump")


def isa_of(tmp_path, e, in_tiers):
    kc.kernel_cache_precompile(e["words"], e["n_in"], e["start_src"], True, e["nt_mask"], tmp_path, in_tiers=in_tiers)
    files = [f for f in os.listdir(tmp_path) if f.endswith(".kcco")]
    assert len(files) == 1
    blob = open(os.path.join(tmp_path, files[0]), "rb").read()
    key_len, _, code_len, _ = struct.unpack("<4Q", blob[8:40])
    key = blob[40:40 + key_len]
    co = os.path.join(tmp_path, "kernel.co")
    with open(co, "wb") as f:
        f.write(blob[40 + key_len:])
    text = subprocess.run([objdump(), "-d", co], check=True, stdout=subprocess.PIPE, text=True).stdout
    return files[0], key, [line.split()[0] for line in text.splitlines() if line.startswith("\t")]


def test_isa_of_the_packed_headline_kernel(tmp_path):
    e = headline()
    name, key, isa = isa_of(tmp_path, e, FIX24_BOTH)
    quads = 2  # the warm form: two float4 per lane
    assert key.endswith(b"q2t" + struct.pack("<I", FIX24_BOTH))  # the tier word is the last thing in the key ...
    assert not name.startswith(e["name"] + "-")                  # ... and makes another kernel of it
    assert isa.count("global_load_dwordx3") == 2 * quads and isa.count("global_load_dwordx4") == 0, [i for i in isa if i.startswith("global")]
    assert isa.count("global_store_dwordx4") == quads
    vector = [i for i in isa if i.startswith("v_")]
    assert len(vector) < 100 * quads, len(vector)


def test_an_f32_kernel_keeps_its_name(tmp_path):
    e = headline()
    name, key, isa = isa_of(tmp_path, e, 0)
    assert name.startswith(e["name"] + "-") and key.endswith(b"q2")
    assert isa.count("global_load_dwordx4") == 4 and isa.count("global_load_dwordx3") == 0


def test_u8_tier_loads_one_dword_per_quad(tmp_path):
    _, _, isa = isa_of(tmp_path, headline(), 0b1010)
    assert isa.count("global_load_dword") == 4 and isa.count("global_load_dwordx4") == 0
    assert len([i for i in isa if i.startswith("v_")]) < 200


def test_refused_tier_words(tmp_path):
    e = headline()
    for tiers in (0b11, 0b010000):  # no tier 3; no tier for an input the program does not have
        with pytest.raises(kc.TexProError):
            kc.kernel_cache_precompile(e["words"], e["n_in"], e["start_src"], True, e["nt_mask"], tmp_path, in_tiers=tiers)
    with pytest.raises(kc.TexProError):  # pitched launches read f32
        kc.kernel_cache_precompile(e["words"], e["n_in"], e["start_src"], False, e["nt_mask"], tmp_path, in_tiers=FIX24_BOTH)


def test_manifest_entries_with_and_without_the_field_precompile():
    all_entries = entries()
    packed = [e for e in all_entries if e.get("in_tiers")]
    assert packed and len(packed) < len(all_entries)
    h = headline()
    assert any(e["words"] == h["words"] and e["nt_mask"] == h["nt_mask"] and e["in_tiers"] == FIX24_BOTH for e in packed)
    from kanter_core_amd import build as kbuild
    assert kbuild.populate_kernel_cache() == len(all_entries)
    have = os.listdir(kbuild.KERNEL_CACHE)
    for e in packed + [h]:
        assert any(f.startswith(e["name"] + "-") and f.endswith(".kcco") for f in have), e["name"]
