#!/usr/bin/env python3
"""Are the kernels of some device units the same machine code as those of another unit?  (What showed that cutting the old
csrc/kernels.hip into one unit per kernel family moved code and changed none: kernels_split_check.txt.)  No GPU needed.

    python profiles/kernels_split_check.py OLD.hip -- NEW1.hip NEW2.hip ...

Compiles every unit's device side with the build's own flags (-S, -Rpass-analysis=kernel-resource-usage), takes every function
from its label to .Lfunc_end with comments stripped and local labels renumbered in order of appearance, and compares per symbol:
the text, and for kernels the resource remarks (SGPRs, VGPRs, AGPRs, scratch, occupancy, spills, LDS)."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from kanter_core_amd import build as kbuild  # noqa: E402


def compile_unit(src):
    out = os.path.join(tempfile.mkdtemp(prefix="kc_split_"), os.path.basename(src) + ".s")
    cmd = [kbuild._hipcc()] + kbuild.FLAGS + kbuild.DEVICE_FLAGS + ["-x", "hip", "--cuda-device-only", "-S",
                                                                  "-Rpass-analysis=kernel-resource-usage", src, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return " ".join(cmd), open(out).read(), r.stdout


def functions(asm):
    """{symbol: normalised body}"""
    out = {}
    lines = asm.split("\n")
    i = 0
    while i < len(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):", lines[i])
        if not m or m.group(1).startswith(".L"):
            i += 1
            continue
        j = i + 1
        while j < len(lines) and not lines[j].startswith(".Lfunc_end") and not re.match(r"^[A-Za-z_][\w$.]*:", lines[j]):
            j += 1
        if j < len(lines) and lines[j].startswith(".Lfunc_end"):
            names = {}
            body = []
            for ln in lines[i + 1:j]:
                ln = ln.split(";")[0].rstrip()
                if not ln.strip():
                    continue
                ln = re.sub(r"\.L[\w$]+", lambda k: names.setdefault(k.group(0), ".L%d" % len(names)), ln)
                body.append(ln)
            assert m.group(1) not in out, m.group(1)
            out[m.group(1)] = "\n".join(body)
        i = j
    return out


def remarks(log):
    """{kernel: [remark lines]}"""
    out = {}
    name = None
    for ln in log.splitlines():
        m = re.search(r"remark: (.*)$", ln)
        if not m:
            continue
        f = re.match(r"Function Name: (\S+)", m.group(1))
        if f:
            name = f.group(1)
            assert name not in out, name
            out[name] = []
        elif name:
            out[name].append(m.group(1).strip())
    return out


def gather(sources):
    funcs, rem = {}, {}
    with ThreadPoolExecutor(max_workers=4) as ex:
        for src, (cmd, asm, log) in zip(sources, ex.map(compile_unit, sources)):
            print(cmd)
            f, r = functions(asm), remarks(log)
            for table, new in ((funcs, f), (rem, r)):
                dup = set(table) & set(new)
                assert not dup, ("defined in two units", src, sorted(dup)[:3])
                table.update(new)
    return funcs, rem


if __name__ == "__main__":
    cut = sys.argv.index("--")
    old_f, old_r = gather(sys.argv[1:cut])
    new_f, new_r = gather(sys.argv[cut + 1:])
    print("old: %d kernels, %d functions, %d instruction lines" % (len(old_r), len(old_f), sum(b.count("\n") + 1 for b in old_f.values())))
    print("new: %d kernels, %d functions, %d instruction lines" % (len(new_r), len(new_f), sum(b.count("\n") + 1 for b in new_f.values())))
    only_old, only_new = sorted(set(old_f) - set(new_f)), sorted(set(new_f) - set(old_f))
    differ = sorted(k for k in set(old_f) & set(new_f) if old_f[k] != new_f[k])
    rdiffer = sorted(k for k in set(old_r) | set(new_r) if old_r.get(k) != new_r.get(k))
    print("symbols only in old: %d, only in new: %d; bodies that differ: %d; remark tables that differ: %d"
          % (len(only_old), len(only_new), len(differ), len(rdiffer)))
    for k in (only_old + only_new + differ + rdiffer)[:20]:
        print("  ", k)
    sys.exit(1 if only_old or only_new or differ or rdiffer else 0)
