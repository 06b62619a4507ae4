#!/usr/bin/env python3
"""Derives the bindings from include/kanter_core_amd.h, the one hand-written description of the C ABI:

    kanter_core_amd/_abi.py                  ctypes structures, constants and SIGNATURES of the Python binding
    bindings/rust/kanter_core_amd_sys.rs     the `extern "C"` module a maintainer of the reference (Rust) adds

Both are committed; tests/test_cabi_symbols.py regenerates them into a scratch directory (--out) and compares.  The parser
understands the subset of C the header uses and refuses everything else with the line it stopped at.  No Rust toolchain
exists in this build environment: the .rs file is source only."""
import argparse
import collections
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kanter_core_amd.h")
OUTPUTS = {"_abi.py": os.path.join(ROOT, "kanter_core_amd"), "kanter_core_amd_sys.rs": os.path.join(ROOT, "bindings", "rust")}

# C scalar -> (ctypes, Rust)
SCALARS = {"int": ("c_int", "i32"), "int32_t": ("c_int32", "i32"), "uint32_t": ("c_uint32", "u32"), "uint64_t": ("c_uint64", "u64"),
           "uint8_t": ("c_uint8", "u8"), "size_t": ("c_size_t", "usize"), "float": ("c_float", "f32"), "double": ("c_double", "f64"),
           "char": ("c_char", "c_char"), "void": (None, "c_void")}
# The two function-like macros of the header stay hand-written wherever they are used (api.mip_coverage_ref and
# api.bc_punch_through_ref, these one-liners); every other one is refused.
MACROS = {
    "KC_MIP_COVERAGE_REF": """/// KC_MIP_COVERAGE with the reference byte b, 1..255 (KC_MIP_COVERAGE_REF)
pub const fn kc_mip_coverage_ref(b: u8) -> u32 { KC_MIP_COVERAGE | (b as u32) << 24 }""",
    "KC_BC_PUNCH_THROUGH_REF": """/// KC_BC_PUNCH_THROUGH with the reference byte b, 1..255 (KC_BC_PUNCH_THROUGH_REF)
pub const fn kc_bc_punch_through_ref(b: u8) -> u32 { KC_BC_PUNCH_THROUGH | (b as u32) << 24 }""",
}


class HeaderError(ValueError):
    def __init__(self, line, what):
        super().__init__("include/kanter_core_amd.h:%d: %s" % (line, what))
        self.line = line


# base: a scalar, struct or handle name; const: the pointee is const; stars: pointer levels; ptr_const: `*const`, a read-only
# pointer; dims: array bounds, outermost first (None: `[]`)
Type = collections.namedtuple("Type", "base const stars ptr_const dims")
Define = collections.namedtuple("Define", "name value unsigned")
Enum = collections.namedtuple("Enum", "name members")          # members: [(name, value)]
Macro = collections.namedtuple("Macro", "name")                # one of the function-like ones
Opaque = collections.namedtuple("Opaque", "name")
Struct = collections.namedtuple("Struct", "name fields")       # fields: [(name, Type)]
Func = collections.namedtuple("Func", "name ret params")       # params: [(name, Type)]

_DECL = re.compile(r"\s*(const\s+)?(\w+)\b\s*((?:\*\s*(?:const\b\s*)?)*)(\w+)?\s*((?:\[\s*\w*\s*\])*)\s*")


class Header:
    """The declarations of a header, `items` in its order."""

    def __init__(self, text):
        self.found = []   # (line, item)
        self.values = {}  # every enumerator and object-like define
        self._parse(text)
        self.items = [i for _, i in sorted(self.found, key=lambda f: f[0])]

    def of(self, kind):
        return [i for _, i in self.found if isinstance(i, kind)]

    def _decl(self, text, line, named=True):
        """`const T *name[N]` -> (name, Type); a name the header never declared is refused."""
        m = _DECL.fullmatch(text)
        if not m or bool(m.group(4)) != named:
            raise HeaderError(line, "cannot read the declaration %r" % " ".join(text.split()))
        base, stars = m.group(2), m.group(3).count("*")
        by_value = {s.name for s in self.of(Struct)} | set(SCALARS) - {"void"}
        if base not in by_value and not (stars and (base == "void" or base in {o.name for o in self.of(Opaque)})):
            raise HeaderError(line, "unknown type %r in %r" % (base, " ".join(text.split())))
        dims = []
        for d in re.findall(r"\[\s*(\w*)\s*\]", m.group(5)):
            if d and not d.isdigit() and d not in self.values:
                raise HeaderError(line, "unknown array bound %r" % d)
            dims.append(int(d) if d.isdigit() else d or None)
        return m.group(4), Type(base, bool(m.group(1)), stars, "const" in m.group(3), tuple(dims))

    def _parse(self, text):
        blank = lambda m: re.sub(r"[^\n]", " ", m.group())
        text = re.sub(r"/\*.*?\*/|//[^\n]*", blank, text, flags=re.S)
        lines, skipping = text.split("\n"), False
        for n, s in enumerate(lines, 1):
            if s.lstrip().startswith("#"):
                s = " ".join(s.split())
                d = re.fullmatch(r"# ?define (\w+)(\([^)]*\))? ?(.*)", s)
                if s.endswith("\\") or not (d or re.match(r"# ?(ifdef|ifndef|endif|include)\b", s)):
                    raise HeaderError(n, "cannot read the directive %r" % s)
                if s.startswith("#ifdef __cplusplus"):
                    skipping = True
                elif s.startswith("#endif"):
                    skipping = False
                elif d and d.group(1) in MACROS and d.group(2):
                    self.found.append((n, Macro(d.group(1))))
                elif d and d.group(1) != "KC_API" and (d.group(2) or d.group(3)):  # KC_API: the export attribute; no body: the guard
                    v = re.fullmatch(r"(\d+|0[xX][0-9a-fA-F]+)([uU]?)", d.group(3))
                    if d.group(2) or not v:
                        raise HeaderError(n, "#define %s is neither an integer literal nor %s" % (d.group(1), " or ".join(MACROS)))
                    self.found.append((n, Define(d.group(1), int(v.group(1), 0), bool(v.group(2)))))
                    self.values[d.group(1)] = int(v.group(1), 0)
            if skipping or s.lstrip().startswith("#"):  # `extern "C" {` and its brace are C++ only
                lines[n - 1] = ""
        text = "\n".join(lines)
        line_at = lambda pos: text.count("\n", 0, pos) + 1
        start, depth = 0, 0
        for pos, ch in enumerate(text):
            depth += (ch == "{") - (ch == "}")
            if ch == ";" and depth == 0:
                stmt = text[start:pos]
                start += len(stmt) - len(stmt.lstrip())
                self._statement(text[start:pos], start, line_at)
                start = pos + 1
        if text[start:].strip():
            raise HeaderError(line_at(start + len(text[start:]) - len(text[start:].lstrip())), "unterminated declaration")

    def _statement(self, stmt, pos, line_at):
        line = line_at(pos)
        m = re.fullmatch(r"typedef\s+struct\s+(\w+)\s+(\w+)", stmt)
        if m and m.group(1) == m.group(2):
            return self.found.append((line, Opaque(m.group(1))))
        m = re.fullmatch(r"typedef\s+(enum|struct)\s+(\w+)\s*\{(.*)\}\s*(\w+)", stmt, re.S)
        if m and m.group(2) == m.group(4) and m.group(1) == "enum":
            members = []
            for part in re.finditer(r"[^,]*[^,\s][^,]*", m.group(3)):
                e = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", part.group())
                if not e:
                    raise HeaderError(line_at(pos + m.start(3) + part.start()), "enumerator without an explicit integer value: %r" % part.group().strip())
                members.append((e.group(1), int(e.group(2))))
                self.values[e.group(1)] = int(e.group(2))
            return self.found.append((line, Enum(m.group(2), members)))
        if m and m.group(2) == m.group(4):
            fields = []
            for part in re.finditer(r"[^;]*[^;\s][^;]*", m.group(3)):
                at = line_at(pos + m.start(3) + part.start() + len(part.group()) - len(part.group().lstrip()))
                first, *more = part.group().split(",")
                name, t = self._decl(first, at)
                fields.append((name, t))
                for decl in more:  # `uint32_t x, y`: the specifiers are shared, stars and bounds are each declarator's own
                    fields.append(self._decl("%s%s %s" % ("const " if t.const else "", t.base, decl), at))
                if any(None in t.dims for _, t in fields[-len(more) - 1:]):
                    raise HeaderError(at, "a member array needs its bounds")
            return self.found.append((line, Struct(m.group(2), fields)))
        m = re.fullmatch(r"KC_API\s+(.*?)\b(\w+)\s*\((.*)\)", stmt, re.S)
        if m:
            ret = m.group(1).strip()
            ret = Type("void", False, 0, False, ()) if ret == "void" else self._decl(ret, line, named=False)[1]
            params = [] if m.group(3).strip() == "void" else [self._decl(p, line) for p in m.group(3).split(",")]
            return self.found.append((line, Func(m.group(2), ret, params)))
        raise HeaderError(line, "cannot read the declaration %r" % " ".join(stmt.split())[:80])


# ---------------------------------------------------------------------------------------------- Python (ctypes)
def ctypes_type(h, t, param=False):
    """One rule per C type.  Handles and `void *` are addresses; so are `uint8_t *` and `float *`, the bulk buffers, which callers
    hand over as integers (numpy's .ctypes.data) as well as arrays and byref(); other scalars and structs keep a typed pointer."""
    stars = t.stars + (1 if param and t.dims else 0)
    struct = t.base in {s.name for s in h.of(Struct)}
    if stars == 0:
        r = t.base if struct else "C." + SCALARS[t.base][0]
    elif stars > 1:
        r = "C.POINTER(C.c_void_p)"  # a pointer to any pointer
    elif struct:
        r = "C.POINTER(%s)" % t.base
    elif t.base == "char":
        r = "C.c_char_p"
    elif t.base in ("void", "uint8_t", "float") or t.base not in SCALARS:
        r = "C.c_void_p"
    else:
        r = "C.POINTER(C.%s)" % SCALARS[t.base][0]
    for d in () if param else reversed(t.dims):
        r = "%s * %s" % ("(%s)" % r if " * " in r else r, d)
    return r


def _join(blocks, gap):
    """One-line blocks that follow one another stay together; all others stand `gap` apart."""
    lone = [False] + ["\n" not in b for b in blocks]
    return "".join(("" if n == 0 else "\n" if lone[n] and lone[n + 1] else gap) + b for n, b in enumerate(blocks))


def _void(t):
    return t.base == "void" and not t.stars


def render_python(h):
    blocks = ['"""GENERATED by bindings/gen.py from include/kanter_core_amd.h -- do not edit; rerun `python bindings/gen.py`.\n\n'
              'The C ABI as ctypes sees it: every struct, every enumerator and #define under its C name, and SIGNATURES.\n"""\n'
              "import ctypes as C"]
    for i in h.items:
        if isinstance(i, Define):
            blocks.append("%s = %d" % (i.name, i.value))
        elif isinstance(i, Enum):
            blocks.append("\n".join(["# %s" % i.name] + ["%s = %d" % m for m in i.members]))
        elif isinstance(i, Struct):
            fields = ['        ("%s", %s),' % (n, ctypes_type(h, t)) for n, t in i.fields]
            blocks.append("\n".join(["class %s(C.Structure):" % i.name, "    _fields_ = ["] + fields + ["    ]"]))
    sigs = ['    "%s": (%s, [%s]),' % (f.name, "None" if _void(f.ret) else ctypes_type(h, f.ret),
                                       ", ".join(ctypes_type(h, t, True) for _, t in f.params)) for f in h.of(Func)]
    blocks.append("\n".join(["# name -> (restype, argtypes); every entry point the header declares.", "SIGNATURES = {"] + sigs + ["}"]))
    return _join(blocks, "\n\n\n") + "\n"


# ---------------------------------------------------------------------------------------------- Rust
def rust_name(c_name):
    return "".join(w.capitalize() for w in c_name.split("_")) if c_name.startswith("kc_") else SCALARS[c_name][1]


def rust_type(t, param=False):
    r = rust_name(t.base)
    stars = t.stars + (1 if param and t.dims else 0)
    # constness of the pointee: `const T *` -> *const T; `T *const x[]` -> the array of pointers itself is read-only
    ptrs = ["*const " if level == 0 and t.const else "*mut " for level in range(stars)]
    if param and t.dims and t.ptr_const:
        ptrs[-1] = "*const "
    for ptr in ptrs:
        r = ptr + r
    for d in () if param else reversed(t.dims):
        r = "[%s; %s]" % (r, d)
    return r


def render_rust(h):
    blocks = ["// GENERATED by bindings/gen.py from include/kanter_core_amd.h -- do not edit; rerun `python bindings/gen.py`.\n"
              '// `extern "C"` declarations for libkanter_core_amd.so (MI355X backend of the kanter_core /\n'
              "// vismut_core per-pixel hot path).  See INTEGRATION.md for the replacement bodies of\n"
              "// src/node/*.rs::process and src/shared.rs::resize_buffers that call these.  The header documents every item.\n"
              "#![allow(non_camel_case_types, dead_code)]\nuse std::os::raw::{c_char, c_void};"]
    floats = set()  # structs that hold a float, directly or nested: no Eq
    for i in h.items:
        if isinstance(i, Define):
            blocks.append("pub const %s: %s = %d;" % (i.name, "u32" if i.unsigned else "usize", i.value))
        elif isinstance(i, Macro):
            blocks.append(MACROS[i.name])
        elif isinstance(i, Enum):
            blocks.append("\n".join(["// %s" % i.name] + ["pub const %s: i32 = %d;" % m for m in i.members]))
        elif isinstance(i, Opaque):
            blocks.append("#[repr(C)] pub struct %s { _private: [u8; 0] }" % rust_name(i.name))
        elif isinstance(i, Struct):
            if any(t.base in ("float", "double") or t.base in floats for _, t in i.fields if not t.stars):
                floats.add(i.name)
            derive = "Clone, Copy, Debug" + ("" if i.name in floats else ", PartialEq, Eq")
            fields = ["    pub %s: %s," % (n, rust_type(t)) for n, t in i.fields]
            blocks.append("\n".join(["/// %s" % i.name, "#[repr(C)] #[derive(%s)]" % derive, "pub struct %s {" % rust_name(i.name)] + fields + ["}"]))
    fns = ["    pub fn %s(%s)%s;" % (f.name, ", ".join("%s: %s" % (n + "_" if n in ("in", "type", "box") else n, rust_type(t, True)) for n, t in f.params),
                                    "" if _void(f.ret) else " -> %s" % rust_type(f.ret)) for f in h.of(Func)]
    blocks.append("\n".join(['#[link(name = "kanter_core_amd")]', 'extern "C" {'] + fns + ["}"]))
    return _join(blocks, "\n\n") + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", metavar="DIR", help="write both files into DIR instead of their places in the tree")
    args = ap.parse_args()
    h = Header(open(HEADER).read())
    for name, text in (("_abi.py", render_python(h)), ("kanter_core_amd_sys.rs", render_rust(h))):
        path = os.path.join(args.out or OUTPUTS[name], name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
        print("%d functions, %d structs -> %s" % (len(h.of(Func)), len(h.of(Struct)), path))


if __name__ == "__main__":
    main()
