"""Shared helpers for the parity tests: synthetic planes, ulp distance,
bitwise comparison that treats NaN == NaN; and the compiler's resource remarks of a device unit for the build-time guards."""
import os
import re
import shutil
import subprocess

import numpy as np

SEED_A, SEED_B = 0x5EED0001, 0x5EED0002


def splitmix_plane(seed, channel, h, w):
    """u in [0, 1): (splitmix64(seed, idx) >> 40) * 2^-24 with idx = (c*H + y)*W + x."""
    idx = (np.uint64(channel) * np.uint64(h) * np.uint64(w)) + np.arange(h * w, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = np.uint64(seed) + (idx + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(h, w)


def splitmix_rows(seed, channel, h, w, y0, y1):
    """Rows [y0, y1) of splitmix_plane(seed, channel, h, w) without generating the rest."""
    idx = (np.uint64(channel) * np.uint64(h) * np.uint64(w)) + np.uint64(y0) * np.uint64(w) + np.arange((y1 - y0) * w, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = np.uint64(seed) + (idx + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(y1 - y0, w)


def synthetic_rgba(seed, h, w):
    return [splitmix_plane(seed, c, h, w) for c in range(4)]


EDGE_VALUES = np.array([0.0, -0.0, 1.0, 2.0, -1.0, np.inf, -np.inf, np.nan, 5.877e-39, 0.1, 0.5, 254.5 / 255,
                        1e-30, 3.0, -2.5, 1e30], np.float32)


def with_edge_cases(plane, shift=0):
    """Overwrites the head of the plane with IEEE edge cases (all pairs appear when two planes
    use different shifts)."""
    p = plane.copy().reshape(-1)
    n = len(EDGE_VALUES)
    reps = min(len(p) // n, n)
    for r in range(reps):
        p[r * n:(r + 1) * n] = np.roll(EDGE_VALUES, shift * r)
    return p.reshape(plane.shape)


def ordered_bits(a):
    """Maps f32 to integers that are monotone in the float order (for ulp distances)."""
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, np.int64(-2147483648) - i, i)


def max_ulp(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    both_nan = np.isnan(a) & np.isnan(b)
    one_nan = np.isnan(a) ^ np.isnan(b)
    if one_nan.any():
        return np.inf
    d = np.abs(ordered_bits(a) - ordered_bits(b))
    d[both_nan] = 0
    return int(d.max()) if d.size else 0


def bit_equal(a, b):
    """Bit-exact, except that any NaN equals any NaN (payloads are not part of the contract)."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | nan))


def assert_planes(got, want, ulp=0, what=""):
    assert len(got) == len(want), what
    for c, (g, w) in enumerate(zip(got, want)):
        if ulp == 0:
            assert bit_equal(g, w), "%s plane %d: %d mismatches, max ulp %s" % (
                what, c, int((~((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w)))).sum()), max_ulp(g, w))
        else:
            assert max_ulp(g, w) <= ulp, "%s plane %d: max ulp %s > %d" % (what, c, max_ulp(g, w), ulp)


def key_range(plane):
    """(min bits, max bits, NaN count) of a plane through the order key; None bits when it holds no non-NaN value."""
    a = np.ascontiguousarray(plane, np.float32).reshape(-1).view(np.uint32)
    nan = (a & 0x7fffffff) > 0x7f800000
    k = np.where(a >> 31 == 1, ~a, a | np.uint32(0x80000000))[~nan]
    if k.size == 0:
        return None, None, int(nan.sum())

    def back(key):
        key = np.uint32(key)
        return int(key & np.uint32(0x7fffffff)) if key >> np.uint32(31) else int(~key)
    return back(k.min()), back(k.max()), int(nan.sum())


def pow_mismatch(got, want):
    """Where `got` breaks the Pow contract against `want` (both f32): a match is bit-equal (any NaN matches any NaN) or, for
    two finite nonzero values of the same sign, one ulp apart.  So a zero's sign, inf against FLT_MAX and a flushed
    subnormal are all mismatches, unlike under max_ulp's ordered distance."""
    g = np.ascontiguousarray(got, np.float32)
    w = np.ascontiguousarray(want, np.float32)
    gi, wi = g.view(np.uint32).astype(np.int64), w.view(np.uint32).astype(np.int64)
    same = (gi == wi) | (np.isnan(g) & np.isnan(w))
    near = np.isfinite(g) & np.isfinite(w) & (g != 0) & (w != 0) & ((gi >> 31) == (wi >> 31)) & (np.abs(gi - wi) == 1)
    return ~(same | near)


def assert_pow_planes(got, want, what=""):
    """Pow planes against a reference under the contract of pow_mismatch, plane by plane."""
    assert len(got) == len(want), what
    for c, (g, w) in enumerate(zip(got, want)):
        g = np.asarray(g, np.float32)
        w = np.asarray(w, np.float32)
        assert g.shape == w.shape, "%s plane %d: shape %s != %s" % (what, c, g.shape, w.shape)
        bad = pow_mismatch(g, w)
        if bad.any():
            i = np.flatnonzero(bad.reshape(-1))[:4]
            raise AssertionError("%s plane %d: %d mismatches, e.g. got %s want %s at %s" % (
                what, c, int(bad.sum()), g.reshape(-1)[i].tolist(), w.reshape(-1)[i].tolist(), i.tolist()))


def resize_source(seed, channel, h, w):
    """A plane of values in [-0.25, 1.25) (resampled results exercise the clamp to [0, 1] on both sides); numpy's
    generator, which is much faster than splitmix_plane for the large planes of the resize tests."""
    rng = np.random.default_rng([seed, channel, h, w])
    return rng.random((h, w), dtype=np.float32) * np.float32(1.5) - np.float32(0.25)


SALT_VALUES = [np.nan, np.inf, -np.inf, -0.0, 1e-40, 3e38, 1.25, -0.25]  # 3e38 is written as a vertical pair: its sums overflow


def salt(plane, rows, cols, shift=0, values=SALT_VALUES):
    """Writes IEEE edge cases at the crossings of the given rows and columns (negative: from the end), cycling through
    `values`; a 3e38 sample gets a 3e38 neighbour below it (above it on the last row), so that vertical sums
    overflow to inf although every sample is finite."""
    h, w = plane.shape
    rows = sorted({r % h for r in rows})
    cols = sorted({c % w for c in cols})
    k = shift
    for r in rows:
        for c in cols:
            v = values[k % len(values)]
            plane[r, c] = v
            if v == 3e38:
                plane[r + 1 if r + 1 < h else r - 1, c] = v
            k += 1
    return plane


def edge_lines(n, periods, count=3):
    """Line indices on the edges of tiles, bands or strips of the given periods along an axis of n: the first and last
    two lines, and the two lines on each side of the first `count` multiples of every period (and of the last ones)."""
    out = {0, 1, n - 2, n - 1}
    for p in periods:
        for k in range(1, count + 1):
            for m in (k * p, n - (n % p or p) - (k - 1) * p):
                out.update(x for x in (m - 1, m) if 0 <= x < n)
    return sorted(out)


GUARD_ROWS = 8  # rows of guard above and below a wrapped view inside its parent tensor


def wrap_layout(name, w):
    """(pitch, column offset) in floats of a named layout of a caller-owned plane `w` wide (q = 4 * ceil(w / 4)): "tight" rows
    q apart, "pad48" q + 12 (48 bytes of padding), "offset" q + 68 with the view 4 floats in: every row starts 16 bytes off a
    32-byte boundary and the pitch is no multiple of 64 bytes."""
    q = (w + 3) // 4 * 4
    return {"tight": (q, 0), "pad48": (q + 12, 0), "offset": (q + 68, 4)}[name]


MIXED = ["tight", "pad48", "offset", "pool"]  # the layouts of R, G, B, A of a "mixed" RGBA image


class WrappedImage:
    """What wrapped_image returns: .image (the SlotImage), .planes (the pixels, numpy) and the parent tensors it keeps alive."""

    def __init__(self, kc, torch, image, planes, parents):
        self.kc, self.torch, self.image, self.planes, self.parents = kc, torch, image, planes, parents

    def assert_untouched(self):
        """Every parent tensor still holds the bits of its host copy: the library only reads a wrapped plane."""
        self.kc.sync()
        self.torch.cuda.synchronize()
        for k, (t, host) in enumerate(self.parents):
            now = t.cpu().numpy().view(np.uint32)
            assert np.array_equal(now, host.view(np.uint32)), "parent tensor %d: %d words written" % (k, int((now != host.view(np.uint32)).sum()))


def wrapped_image(kc, torch, planes, layouts, guard):
    """A SlotImage (Gray for one plane, RGBA for four) whose planes are kc_plane_wrap views into parent tensors filled with
    `guard`.  layouts: one entry per plane (or one for all) -- a name of wrap_layout, a (pitch_floats, col_offset_floats) pair,
    "pool" (a plane of the library's pool with the same pixels) or ("const", v) (a constant plane).  The parent of a view is
    (GUARD_ROWS + h + GUARD_ROWS, pitch) float32; the view starts at row GUARD_ROWS, column col_offset, so everything a kernel
    could read beside the pixels -- the tail of the last quad, the padding, the rows before and after -- is guard and lies
    inside memory the test owns."""
    import ctypes as C
    from kanter_core_amd import _lib
    L = _lib.load()
    planes = [np.ascontiguousarray(p, np.float32) for p in planes]
    assert len(planes) in (1, 4)
    h, w = planes[0].shape
    if isinstance(layouts, (str, tuple)):
        layouts = [layouts] * len(planes)
    assert len(layouts) == len(planes)
    handles, parents = [], []
    for p, lay in zip(planes, layouts):
        hnd = C.c_void_p()
        if lay == "pool":
            assert L.kc_plane_alloc(w, h, C.byref(hnd)) == 0
            assert L.kc_plane_upload_f32(hnd, p.ctypes.data, w * 4) == 0
        elif isinstance(lay, tuple) and lay[0] == "const":
            assert L.kc_plane_const(w, h, float(lay[1]), C.byref(hnd)) == 0
        else:
            pitch, off = wrap_layout(lay, w) if isinstance(lay, str) else lay
            assert pitch % 4 == 0 and off % 4 == 0 and off + (w + 3) // 4 * 4 <= pitch, (lay, w)
            host = np.full((GUARD_ROWS + h + GUARD_ROWS, pitch), guard, np.float32)
            host[GUARD_ROWS:GUARD_ROWS + h, off:off + w] = p
            t = torch.from_numpy(host).cuda()
            ptr = t.data_ptr() + (GUARD_ROWS * pitch + off) * 4
            assert L.kc_plane_wrap(ptr, w, h, pitch * 4, C.byref(hnd)) == 0, (lay, w, h)
            parents.append((t, host))
        handles.append(hnd)
    torch.cuda.synchronize()
    kc.sync()
    img = C.c_void_p()
    if len(planes) == 4:
        assert L.kc_image_rgba((C.c_void_p * 4)(*handles), C.byref(img)) == 0
    else:
        assert L.kc_image_gray(handles[0], C.byref(img)) == 0
    for hnd in handles:
        L.kc_plane_release(hnd)
    return WrappedImage(kc, torch, kc.SlotImage(img.value), planes, parents)


def kernel_resource_usage(unit, tmp):
    """{mangled kernel name: {"VGPRs": n, "ScratchSize": bytes per lane}} of every kernel of csrc/<unit> (a member of the
    build's SOURCES that includes bc_blocks.h), from a cross-compile with the build's own flags and
    -Rpass-analysis=kernel-resource-usage; the object goes to the directory `tmp`.  Skips the test without hipcc."""
    import pytest
    from kanter_core_amd import build as kbuild
    hipcc = kbuild._hipcc()
    if shutil.which(hipcc) is None and not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    assert unit in kbuild.SOURCES and "bc_blocks.h" in kbuild.HEADERS
    src = os.path.join(os.path.dirname(os.path.abspath(kbuild.__file__)), "csrc", unit)
    cmd = [hipcc] + kbuild.FLAGS + kbuild.DEVICE_FLAGS + ["-x", "hip", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                                                          "-o", os.path.join(str(tmp), os.path.splitext(unit)[0] + ".o")]
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
