"""The channel states of an RGBA image, enumerated, for the sweep of the mip families (test_gpu_mip_states.py, the conditions on
its inputs in test_mip_states_host.py, and the "mips_rules" rows of test_gpu_fuzz_consumers.py).

A pattern says, per channel, whether it is a constant (None) or which alias class of resident planes it belongs to (class
indices in restricted-growth order: the first resident channel is class 0).  There are 1 + 4 * 1 + 6 * 2 + 4 * 5 + 15 = 52 of
them.  state() turns a pattern and a shape into pixels: class j of pattern i lives in memory as KINDS[(i + j) % 5], so the
classes of one image differ in pitch and over the sweep every channel position meets every kind.  reference() composes the
expected chains from the families' own numpy references, computed once per distinct input and shared read-only.  build() makes
the image on the device, one plane handle per class.  Nothing here needs a device to import."""
import ctypes as C

import numpy as np

import mip_alpha_ref
import mip_coverage_ref
import mip_normals_ref
import mip_ref
import mip_roughness_ref
from util import GUARD_ROWS, wrap_layout

F = np.float32
# "pool" and "pending" (a pool plane once it is forced) have one pitch: they are two apart, so that the two classes of a
# two-class pattern, which take neighbouring kinds, never get both
KINDS = ["pool", "tight", "pending", "pad48", "offset"]
WRAPPED = ("tight", "pad48", "offset")
CONSTANTS = (0.8, 0.3, 0.9, 0.6)  # R, G, B, A
EXTRA_ALPHAS = (1.0, 0.0)  # a constant alpha also runs as weight 1 (the plain chain) and weight 0 (constant-zero colour)
SHAPES = [(130, 70), (37, 150)]  # (w, h)
COVERAGE_REF = 128
FLAG_SETS = [dict(), dict(normals=True), dict(coverage=COVERAGE_REF), dict(normals=True, coverage=COVERAGE_REF),
             dict(alpha_weighted=True), dict(alpha_weighted=True, coverage=COVERAGE_REF)]
SEEDED = np.array([-0.0, 1e-45, 1e-40, 2.0 ** -17, 2.0 ** -16, 2.0, -0.25, 1.5], F)


def flag_id(flags):
    return "+".join("%s=%s" % kv for kv in sorted(flags.items())) or "plain"


def reads_alpha(flags):
    """whether the flag set does anything with alpha beyond the plain rule"""
    return bool(flags.get("coverage") or flags.get("alpha_weighted"))


def patterns():
    """The 52 tuples, in a fixed order (the index is part of the test ids): channel by channel, a constant first, then the
    classes seen so far, then a new class.  Pattern 0 is four constants, the last one four planes of their own."""
    out = []

    def grow(prefix, classes):
        if len(prefix) == 4:
            out.append(tuple(prefix))
            return
        grow(prefix + [None], classes)
        for j in range(classes + 1):
            grow(prefix + [j], max(classes, j + 1))
    grow([], 0)
    return out


def pattern_index(pattern):
    return patterns().index(tuple(pattern))


def class_count(pattern):
    return len({j for j in pattern if j is not None})


def first_channel(pattern, j):
    return list(pattern).index(j)


def kinds_of(index, pattern, rotate=0):
    """the memory kind of every class of pattern number `index`"""
    return [KINDS[(index + j + rotate) % len(KINDS)] for j in range(class_count(pattern))]


def pool_pitch(w):
    """floats between the rows of a plane from the library's pool: 4 w bytes rounded up to 256"""
    return (4 * w + 255) // 256 * 64


def pitch_of(kind, w):
    """floats between the rows of a class of the kind, once it is resident"""
    return wrap_layout(kind, w)[0] if kind in WRAPPED else pool_pitch(w)


_BASE = {}


def base_plane(w, h, c):
    """Base plane c: cutout-like (35 % zeros, 15 % ones, an empty region that leaves the pull-push fill work above level 1) with
    eight seeded values, among them a negative zero, denormals and values outside [0, 1]; no NaN and no infinity."""
    if (w, h, c) not in _BASE:
        rng = np.random.default_rng([41, w, h, c])
        p = rng.random((h, w), dtype=F)
        u = rng.random((h, w))
        p[u < 0.35] = 0.0
        p[u > 0.85] = 1.0
        p[8:40, 8:24] = 0.0
        p.flat[c:c + 8] = SEEDED
        p.setflags(write=False)
        _BASE[w, h, c] = p
    return _BASE[w, h, c]


def pending_inputs(w, h, c):
    """the two planes whose Multiply is a pending class's pixels"""
    return base_plane(w, h, c), base_plane(w, h, c + 4)


def class_plane(w, h, c, kind):
    """the pixels of a class whose first channel is c"""
    if kind != "pending":
        return base_plane(w, h, c)
    key = (w, h, c, "pending")
    if key not in _BASE:
        from oracle import oracle as orc
        p = orc.mix_plane("Multiply", *pending_inputs(w, h, c))
        p.setflags(write=False)
        _BASE[key] = p
    return _BASE[key]


def const_plane(w, h, v):
    key = (w, h, "const", repr(F(v)))
    if key not in _BASE:
        p = np.full((h, w), v, F)
        p.setflags(write=False)
        _BASE[key] = p
    return _BASE[key]


class State:
    """One pattern at one shape: .index, .pattern, .w, .h, .kinds (per class), .values (per channel, the constant or None),
    .keys (per channel, hashable: two channels have one key exactly when they have the same pixels) and .planes (the pixels)."""

    def __init__(self, index, w, h, alpha=None, rotate=0):
        self.index, self.w, self.h = index, w, h
        self.pattern = patterns()[index]
        self.kinds = kinds_of(index, self.pattern, rotate)
        self.values = [None if j is not None else F(CONSTANTS[ch]) for ch, j in enumerate(self.pattern)]
        if alpha is not None:
            assert self.pattern[3] is None
            self.values[3] = F(alpha)
        self.keys, self.planes = [], []
        for ch, j in enumerate(self.pattern):
            if j is None:
                self.keys.append(("const", repr(self.values[ch])))
                self.planes.append(const_plane(w, h, self.values[ch]))
            else:
                c = first_channel(self.pattern, j)
                pending = self.kinds[j] == "pending"
                self.keys.append(("class", c, pending))
                self.planes.append(class_plane(w, h, c, self.kinds[j]))

    def resident(self, ch):
        return self.pattern[ch] is not None

    def __repr__(self):
        alpha = "" if self.pattern[3] is not None else " alpha=%r" % float(self.values[3])
        return "pattern %d %s kinds %s %dx%d%s" % (self.index, self.pattern, self.kinds, self.w, self.h, alpha)


def states(w, h, flags=None):
    """Every pattern at the shape; where the flag set reads alpha, the constant-alpha patterns with alpha 1 and 0 as well."""
    out = []
    for i, p in enumerate(patterns()):
        out.append(State(i, w, h))
        if p[3] is None and flags is not None and reads_alpha(flags):
            out.extend(State(i, w, h, alpha=a) for a in EXTRA_ALPHAS)
    return out


# ------------------------------------------------------------------ the references, once per distinct input
_REF = {}


def _cached(key, make):
    if key not in _REF:
        got = make()
        for lv in (got if isinstance(got[0], np.ndarray) else [l for ch in got for l in ch]):
            lv.setflags(write=False)
        _REF[key] = got
    return _REF[key]


def _key(plane, key):
    """a caller without keys (planes from elsewhere) gets one from the bits"""
    return key if key is not None else (plane.shape, hash(np.ascontiguousarray(plane, F).tobytes()))


def reference(planes, flags=None, keys=None):
    """-> per channel, the list of levels (level 0 first) of the image of `planes` (1 or 4) under the flag set `flags`: a dict of
    mips()'s keywords normals, coverage and alpha_weighted, or roughness=(channel, (X, Y, Z), power) for roughness_mips() (with
    roughness_keys=(kX, kY, kZ) beside `keys`).  Composed only from the families' reference modules.  keys: per channel, a
    hashable name of the pixels, under which a chain is computed once and shared read-only."""
    flags = dict(flags or {})
    planes = [np.ascontiguousarray(p, F) for p in planes]
    keys = [_key(p, k) for p, k in zip(planes, keys or [None] * len(planes))]
    shape = planes[0].shape

    def plain(ch):
        return _cached(("plain", shape, keys[ch]), lambda: mip_ref.chain(planes[ch]))
    out = [None] * len(planes)
    rough = flags.pop("roughness", None)
    rkeys = flags.pop("roughness_keys", None)
    if rough is not None:
        assert not flags
        channel, xyz, power = rough
        xyz = [np.ascontiguousarray(p, F) for p in xyz]
        rkeys = [_key(p, k) for p, k in zip(xyz, rkeys or [None] * 3)]
        out[channel] = _cached(("roughness", shape, keys[channel], tuple(rkeys), repr(F(power))),
                               lambda: mip_roughness_ref.chain(planes[channel], xyz[0], xyz[1], xyz[2], power))
    elif flags.get("normals"):
        assert not flags.get("alpha_weighted")
        out[:3] = _cached(("normals", shape, tuple(keys[:3])), lambda: mip_normals_ref.chain(*planes[:3]))
    elif flags.get("alpha_weighted"):
        out[:3] = _cached(("alpha", shape, tuple(keys)), lambda: mip_alpha_ref.chain(*planes))
    if flags.get("coverage"):
        out[3] = _cached(("coverage", shape, keys[3], flags["coverage"]), lambda: mip_coverage_ref.chain(planes[3], flags["coverage"])[0])
    return [plain(ch) if got is None else got for ch, got in enumerate(out)]


# ------------------------------------------------------------------ the device side
class Built:
    """What build() returns: .image (the SlotImage), .state, .parents ([(tensor, host copy)] of the wrapped classes) and whatever
    else has to stay alive."""

    def __init__(self, kc, torch, image, state, parents, keep):
        self.kc, self.torch, self.image, self.state, self.parents, self.keep = kc, torch, image, state, parents, keep

    def assert_untouched(self, what=""):
        """The source is only read: the image's planes are still the pixels, and every parent tensor still holds its host
        copy's bits -- the guard around the views included."""
        from util import assert_planes
        assert_planes(self.image.planes(), self.state.planes, what="%s: the image afterwards" % (what,))
        self.kc.sync()
        self.torch.cuda.synchronize()
        for k, (t, host) in enumerate(self.parents):
            now = t.cpu().numpy().view(np.uint32)
            assert np.array_equal(now, host.view(np.uint32)), "%s: parent tensor %d: %d words written" % (what, k, int((now != host.view(np.uint32)).sum()))


def build(kc, torch, state):
    """The RGBA image of a state: one plane handle per class (a pool plane, a view into a NaN-guarded parent tensor exactly as
    util.wrapped_image makes them, or a pending Gray Multiply), a constant plane per constant channel, and the same handle for
    every channel of a class."""
    from kanter_core_amd import _lib
    L = _lib.load()
    w, h = state.w, state.h
    parents, keep, handles, grays = [], [], [], []
    for j, kind in enumerate(state.kinds):
        c = first_channel(state.pattern, j)
        hnd = C.c_void_p()
        if kind == "pending":
            a, b = pending_inputs(w, h, c)
            grays.append(kc.mix_process(kc.SlotImage.from_planes([a]), kc.SlotImage.from_planes([b]), kc.MixType.Multiply))
            handles.append(None)
            continue
        p = class_plane(w, h, c, kind)
        if kind == "pool":
            assert L.kc_plane_alloc(w, h, C.byref(hnd)) == 0
            assert L.kc_plane_upload_f32(hnd, p.ctypes.data, w * 4) == 0
        else:
            pitch, off = wrap_layout(kind, w)
            assert pitch % 4 == 0 and off % 4 == 0 and off + (w + 3) // 4 * 4 <= pitch, (kind, w)
            host = np.full((GUARD_ROWS + h + GUARD_ROWS, pitch), np.nan, F)
            host[GUARD_ROWS:GUARD_ROWS + h, off:off + w] = p
            t = torch.from_numpy(host).cuda()
            ptr = t.data_ptr() + (GUARD_ROWS * pitch + off) * 4
            assert L.kc_plane_wrap(ptr, w, h, pitch * 4, C.byref(hnd)) == 0, (kind, w, h)
            parents.append((t, host))
        handles.append(hnd)
        grays.append(None)
    consts = {}
    for ch, v in enumerate(state.values):
        if v is not None:
            consts[ch] = C.c_void_p()
            assert L.kc_plane_const(w, h, float(v), C.byref(consts[ch])) == 0
    torch.cuda.synchronize()
    kc.sync()

    def gray_of(hnd):
        img = C.c_void_p()
        assert L.kc_image_gray(hnd, C.byref(img)) == 0
        return kc.SlotImage(img.value)
    if "pending" in state.kinds:  # CombineRgba takes the planes themselves, and leaves the chain pending
        for j, hnd in enumerate(handles):
            if hnd is not None:
                grays[j] = gray_of(hnd)
        parts = [gray_of(consts[ch]) if j is None else grays[j] for ch, j in enumerate(state.pattern)]
        image = kc.combine_rgba_process(parts)
        keep.append(parts)
    else:
        img = C.c_void_p()
        arr = (C.c_void_p * 4)(*[consts[ch] if j is None else handles[j] for ch, j in enumerate(state.pattern)])
        assert L.kc_image_rgba(arr, C.byref(img)) == 0
        image = kc.SlotImage(img.value)
    for hnd in list(consts.values()) + [x for x in handles if x is not None]:
        L.kc_plane_release(hnd)
    return Built(kc, torch, image, state, parents, keep)
