"""The KC_MIP_COVERAGE contract of include/kanter_core_amd.h in numpy, on top of mip_ref.py: the plain chain p_k of alpha, and for
every level k >= 1 the scale s_k that takes its T_k-th largest key to the reference byte B, T_k the share of level 0's covered
texels.  The stored level is p_k * s_k in float32; a level with T_k == 0 or with exactly T_k covered texels keeps p_k bit for bit.
numpy's float32 / and * are correctly rounded single operations."""
import collections

import numpy as np

import mip_ref

F = np.float32
FLOOR = F(2.0 ** -16)  # ve = max(v, FLOOR): alpha below one step of a 16-bit export counts as empty

Level = collections.namedtuple("Level", "texels target plain_covered v scale")


def threshold(ref):
    """r_B = (float)B / 255.0f"""
    return F(ref) / F(255.0)


def quant_u8(a):
    """kc_image_to_u8's linear quantiser: clamp, * 255, truncate, NaN -> 255."""
    a = np.asarray(a, F)
    with np.errstate(invalid="ignore"):
        x = np.where(a < 0, F(0.0), a)
        x = np.where(x > 1, F(1.0), x).astype(F) * F(255.0)
        x = np.where(x <= F(255.0), x, F(255.0))  # NaN -> 255
    return x.astype(np.uint32)


def key(a):
    """a clamped to [0, 1], NaN -> 1, -0.0 and anything not greater than 0 -> +0.0; float32."""
    a = np.asarray(a, F)
    with np.errstate(invalid="ignore"):
        k = np.where(a > 0, a, F(0.0))
        k = np.where(k > 1, F(1.0), k)
    return np.where(np.isnan(a), F(1.0), k).astype(F)


def covered(a, ref):
    """How many texels of the plane a renderer's test against the byte `ref` keeps."""
    return int((quant_u8(a) >= ref).sum())


def target(n0, nk, c0):
    return 0 if c0 == 0 else min(nk, max(1, (c0 * nk + n0 // 2) // n0))


def scale(v, ref):
    """s from the selected key v."""
    v = F(v)
    ve = v if v > FLOOR else FLOOR
    with np.errstate(all="ignore"):
        s = threshold(ref) / ve
        while quant_u8(ve * s) < ref:
            s = np.nextafter(s, F(np.inf))
    assert s.dtype == F
    return s


def kth_largest(plane, t):
    """The t-th largest key of the plane (1 <= t <= its texels)."""
    bits = key(plane).reshape(-1).view(np.uint32)  # non-negative floats order as their bit patterns
    return np.partition(bits, bits.size - t)[bits.size - t:bits.size - t + 1].view(F)[0]


def chain(alpha, ref):
    """-> (stored levels, [Level]): level 0 is the plane itself."""
    plain = mip_ref.chain(alpha)
    n0, c0 = plain[0].size, covered(plain[0], ref)
    levels, info = [plain[0]], [Level(n0, c0, c0, F(0.0), F(1.0))]
    for p in plain[1:]:
        t, pc = target(n0, p.size, c0), covered(p, ref)
        if t == 0 or pc == t:
            levels.append(p)
            info.append(Level(p.size, t, pc, F(0.0), F(1.0)))
            continue
        v = kth_largest(p, t)
        s = scale(v, ref)
        with np.errstate(all="ignore"):
            d = p * s
        assert d.dtype == F
        levels.append(d)
        info.append(Level(p.size, t, pc, v, s))
    return levels, info
