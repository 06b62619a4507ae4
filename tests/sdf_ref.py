"""The rule of kc_image_distance_field (include/kanter_core_amd.h, "Signed distance fields") restated in numpy: the class of a
texel, the squared distance to the nearest texel of the other class -- by definition over all pairs (d2_brute) and by a
windowed separable search for larger shapes (d2_windowed) -- the cap and the f64 value rule.  NONE stands for "the other class is
empty"; it is above every cap."""
import numpy as np

F = np.float32
NONE = np.int64(1) << 40
MAX_SPREAD = 254


def quant_u8(a):
    """to_u8's quantiser: ((v.clamp(0, 1) * 255.).min(255.)) as u8 in f32, NaN -> 255"""
    a = np.asarray(a, F)
    with np.errstate(invalid="ignore"):
        x = np.where(a < 0, F(0), a).astype(F)
        x = np.where(x > 1, F(1), x).astype(F)
        x = (x * F(255.0)).astype(F)
        x = np.where(x <= F(255.0), x, F(255.0))  # NaN fails the comparison
    return x.astype(np.uint8)


def inside(plane, B):
    return quant_u8(plane) >= B


def cap(S):
    return S * S + S + 1


def _axis_dist(n, wrap):
    """|i - j| for every pair of positions of an axis, or the torus distance"""
    d = np.abs(np.arange(n, dtype=np.int64)[:, None] - np.arange(n, dtype=np.int64)[None, :])
    return np.minimum(d, n - d) if wrap else d


def d2_brute(mask, wrap):
    """The definition: for every texel the smallest dx^2 + dy^2 over ALL texels of the other class (NONE without one)."""
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    dy2, dx2 = (_axis_dist(h, wrap) ** 2).astype(np.int32), (_axis_dist(w, wrap) ** 2).astype(np.int32)  # extents below 2^15
    out = np.full((h, w), NONE, np.int64)
    for cls in (False, True):
        oy, ox = np.nonzero(mask != cls)  # the other class of the texels of class cls
        if len(oy) == 0:
            continue
        for y in range(h):  # the texels of class cls row by row: a pair table of (texels of the row) x (the other class)
            tx = np.nonzero(mask[y] == cls)[0]
            for a in range(0, len(tx), 512):
                d = dx2[np.ix_(tx[a:a + 512], ox)]
                d += dy2[y, oy][None, :]
                out[y, tx[a:a + 512]] = d.min(axis=1)
    return out


def _shift(a, k, axis, wrap, fill):
    """a seen from k positions further along the axis: out[i] = a[i + k]; positions that do not exist hold `fill`"""
    if wrap:
        return np.roll(a, -k, axis=axis)
    n = a.shape[axis]
    out = np.full(a.shape, fill, a.dtype)
    if abs(k) >= n:
        return out
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis] = slice(k, n) if k > 0 else slice(0, n + k)
    dst[axis] = slice(0, n - k) if k > 0 else slice(-k, n)
    out[tuple(dst)] = a[tuple(src)]
    return out


def d2_windowed(mask, S, wrap):
    """The separable search with windows of radius S: exact for every texel whose D2 is below cap(S); the others hold some value
    >= cap(S).  Columns first (the distance along y to the nearest texel of each class, NONE beyond S), then rows."""
    mask = np.asarray(mask, bool)
    best = np.full(mask.shape, NONE, np.int64)
    for cls in (False, True):
        other = mask != cls
        g = np.where(other, np.int64(0), NONE)  # per texel: the distance along its column to the nearest texel of `other`
        for k in range(1, S + 1):
            for s in (k, -k):
                g = np.minimum(g, np.where(_shift(other, s, 0, wrap, False), np.int64(k), NONE))
        g2 = np.where(g >= NONE, NONE, g * g)
        d = g2.copy()
        for k in range(1, S + 1):
            for s in (k, -k):
                d = np.minimum(d, _shift(g2, s, 1, wrap, NONE) + k * k)
        best = np.where(mask == cls, d, best)
    return np.minimum(best, NONE)


def value(d2, mask, S):
    """The value rule: d2 after or before capping (anything >= cap(S) saturates), in f64, rounded to f32 once."""
    d2c = np.minimum(np.asarray(d2, np.int64), cap(S))
    mask = np.asarray(mask, bool)
    d = np.sqrt(d2c.astype(np.float64))
    sd = np.where(mask, d - 0.5, 0.5 - d)
    v = (0.5 + sd / (2.0 * S)).astype(F)
    return np.where(d2c == cap(S), np.where(mask, F(1.0), F(0.0)), v).astype(F)


def distance_field_brute(plane, B, S, wrap):
    m = inside(plane, B)
    return value(d2_brute(m, wrap), m, S)


def distance_field(plane, B, S, wrap):
    """The windowed form, for larger shapes"""
    m = inside(plane, B)
    return value(d2_windowed(m, S, wrap), m, S)
