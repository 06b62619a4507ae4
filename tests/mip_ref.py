"""The mip contract of include/kanter_core_amd.h in numpy float32: level k is the 2 x 2 box of level k - 1 as stored,
d(x, y) = ((s(x0, y0) + s(x1, y0)) + (s(x0, y1) + s(x1, y1))) * 0.25 with x1 = min(2x + 1, w - 1), y1 = min(2y + 1, h - 1)."""
import numpy as np


def level_count(w, h):
    return max(w, h).bit_length()  # 1 + floor(log2(max(w, h)))


def level_size(w, h, k):
    return max(1, w >> k), max(1, h >> k)


def reduce(level):
    """One level down: (h, w) float32 -> (max(1, h >> 1), max(1, w >> 1)) float32."""
    s = np.ascontiguousarray(level, np.float32)
    h, w = s.shape
    x0 = 2 * np.arange(max(1, w >> 1))
    y0 = 2 * np.arange(max(1, h >> 1))
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    with np.errstate(all="ignore"):
        top = s[np.ix_(y0, x0)] + s[np.ix_(y0, x1)]
        bottom = s[np.ix_(y1, x0)] + s[np.ix_(y1, x1)]
        out = (top + bottom) * np.float32(0.25)
    assert out.dtype == np.float32
    return out


def chain(image):
    """All levels of a plane, level 0 first, the last 1 x 1."""
    levels = [np.ascontiguousarray(image, np.float32)]
    while levels[-1].shape != (1, 1):
        levels.append(reduce(levels[-1]))
    return levels
