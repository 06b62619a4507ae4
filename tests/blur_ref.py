"""The blur rule of include/kanter_core_amd.h (kc_image_blur) restated in numpy: f32 arrays, one rounding per operation, taps by
index gathers.  The weights here use numpy's own f64 exp; the tests that compare a kernel's bits pass the library's weights in."""
import math

import numpy as np

F = np.float32
MAX_RADIUS = 64


def radius(sigma):
    """R of a sigma > 0 (the f32 sigma, as the C ABI receives it)"""
    return max(1, int(math.ceil(3.0 * float(F(sigma)))))


def weights(sigma):
    """w_0..w_R as f32: g_k / total in f64, total = g_0 + 2 (g_1 + ... + g_R) summed in ascending k"""
    s = float(F(sigma))
    R = radius(sigma)
    g = [float(np.exp(np.float64(-float(k * k) / (2.0 * s * s)))) for k in range(R + 1)]
    side = 0.0
    for k in range(1, R + 1):
        side = side + g[k]
    total = g[0] + 2.0 * side
    return np.array([g[k] / total for k in range(R + 1)], np.float64).astype(F)


def texel(taps, w):
    """The rule on arrays of taps: taps[..., 0..2R], the centre at R -> f32 of the leading shape"""
    t = np.asarray(taps, F)
    w = np.asarray(w, F)
    R = len(w) - 1
    assert t.shape[-1] == 2 * R + 1 and R >= 1
    with np.errstate(all="ignore"):
        acc = w[R] * (t[..., 0] + t[..., 2 * R])
        for k in range(R - 1, 0, -1):
            acc = acc + w[k] * (t[..., R - k] + t[..., R + k])
        acc = acc + w[0] * t[..., R]
    return np.asarray(acc, F)


def tap_index(n, j, wrap):
    """positions i + j of an axis of n texels: clamped, or modulo n"""
    i = np.arange(n, dtype=np.int64) + j
    return i % n if wrap else np.clip(i, 0, n - 1)


def blur_axis(plane, w, axis, wrap):
    """One pass along `axis` (1: x, 0: y) of a 2-D f32 plane"""
    p = np.asarray(plane, F)
    w = np.asarray(w, F)
    R = len(w) - 1
    n = p.shape[axis]
    take = lambda j: np.take(p, tap_index(n, j, wrap), axis=axis)
    with np.errstate(all="ignore"):
        acc = w[R] * (take(-R) + take(R))
        for k in range(R - 1, 0, -1):
            acc = acc + w[k] * (take(-k) + take(k))
        acc = acc + w[0] * p
    assert acc.dtype == F
    return acc


def blur(plane, wx, wy, wrap):
    """x first, then y on the result; None leaves an axis out"""
    p = np.asarray(plane, F)
    if wx is not None:
        p = blur_axis(p, wx, 1, wrap)
    if wy is not None:
        p = blur_axis(p, wy, 0, wrap)
    return p


def conv_axis_f64(plane, w, axis, wrap):
    """The same pass with the same f32 weights and f32 input, every operation in f64: (result, sum_k w_k (|t_-k| + |t_k|))"""
    p = np.asarray(plane, F).astype(np.float64)
    w = np.asarray(w, F).astype(np.float64)
    R = len(w) - 1
    n = p.shape[axis]
    acc, mag = w[0] * p, w[0] * np.abs(p)
    for k in range(1, R + 1):
        a, b = np.take(p, tap_index(n, -k, wrap), axis=axis), np.take(p, tap_index(n, k, wrap), axis=axis)
        acc = acc + w[k] * (a + b)
        mag = mag + w[k] * (np.abs(a) + np.abs(b))
    return acc, mag
