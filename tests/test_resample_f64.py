"""The CPU oracle's resampler against an independent float64 one (CPU only).

The reference resamples with image::imageops::resize (crate image 0.24.0, imageops/sample.rs), called per plane from
src/shared.rs:159-199: a vertical pass (unclamped f32 result) and then a horizontal pass, clamped to [0, 1]. Per axis of
`n_in` samples resampled to `n_out`, for output index o:

    ratio  = n_in as f32 / n_out as f32      sratio = max(ratio, 1)      S = support * sratio
    c      = (o as f32 + 0.5) * ratio
    left   = clamp(floor(c - S), 0, n_in - 1)
    right  = clamp(ceil(c + S), left + 1, n_in)
    w_i    = K((i as f32 - (c - 0.5)) / sratio)   for i in left .. right, divided by their sum

with these kernels K and supports: Nearest = box (support 0), Triangle = 1 - |x| (support 1), CatmullRom = the
Mitchell-Netravali BC-spline with B = 0, C = 0.5 (support 2), Gaussian = exp(-x^2 / (2 r^2)) / (sqrt(2 pi) r) with
r = 0.5 (support 3), Lanczos3 = sinc(x) sinc(x / 3) for |x| < 3 (support 3).

Here the window positions and kernel arguments are computed in f32 exactly as above (numpy float32 arithmetic rounds
every operation as Rust's f32 does); the kernel values, the normalisation and both passes are float64. Then:

* the oracle's windows (orc.resize_taps) equal these windows exactly;
* its normalised weights agree with the f64 ones to 2^-20 of the row's sum of |w| (relative to the row, so that it
  stays meaningful for the weights near a zero of the kernel), plus, for CatmullRom, the rounding of the f32 cubic
  whose terms cancel near |x| = 2 (`cancellation`);
* orc.resize_plane lies within the bound of `error_bound` of the f64 result;
* non-finite inputs give NaN at the same positions, and the infinities that reach the clamp give the same 0 or 1.
"""
import numpy as np
import pytest

from util import SEED_A, splitmix_plane

FILTERS = ["Nearest", "Triangle", "CatmullRom", "Gaussian", "Lanczos3"]
SUPPORT = {"Nearest": 0.0, "Triangle": 1.0, "CatmullRom": 2.0, "Gaussian": 3.0, "Lanczos3": 3.0}
U = 2.0 ** -24  # unit roundoff of f32


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


def kernel(filt, x):
    """The filter's kernel in float64 at the f32 arguments x."""
    x = np.asarray(x, np.float64)
    a = np.abs(x)
    if filt == "Nearest":
        return np.ones_like(x)
    if filt == "Triangle":
        return np.where(a < 1.0, 1.0 - a, 0.0)
    if filt == "CatmullRom":
        b, c = 0.0, 0.5
        inner = (12 - 9 * b - 6 * c) * a ** 3 + (-18 + 12 * b + 6 * c) * a ** 2 + (6 - 2 * b)
        outer = (-b - 6 * c) * a ** 3 + (6 * b + 30 * c) * a ** 2 + (-12 * b - 48 * c) * a + (8 * b + 24 * c)
        return np.where(a < 1.0, inner, np.where(a < 2.0, outer, 0.0)) / 6.0
    if filt == "Gaussian":
        r = 0.5
        return np.exp(-(x * x) / (2 * r * r)) / (np.sqrt(2 * np.pi) * r)
    if filt == "Lanczos3":
        return np.where(a < 3.0, np.sinc(x) * np.sinc(x / 3.0), 0.0)
    raise ValueError(filt)


def cancellation(filt, x):
    """4 u times this bounds the absolute rounding error of the f32 kernel at x beyond 5 u relative: the sum of the
    magnitudes of the terms of CatmullRom's cubics, which cancel near |x| = 2; 1 for Lanczos3, whose f32 sin arguments
    (pi x up to 3 pi) are rounded, which near a zero of the kernel is an absolute error; 0 for the others."""
    a = np.abs(np.asarray(x, np.float64))
    if filt == "Lanczos3":
        return np.where(a < 3.0, 1.0, 0.0)
    if filt != "CatmullRom":
        return np.zeros_like(a)
    return np.where(a < 1.0, 9 * a ** 3 + 15 * a ** 2 + 6, np.where(a < 2.0, 3 * a ** 3 + 15 * a ** 2 + 24 * a + 12, 0.0)) / 6.0


def windows(n_in, n_out, filt, scales=None):
    """(left, right, weights): per output index its window [left, right) from the f32 positions and its normalised f64
    weights (a list of arrays); `scales`, when a list, receives cancellation() / |sum K| per row."""
    f32 = np.float32
    ratio = f32(n_in) / f32(n_out)
    sratio = max(ratio, f32(1.0))
    s = f32(SUPPORT[filt]) * sratio
    left, right, ws = [], [], []
    for o in range(n_out):
        c = (f32(o) + f32(0.5)) * ratio
        l = min(max(int(np.floor(c - s)), 0), n_in - 1)
        r = min(max(int(np.ceil(c + s)), l + 1), n_in)
        arg = (np.arange(l, r).astype(f32) - (c - f32(0.5))) / sratio  # f32 throughout
        assert arg.dtype == np.float32
        w = kernel(filt, arg)
        left.append(l)
        right.append(r)
        ws.append(w / w.sum())
        if scales is not None:
            scales.append(cancellation(filt, arg) / abs(w.sum()))
    return np.array(left), np.array(right), ws


def matrix(n_in, ws, left):
    m = np.zeros((len(ws), n_in))
    for o, w in enumerate(ws):
        m[o, left[o]:left[o] + len(w)] = w
    return m


def resample_f64(x, w_out, h_out, filt):
    """Both passes in float64 over the windows only (vertical, then horizontal; the clamp is the caller's).  Returns the
    result and, per axis, (matrix of the weights, matrix of their cancellation scales, normalised weight rows)."""
    h_in, w_in = x.shape
    sv, sh = [], []
    lv, _, wv = windows(h_in, h_out, filt, sv)
    lh, _, wh = windows(w_in, w_out, filt, sh)
    x = x.astype(np.float64)
    t = np.empty((h_out, w_in))
    y = np.empty((h_out, w_out))
    with np.errstate(invalid="ignore", over="ignore"):
        for o, w in enumerate(wv):
            t[o] = w @ x[lv[o]:lv[o] + len(w)]
        for o, w in enumerate(wh):
            y[:, o] = t[:, lh[o]:lh[o] + len(w)] @ w
    return y, (matrix(h_in, wv, lv), matrix(h_in, sv, lv), wv), (matrix(w_in, wh, lh), matrix(w_in, sh, lh), wh)


def error_matrix(axis):
    """Per weight of an axis, the most its f32 counterpart and its share of the f32 accumulation can add to a result, in
    units of the |x| they multiply (see error_bound)."""
    m, scales, ws = axis
    n = max(len(w) for w in ws)
    rho = max(max(np.abs(w).sum() / abs(w.sum()), 1.0) for w in ws)
    return U * ((n * (1.0 + rho) + 6.0) * np.abs(m) + 4.0 * scales)


def error_bound(x, v, h):
    """Per output, the bound (E_v |x|) |M_h|^T + (|M_v| |x|) E_h^T on |oracle - f64| before the clamp, where M is an axis's
    matrix of normalised weights and E = error_matrix(axis) = u ((n (1 + rho) + 6) |M| + 4 C).

    Derivation (first order in u = 2^-24; n = the most taps of an axis, rho = the largest sum |w| / |sum w| of its rows
    before normalisation, at least 1; C = cancellation() / |sum K| per weight):
      * an f32 weight carries the kernel evaluation (sin / exp / divisions: at most 5 u relative, and CatmullRom's cubic
        4 u of the magnitude of its terms: 4 u C) and the division by the f32 sum of its row, whose sequential
        accumulation is off by at most (n - 1) u sum |w|, i.e. (n - 1) rho u relative to the sum: at most
        ((n - 1) rho + 6) u |w| + 4 u C per weight;
      * a pass is a dot product of at most n terms accumulated in f32 from 0.0: at most n u of sum |w x|;
      * the horizontal pass carries the vertical pass's error through |M_h|; the clamp to [0, 1] never widens a
        difference.
    A subnormal source adds an absolute error of a few 2^-149 per operation, covered by 2^-140."""
    ax = np.abs(x.astype(np.float64))
    ev, eh = error_matrix(v), error_matrix(h)
    return (ev @ ax) @ np.abs(h[0]).T + (np.abs(v[0]) @ ax) @ eh.T + 2.0 ** -140


# (n_in, n_out): ratios of about 1/8, 1/3.7, 1/2, 0.97, 1.03, 2, 4.29 and 8 (ratio = in / out), 1-sample axes
AXES = [(13, 104), (17, 63), (16, 32), (97, 100), (103, 100), (34, 17), (3000, 700), (256, 32), (1, 7), (7, 1), (1, 1),
        (11, 3), (5, 17)]


@pytest.mark.parametrize("filt", FILTERS)
def test_windows_and_weights(orc, filt):
    axes = AXES + [(i, o) for i in range(1, 18) for o in range(1, 18)]
    for n_in, n_out in axes:
        scales = []
        left, right, ws = windows(n_in, n_out, filt, scales)
        ol, oc, ow = orc.resize_taps(n_in, n_out, filt)
        assert np.array_equal(ol, left), (filt, n_in, n_out, "left")
        assert np.array_equal(oc, right - left), (filt, n_in, n_out, "count")
        for o, w in enumerate(ws):
            got = ow[o, :len(w)].astype(np.float64)
            tol = 2.0 ** -20 * np.abs(w).sum() + 4 * U * scales[o]
            assert (np.abs(got - w) <= tol).all(), (filt, n_in, n_out, o, np.abs(got - w).max() / np.abs(w).sum())
            assert not ow[o, len(w):].any(), (filt, n_in, n_out, o, "weights past the window")


SHAPES = [  # (source (w, h), destination (w, h))
    ((104, 96), (13, 12)),     # 1/8
    ((63, 59), (17, 16)),      # about 1/3.7
    ((64, 34), (32, 17)),      # 1/2
    ((97, 33), (100, 34)),     # 0.97, 1.03 in the other direction
    ((103, 35), (100, 34)),
    ((17, 9), (34, 18)),       # 2
    ((7, 300), (30, 70)),      # 4.29 across, 1/4.29 down
    ((5, 3), (40, 24)),        # 8
    ((1, 17), (9, 5)),         # 1-pixel axes
    ((17, 1), (3, 11)),
    ((1, 1), (4, 3)),
    ((9, 11), (1, 1)),
]


def source(h, w, seed):
    return splitmix_plane(SEED_A + seed, 0, h, w) * np.float32(1.5) - np.float32(0.25)  # [-0.25, 1.25): the clamp matters


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("src,dst", SHAPES)
def test_resize_plane_within_the_f64_bound(orc, filt, src, dst):
    (sw, sh), (dw, dh) = src, dst
    x = source(sh, sw, sw * 31 + sh)
    x[0, 0] = np.float32(5.877e-39)  # a subnormal
    y, v, h = resample_f64(x, dw, dh, filt)
    want = np.clip(y, 0.0, 1.0)
    got = orc.resize_plane(x, dw, dh, filt).astype(np.float64)
    bound = error_bound(x, v, h)
    err = np.abs(got - want)
    assert (err <= bound).all(), (filt, src, dst, float((err / bound).max()))


def unresolved(x, v, h):
    """Outputs whose f64 sign or NaN-ness f32 arithmetic need not reproduce: an infinite input (or intermediate) meets a
    weight within its absolute error of 0 (a weight near a zero of the kernel: its f32 sign need not be the f64 one)."""
    def weak(axis):
        m, scales, _ = axis
        return (m != 0) & (np.abs(m) <= 8 * U * scales)

    bad = ~np.isfinite(x)
    with np.errstate(invalid="ignore", over="ignore"):
        t_weak = (weak(v).astype(np.float64) @ bad) > 0
        t_bad = ((np.abs(v[0]) @ np.where(bad, 1.0, 0.0)) > 0) | t_weak
        return ((t_weak.astype(np.float64) @ (h[0] != 0).T) > 0) | ((t_bad.astype(np.float64) @ weak(h).T) > 0)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("src,dst", [((33, 29), (11, 9)), ((13, 11), (40, 29)), ((17, 17), (16, 18)), ((1, 9), (3, 4))])
def test_non_finite_positions(orc, filt, src, dst):
    (sw, sh), (dw, dh) = src, dst
    x = source(sh, sw, 7)
    x[sh // 2, sw // 2] = np.nan
    x[0, sw - 1] = np.inf
    x[sh - 1, 0] = -np.inf
    if sh > 3 and sw > 3:
        x[sh // 3, sw // 3] = np.inf
        x[sh // 3 + 1, sw // 3] = -np.inf  # vertical neighbours: inf + -inf = NaN where both are in a window
        x[1, 1] = -0.0
        x[2, 2] = np.float32(1e30)
    y, v, h = resample_f64(x, dw, dh, filt)
    got = orc.resize_plane(x, dw, dh, filt)
    sure = ~unresolved(x, v, h)
    assert sure.mean() > 0.5, (filt, src, dst)  # most outputs are decided
    assert np.array_equal(np.isnan(got) & sure, np.isnan(y) & sure), (filt, src, dst, "NaN positions")
    assert np.isnan(y).any() == np.isnan(got).any(), (filt, src, dst)
    inf = np.isinf(y) & sure
    assert np.array_equal(got[inf], np.where(y[inf] > 0, 1.0, 0.0).astype(np.float32)), (filt, src, dst, "clamped infinities")
