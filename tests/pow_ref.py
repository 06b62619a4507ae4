"""A high-precision reference for Mix(Pow) (f32::powf, src/node/mix.rs:189) and the input regions its tests sample.

correctly_rounded(a, b): pow in float64 (np.power) rounded to f32 once; the samples whose f64 value lies within 2^-20 of an
f32 ulp of a rounding boundary are settled with mpmath at 120 bits (np.power's own error, < 1 f64 ulp, is 2^-28 f32 ulps).

pow_band(a, b, v): the error bound of the library's pow_positive (kanter_core_amd/csrc/pow_positive.inc) on its f64 value,
in f32 ulps of the result.  Derivation, with u = 2^-53 the f64 unit roundoff, a = z 2^k, z = c_i (1 + r):
  log2 a = k + log2 c_i + r P6(r).  Truncation of r P6(r): < 2^-40.9 |log2(1 + r)|, and |log2(1 + r)| < 0.036 (|r| < 2^-5.4).
    Roundings: the table's log2 c_i (u / 2), k + log2 c_i (u (|k| + 1)), Horner on r P6(r) (< 4 u |r P6(r)|), the last fma
    (u |l2|): together < 2^-52 (|l2| + 2).  On the interval around 1 (c_i = 1, k = 0, r = a - 1 exactly) only the Horner and
    the fma roundings remain: < 2^-52 |l2|, and the truncation is relative to |l2| itself.
    E_l2 = 2^-40.9 L + 2^-51 (|l2| + 2), L = 0.036;  around 1: E_l2 = 2^-40.9 |l2| + 2^-51 |l2|.
  y = b l2: |E_y| <= |b| E_l2 + u |y|.
  2^y = 2^(kd / 32) (1 + f Q4(f)): truncation < 2^-48 relative; Horner, the fma with 1, the table entry and the product: < 4 u.
  Relative error of the f64 value: R = ln 2 E_y + 2^-48 + 2^-51 (>= 4 u).  Band = 2 R |v| / (f32 ulp step), with a factor 2
  for what the bound leaves out (second-order terms).
Outside the band around an f32 rounding boundary the f32 result must be the correctly rounded one; inside it, either
neighbour of the boundary is the contract (pow_positive.inc: "the correctly rounded power except when the exact value lies
that close to a rounding boundary")."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
TIE_SETTLE = 2.0 ** -20  # f32 ulps from a rounding boundary below which mpmath decides


def _f32(x):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(np.float32)


def _pow64(a, b):
    with np.errstate(all="ignore"):
        return np.power(np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64))


def boundary_distance(v, r):
    """Distance, in f32 ulp steps, of the f64 value v from the rounding boundary between r = f32(v) and the f32 neighbour
    on v's side (0.5 - |frac|: 0 on the boundary); and that neighbour.  Exact values (v == r) and infinite v are 0.5 away."""
    v = np.asarray(v, np.float64)
    r = np.asarray(r, np.float32)
    with np.errstate(all="ignore"):
        toward = np.where(v >= r.astype(np.float64), np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
        alt = np.nextafter(r, toward)
        step = np.abs(alt.astype(np.float64) - r.astype(np.float64))
        # at the top of the range the neighbour of FLT_MAX is inf: the boundary is FLT_MAX + 2^103
        step = np.where(np.isfinite(step), step, 2.0 ** 104)
        base = np.where(np.isinf(r), np.sign(v) * FLT_MAX, r.astype(np.float64))
        frac = np.abs(v - base) / step
        frac = np.where(np.isinf(r), 1.0 - frac, frac)  # r = inf: measured from FLT_MAX
        d = np.abs(0.5 - frac)
    d = np.where(np.isfinite(v) & np.isfinite(d) & (v != r.astype(np.float64)), d, 0.5)
    return d, alt, step


def _mp_pow_f32(a, b):
    """pow(a, b) of two f32 values, correctly rounded to f32 (round half to even), at 120 bits."""
    import mpmath
    with mpmath.workprec(120):
        x = mpmath.power(mpmath.mpf(float(a)), mpmath.mpf(float(b)))
        with np.errstate(over="ignore"):
            lo = np.float32(float(x))  # an f32 next to x (f64 first, then f32: within one step)
        cands = {np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))}
        best = None
        for c in sorted(cands, key=lambda c: float(c)):
            if not np.isfinite(c):
                continue
            e = abs(mpmath.mpf(float(c)) - x)
            key = (e, int(np.array(c, np.float32).view(np.uint32)) & 1)
            if best is None or key < best[0]:
                best = (key, c)
        c = best[1]
        if abs(c) == np.float32(FLT_MAX) and abs(x) >= mpmath.mpf(FLT_MAX) + mpmath.mpf(2) ** 103:
            return np.float32(np.inf) if x > 0 else np.float32(-np.inf)
        return np.float32(c)


def correctly_rounded(a, b):
    """(f32 correctly rounded pow, its f64 value, indices settled by mpmath) for f32 arrays a, b of positive finite bases
    and finite exponents (every sample of the regions below)."""
    a = np.asarray(a, np.float32).reshape(-1)
    b = np.asarray(b, np.float32).reshape(-1)
    v = _pow64(a, b)
    r = _f32(v)
    d, _, _ = boundary_distance(v, r)
    near = np.flatnonzero(d < TIE_SETTLE)
    for i in near:
        r[i] = _mp_pow_f32(a[i], b[i])
    return r, v, near


def pow_band(a, b, v):
    """The f32 ulps around a rounding boundary inside which pow_positive may return either neighbour (module docstring)."""
    a = np.asarray(a, np.float32).reshape(-1)
    b = np.asarray(b, np.float32).reshape(-1).astype(np.float64)
    bits = a.view(np.uint32)
    with np.errstate(all="ignore"):
        l2 = np.log2(a.astype(np.float64))
        y = b * l2
        near1 = (bits >= 0x3f7f0000) & (bits < 0x3f830000)
        e_l2 = np.where(near1, (2.0 ** -40.9 + 2.0 ** -51) * np.abs(l2), 2.0 ** -40.9 * 0.036 + 2.0 ** -51 * (np.abs(l2) + 2))
        e_y = np.abs(b) * e_l2 + 2.0 ** -53 * np.abs(y)
        rel = np.log(2.0) * e_y + 2.0 ** -48 + 2.0 ** -51
        r = _f32(v)
        _, _, step = boundary_distance(v, r)
        band = 2 * rel * np.abs(v) / step
    return np.where(np.isfinite(band), band, 0.0)


def contract_failures(got, a, b):
    """Indices where `got` (f32, pow(a, b) by the library) breaks the contract; and the fraction of samples in the band."""
    got = np.asarray(got, np.float32).reshape(-1)
    cr, v, near = correctly_rounded(a, b)
    band = pow_band(a, b, v)
    d, alt, _ = boundary_distance(v, cr)
    for i in near:  # settled by mpmath: the f64 value is not trusted to say which side; accept the boundary's other neighbour
        d[i] = 0.0
        alt[i] = np.nextafter(cr[i], np.float32(np.inf)) if v[i] > float(cr[i]) else np.nextafter(cr[i], np.float32(-np.inf))
    in_band = d < band
    ok = (got.view(np.uint32) == cr.view(np.uint32)) | (in_band & (got.view(np.uint32) == alt.view(np.uint32)))
    return np.flatnonzero(~ok), float(in_band.mean())


# ---------------------------------------------------------------------------------------------------- the regions
def _bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


def _exp_for(rng, a, y_lo, y_hi):
    """Exponents b (f32) that put b log2 a in [y_lo, y_hi]."""
    y = rng.uniform(y_lo, y_hi, a.shape)
    with np.errstate(all="ignore"):
        return _f32(y / np.log2(a.astype(np.float64)))


def region(name, n, seed=0):
    """(a, b): n f32 pairs, positive finite bases and finite exponents."""
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    if name == "image":
        a = _f32(rng.integers(1, 1 << 24, n) * 2.0 ** -24)
        b = _f32(rng.integers(0, 1 << 24, n) * 2.0 ** -22)  # [0, 4)
    elif name == "positive":
        a = _bits(rng.integers(1, 0x7f800000, n))
        b = _f32(rng.uniform(-4, 4, n))
    elif name == "near_one":
        k = rng.integers(1, 2049, n) * rng.choice([-1, 1], n)
        a = _bits(0x3f800000 + k)
        b = _exp_for(rng, a, -150.0, 128.0)
    elif name == "table_edges":
        i = rng.integers(0, 32, n)
        binade = rng.integers(-12, 13, n)
        d = rng.integers(-1, 2, n)
        a = _bits((0x3f330000 + (i << 18) + d + (binade << 23)).astype(np.int64))
        b = _f32(rng.uniform(-8, 8, n))
    elif name == "subnormal":
        a = _bits(rng.integers(1, 0x00800000, n))
        b = _f32(rng.uniform(-1.1, 1.0, n))
    elif name == "extremes":
        big = rng.random(n) < 0.5
        a = np.where(big, _bits(rng.integers(0x40000000, 0x7f800000, n)), _bits(rng.integers(0x00800000, 0x3f000001, n)))
        top = rng.random(n) < 0.5
        b = np.where(top, _exp_for(rng, a, 126.0, 128.5), _exp_for(rng, a, -151.0, -125.0))
    elif name == "clamp":
        a = _bits(rng.integers(0x35800000, 0x49800000, n))  # [2^-20, 2^20]
        a = np.where(a == 1.0, np.float32(2.0), a)
        sign = rng.choice([-1.0, 1.0], n)
        b = _exp_for(rng, a, 290.0, 1000.0) * _f32(sign)
    else:
        raise KeyError(name)
    ok = np.isfinite(b) & (a > 0) & np.isfinite(a)
    b = np.where(ok, b, np.float32(1.0)).astype(np.float32)
    a = np.where(ok, a, np.float32(0.5)).astype(np.float32)
    return a, b


REGIONS = ["image", "positive", "near_one", "table_edges", "subnormal", "extremes", "clamp"]

# about two dozen special values: every pair of them is checked bit for bit, the sign of a zero included
SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1.0, -1.0, 2.0, -2.0, -8.0, 0.5, -0.5, 1.0 / 3.0, FLT_MAX, -FLT_MAX,
                     np.inf, -np.inf, np.nan, 1e-30, -1e-30, 3.0, -3.0, 0.25, -2.5, 7.0], np.float32)


def special_pairs():
    a, b = np.meshgrid(SPECIALS, SPECIALS, indexing="ij")
    return a.astype(np.float32), b.astype(np.float32)


def f64_rounded(a, b):
    """pow in float64 rounded to f32: what a routine that evaluates pow in f64 and rounds once gives."""
    return _f32(_pow64(a, b))
