"""CPU checks of the Pow reference (tests/pow_ref.py) that test_gpu_pow.py holds the library's Pow routes to, and of the
oracle's powf against it."""
import numpy as np
import pytest

import pow_ref as P
from util import max_ulp


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


def _mp_f32(a, b):
    return np.array([P._mp_pow_f32(x, y) for x, y in zip(a, b)], np.float32)


def test_reference_agrees_with_mpmath():
    """correctly_rounded equals pow at 120 bits rounded to f32 on samples of every region and on samples next to a rounding
    boundary: bases 1 + k 2^-23 with exponents 2^j (exact squares of an odd mantissa sit on f32 midpoints) and their f32
    neighbours."""
    rng = np.random.default_rng(11)
    a, b = [], []
    for name in P.REGIONS:
        ra, rb = P.region(name, 1 << 12, seed=5)
        i = rng.choice(len(ra), 400, replace=False)
        a.append(ra[i])
        b.append(rb[i])
    # near ties: (1 + k 2^-12)^2 = 1 + k 2^-11 + k^2 2^-24 has 25 significant bits for odd k below 2^11.5 (a square under 2):
    # on an f32 midpoint exactly; a neighbouring exponent moves it just off
    k = rng.integers(0, 848, 600) * 2 + 1
    base = (1.0 + k * 2.0 ** -12).astype(np.float32)
    two = np.full(600, 2.0, np.float32)
    a += [base, base, base]
    b += [two, np.nextafter(two, np.float32(3)), np.nextafter(two, np.float32(1))]
    a, b = np.concatenate(a), np.concatenate(b)
    cr, v, near = P.correctly_rounded(a, b)
    mp = _mp_f32(a, b)
    assert len(near) >= 600, "the exact midpoints must be settled by mpmath, %d were" % len(near)
    bad = np.flatnonzero(cr.view(np.uint32) != mp.view(np.uint32))
    assert not len(bad), list(zip(a[bad][:5], b[bad][:5], cr[bad][:5], mp[bad][:5]))


@pytest.mark.parametrize("name", P.REGIONS)
def test_band_is_narrow(name):
    """The pow_positive error band covers under 2^-8 of every region: a loose bound cannot hide errors."""
    a, b = P.region(name, 1 << 18)
    _, v, _ = P.correctly_rounded(a, b)
    d, _, _ = P.boundary_distance(v, P._f32(v))
    assert float((d < P.pow_band(a, b, v)).mean()) < 2.0 ** -8


@pytest.mark.parametrize("name", P.REGIONS)
def test_oracle_powf_within_one_ulp_of_correctly_rounded(orc, name):
    a, b = P.region(name, 1 << 18)
    got = orc.mix_plane("Pow", a.reshape(512, 512), b.reshape(512, 512)).reshape(-1)
    cr, _, _ = P.correctly_rounded(a, b)
    assert max_ulp(got, cr) <= 1


def test_oracle_powf_is_exact_on_the_special_values(orc):
    a, b = P.special_pairs()
    got = orc.mix_plane("Pow", a, b)
    want = P.f64_rounded(a, b)
    bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), list(zip(a[bad][:8], b[bad][:8], got[bad][:8], want[bad][:8]))
    # the table holds what it should: signed zeros and infinities, odd and even integers, non-integers of negative bases
    assert np.isnan(got[list(P.SPECIALS).index(-8.0), list(P.SPECIALS).index(0.5)])
    neg0 = 1
    assert P.SPECIALS[neg0] == 0 and np.signbit(P.SPECIALS[neg0])
    assert got[neg0, list(P.SPECIALS).index(3.0)].view(np.uint32) == np.float32(-0.0).view(np.uint32)
    assert got[neg0, list(P.SPECIALS).index(-1.0)] == -np.inf
