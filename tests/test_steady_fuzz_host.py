"""The generator of the steady-state fuzz (tests/steady_fuzz.py) on the host, no GPU: it is deterministic, the reference refuses
at most one quarter of its graphs, and its sources are what their kinds claim."""
import functools

import numpy as np
import pytest

import steady_fuzz as sf

SWEEPS = [("forced", sf.SEED_FORCED, sf.N_FORCED, False), ("natural", sf.SEED_NATURAL, sf.N_NATURAL, False), ("pow", sf.SEED_POW, sf.N_POW, True)]


@functools.lru_cache(maxsize=None)
def _orc():
    from oracle import oracle as orc
    return orc


@pytest.mark.parametrize("name,base,n,pow_ops", SWEEPS, ids=[s[0] for s in SWEEPS])
def test_the_same_seed_gives_the_same_graph(name, base, n, pow_ops):
    for seed in range(base, base + n, 7):
        a, b = sf.random_case(_orc(), seed, pow_ops), sf.random_case(_orc(), seed, pow_ops)
        assert a.json() == b.json() and a.root == b.root and a.plugs == b.plugs and a.cache_policy == b.cache_policy, hex(seed)
        assert sorted(a.sources) == sorted(b.sources)
        for eid in a.sources:
            sa, sb = a.sources[eid], b.sources[eid]
            assert (sa.kind, sa.clean) == (sb.kind, sb.clean) and (sa.px is None) == (sb.px is None)
            assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(sa.planes, sb.planes)), hex(seed)
    assert sf.random_case(_orc(), base, pow_ops).json() != sf.random_case(_orc(), base + 1, pow_ops).json()


@pytest.mark.parametrize("name,base,n,pow_ops", SWEEPS, ids=[s[0] for s in SWEEPS])
def test_the_reference_refuses_at_most_a_quarter(name, base, n, pow_ops):
    """A graph whose requested node the reference refuses verifies no kernel: the device only has to raise as well."""
    refused = sum(sf.random_case(_orc(), base + s, pow_ops).want() is None for s in range(n))
    print("%s: the reference refuses %d of %d graphs" % (name, refused, n))
    assert 4 * refused <= n, (name, refused, n)


def test_the_sources_are_what_their_kinds_claim():
    seen = {(k, c): 0 for k in sf.KINDS for c in (True, False)}
    from_u8 = 0
    for seed in range(sf.SEED_FORCED, sf.SEED_FORCED + sf.N_FORCED):
        for s in sf.random_case(_orc(), seed).sources.values():
            seen[(s.kind, s.clean)] += 1
            from_u8 += s.px is not None
            for p in s.planes:
                assert p.dtype == np.float32
                if not s.clean:
                    continue
                assert np.isfinite(p).all()
                if s.kind == "fix24":
                    k = p.astype(np.float64) * 2.0 ** 24
                    assert np.array_equal(k, np.rint(k)) and k.min() >= 0 and k.max() <= 2.0 ** 24
                elif s.kind == "u8":
                    k = np.rint(p.astype(np.float64) * 255.0)
                    assert k.min() >= 0 and k.max() <= 255
                    assert np.array_equal(p.view(np.uint32), (k.astype(np.float32) / np.float32(255.0)).view(np.uint32))
                else:  # fits no tier: values below zero and off both grids
                    assert p.size < 12 or (p.min() < 0 and not np.array_equal(p * np.float32(2.0 ** 24), np.rint(p * np.float32(2.0 ** 24))))
    print("sources by (kind, clean):", seen, "made with from_u8:", from_u8)
    # every kind both clean (it packs, or -- f32 -- is refused for its values) and with edge values (it fails its tier)
    assert all(n >= 8 for n in seen.values()) and from_u8 >= 8, (seen, from_u8)
