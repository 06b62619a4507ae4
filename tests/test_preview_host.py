"""kc_preview_level -- the mip level a thumbnail or a viewport of a given extent is cut from -- without a device: against
mip_ref.level_size over a sweep of sizes and extents, its refusals, and the Python names."""
import ctypes as C

import pytest

import mip_ref

KC_ERR_INVALID_ARG = 102


@pytest.fixture(scope="module")
def L():
    from kanter_core_amd import _lib
    return _lib.load()


def want_level(w, h, max_extent):
    k = 0
    while max(mip_ref.level_size(w, h, k)) > max_extent:
        k += 1
    return (k,) + mip_ref.level_size(w, h, k)


def test_preview_level_against_the_reference_sizes(L):
    from kanter_core_amd import api
    sizes = [(1, 1), (1, 5), (5, 1), (5, 3), (64, 64), (67, 45), (130, 70), (256, 16), (200, 130), (1024, 1024), (4096, 4096),
             (8192, 100), (3, 8191), (1 << 20, 7), (65535, 65537)]
    extents = [1, 2, 3, 63, 64, 65, 127, 128, 129, 256, 1000, 4096, 1 << 20, (1 << 32) - 1]
    for w, h in sizes:
        for e in extents:
            got = api.preview_level(w, h, e)
            assert got == want_level(w, h, e), (w, h, e, got)
            assert got[0] < mip_ref.level_count(w, h)
            assert max(got[1:]) <= e and (got[0] == 0 or max(mip_ref.level_size(w, h, got[0] - 1)) > e)
    k, pw, ph = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7)
    for w, h, e in ((0, 8, 8), (8, 0, 8), (8, 8, 0)):
        assert L.kc_preview_level(w, h, e, C.byref(k), C.byref(pw), C.byref(ph)) == KC_ERR_INVALID_ARG
    assert L.kc_preview_level(8, 8, 8, None, C.byref(pw), C.byref(ph)) == KC_ERR_INVALID_ARG
    assert L.kc_preview_level(8, 8, 8, C.byref(k), None, C.byref(ph)) == KC_ERR_INVALID_ARG
    assert L.kc_preview_level(8, 8, 8, C.byref(k), C.byref(pw), None) == KC_ERR_INVALID_ARG
    assert (k.value, pw.value, ph.value) == (7, 7, 7)  # a refusal writes nothing


def test_every_level_of_the_chain_is_the_answer_for_some_extent():
    from kanter_core_amd import api
    for w, h in ((4096, 4096), (130, 70), (256, 16), (1, 1)):
        n = api.mip_level_count(w, h)
        seen = {api.preview_level(w, h, e)[0] for e in range(1, max(w, h) + 1)}
        assert seen == set(range(n)), (w, h)  # every level of the chain is the answer for some extent, and no other
        assert api.preview_level(w, h, max(w, h)) == (0, w, h)
        assert api.preview_level(w, h, 1) == (n - 1, 1, 1)


def test_python_names():
    import kanter_core_amd as kc
    from kanter_core_amd import _lib, api
    assert kc.preview_level is api.preview_level and "kc_preview_level" in _lib.SIGNATURES
    assert api.preview_level(4096, 4096, 128) == (5, 128, 128)
    assert api.preview_level(1024, 256, 128) == (3, 128, 32)
    with pytest.raises(kc.TexProError) as e:
        api.preview_level(8, 8, 0)
    assert e.value.code == KC_ERR_INVALID_ARG
