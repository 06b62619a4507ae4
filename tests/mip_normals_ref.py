"""The KC_MIP_NORMALS contract of include/kanter_core_amd.h in numpy float32: a level is mip_ref.reduce of R, G and B of the
level above it as stored, then, per texel, on the three boxes b: v = b * 2 - 1, l = sqrt((v.x * v.x + v.y * v.y) + v.z * v.z),
u = v / l where l > 0 and l < inf, (0, 0, 1) elsewhere, d = u * 0.5 + 0.5.  np.sqrt and / on float32 are correctly rounded."""
import numpy as np

import mip_ref

F = np.float32


def normal_texel(bx, by, bz):
    """The stored texel of the boxes (arrays of one shape, or scalars) -> three float32 arrays of that shape."""
    b = [np.asarray(x, F) for x in (bx, by, bz)]
    with np.errstate(all="ignore"):
        v = [x * F(2.0) - F(1.0) for x in b]
        l = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        ok = (l > F(0.0)) & (l < F(np.inf))  # false for NaN
        safe = np.where(ok, l, F(1.0))
        u = [np.where(ok, x / safe, F(f)) for x, f in zip(v, (0.0, 0.0, 1.0))]
        d = [x * F(0.5) + F(0.5) for x in u]
    assert all(x.dtype == F for x in d)
    return d


def chain(r, g, b):
    """All levels of the three planes -> [r levels, g levels, b levels], level 0 first (the planes themselves), the last 1 x 1."""
    levels = [[np.ascontiguousarray(p, F)] for p in (r, g, b)]
    while levels[0][-1].shape != (1, 1):
        d = normal_texel(*[mip_ref.reduce(c[-1]) for c in levels])
        for c, x in zip(levels, d):
            c.append(np.ascontiguousarray(x, F))
    return levels
