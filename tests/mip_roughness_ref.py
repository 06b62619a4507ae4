"""The roughness-chain contract of include/kanter_core_amd.h (kc_image_build_roughness_mips) in numpy float32.  Level 0 of the
normal map is decoded to unit vectors, unit(); their plain chains m (mip_ref.chain, vector space, never renormalised) and the
plain chain r of the roughness plane give every level k >= 1 as texel(m_k, r_k, power): r where the footprint is flat or r is
NaN, 1 where the normals cancel, r raised by the normals' variance in between.  np.sqrt and / on float32 are correctly rounded."""
import numpy as np

import mip_ref

F = np.float32
FLOOR = F(2.0 ** -14)


def unit(ex, ey, ez):
    """The stored texels of a normal map (arrays of one shape, or scalars) -> the three float32 arrays of their unit vectors."""
    e = [np.asarray(x, F) for x in (ex, ey, ez)]
    with np.errstate(all="ignore"):
        v = [x * F(2.0) - F(1.0) for x in e]
        l = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        ok = (l > F(0.0)) & (l < F(np.inf))  # false for NaN
        safe = np.where(ok, l, F(1.0))
        u = [np.where(ok, x / safe, F(f)).astype(F) for x, f in zip(v, (0.0, 0.0, 1.0))]
    assert all(x.dtype == F for x in u)
    return u


def texel(mx, my, mz, r, power):
    """rough(m, r, power): the stored texel of the boxes (arrays of one shape, or scalars) -> float32 array of that shape."""
    mx, my, mz, r = [np.asarray(x, F) for x in (mx, my, mz, r)]
    power = F(power)
    with np.errstate(all="ignore"):
        l = np.sqrt((mx * mx + my * my) + mz * mz)
        t = (F(1.0) - l) / np.where(l == F(0.0), F(1.0), l)
        te = t - FLOOR
        rc = np.minimum(np.maximum(r, F(0.0)), F(1.0))
        a = rc * rc
        a2 = a * a
        B = ((F(2.0) * te) * power) * (a2 - F(1.0))
        n = (B - a2) / (B - F(1.0))
        d = np.sqrt(np.sqrt(n))
        out = np.where(t > FLOOR, d, r)      # !(t > floor), NaN included: the plain box
        out = np.where(l == F(0.0), F(1.0), out)
        out = np.where(r != r, r, out)
    out = np.asarray(out, F)
    assert out.dtype == F
    return out


def chain(rho, X, Y, Z, power):
    """All levels of the roughness plane rho beside the normal map's stored X, Y, Z -> levels, level 0 first (rho itself)."""
    r = mip_ref.chain(rho)
    m = [mip_ref.chain(u) for u in unit(X, Y, Z)]
    return [r[0]] + [np.ascontiguousarray(texel(m[0][k], m[1][k], m[2][k], r[k], power), F) for k in range(1, len(r))]
