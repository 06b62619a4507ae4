"""The alpha-weighted mip contract of include/kanter_core_amd.h (KC_MIP_ALPHA_WEIGHT) in numpy float32.  Level 0's alpha gives
every texel a weight, weight(); the premultiplied colour p_c = c * w0 and the weight go down the plain rule (mip_ref.chain); a
texel of a level >= 1 with W > 0 is known and stores P / W, texel(); every other texel takes the colour of the texel above it in
the next coarser level, from the last level down (the push), and 0 where nothing above it is known.  / on float32 is correctly
rounded."""
import numpy as np

import mip_ref

F = np.float32


def weight(a):
    """w0 of an alpha (array or scalar): a clamped to [0, 1]; NaN, -0.0 and negatives give +0.0."""
    a = np.asarray(a, F)
    with np.errstate(all="ignore"):
        out = np.where(a > F(0.0), np.minimum(a, F(1.0)), F(0.0))
    return np.asarray(out, F)


def texel(p, w):
    """(q, known) of the boxes p (premultiplied colour) and w (weight), arrays of one shape or scalars: q = p / w where w > 0."""
    p, w = np.asarray(p, F), np.asarray(w, F)
    known = w > F(0.0)  # false for NaN
    with np.errstate(all="ignore"):
        q = np.where(known, p / np.where(known, w, F(1.0)), F(0.0))
    q = np.asarray(q, F)
    assert q.dtype == F
    return q, known


def pull(R, G, B, A):
    """-> (per channel the levels of q, level 0 the colour itself where known and 0 elsewhere; the levels of `known`)."""
    w0 = weight(A)
    k0 = w0 > F(0.0)
    W = mip_ref.chain(w0)
    known = [k0] + [lv > F(0.0) for lv in W[1:]]
    out = []
    for c in (R, G, B):
        c = np.ascontiguousarray(c, F)
        with np.errstate(all="ignore"):
            p0 = np.where(k0, c * w0, F(0.0)).astype(F)  # a select: nothing under a transparent texel enters
        P = mip_ref.chain(p0)
        out.append([np.where(k0, c, F(0.0)).astype(F)] + [texel(P[k], W[k])[0] for k in range(1, len(P))])
    return out, known


def chain(R, G, B, A):
    """All levels of the three colour planes under the rule -> three lists of levels, level 0 first.  The top-down form: an
    unknown texel (x, y) of level k stores F_{k+1}(min(x >> 1, W - 1), min(y >> 1, H - 1)); the last level's unknown texel 0."""
    q, known = pull(R, G, B, A)
    n = len(known)
    out = [[None] * n for _ in range(3)]
    for k in range(n - 1, -1, -1):
        h, w = known[k].shape
        for c in range(3):
            if k == n - 1:
                fill = np.zeros((h, w), F)
            else:
                up = out[c][k + 1]
                uh, uw = up.shape
                fill = up[np.ix_(np.minimum(np.arange(h) >> 1, uh - 1), np.minimum(np.arange(w) >> 1, uw - 1))]
            out[c][k] = np.ascontiguousarray(np.where(known[k], q[c][k], fill), F)
    return out


def chain_by_ancestors(R, G, B, A):
    """The same chain in the per-texel form: every unknown texel takes q of its nearest known ancestor
    (min(x >> (j - k), W_j - 1), min(y >> (j - k), H_j - 1)), j > k, or 0 if it has none.  No ordering between levels."""
    q, known = pull(R, G, B, A)
    n = len(known)
    out = [[None] * n for _ in range(3)]
    for k in range(n):
        h, w = known[k].shape
        ys, xs = np.arange(h), np.arange(w)
        res = [np.where(known[k], q[c][k], F(0.0)).astype(F) for c in range(3)]
        todo = ~known[k]
        for j in range(k + 1, n):
            if not todo.any():
                break
            uh, uw = known[j].shape
            ix = np.ix_(np.minimum(ys >> (j - k), uh - 1), np.minimum(xs >> (j - k), uw - 1))
            hit = todo & known[j][ix]
            for c in range(3):
                res[c] = np.where(hit, q[c][j][ix], res[c]).astype(F)
            todo &= ~hit
        for c in range(3):
            out[c][k] = np.ascontiguousarray(res[c], F)
    return out
