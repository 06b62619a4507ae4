"""Numpy reference of BC1 with punch-through alpha (KC_BC_PUNCH_THROUGH, include/kanter_core_amd.h), vectorised over blocks,
built on bc_ref.  Input: the RGBA8 bytes kc_image_to_u8 writes, uint8 (h, w, 4), and the reference byte B.  Output: uint8
(by, bx, 8).  Imports nothing from the product."""
import numpy as np

import bc_ref
from bc_ref import _pack565, expand565

EMPTY = np.array([0, 0, 0, 0, 255, 255, 255, 255], np.uint8)  # n == 0: c0 = c1 = 0, every index 3


def class_alpha(h, w, r_b, seed=0):
    """A float32 (h, w) alpha plane built by block class, for the threshold r_b of a reference byte.  Uniform random alpha
    makes practically every block mixed, so: blocks (i, j) with (i + j) % 3 == 0 get random alpha, those with == 1 values below
    the threshold (0, -0.0, a negative and the float just below r_b among them), those with == 2 values at or above it (r_b
    itself, 1, 2, inf and NaN among them)."""
    rng = np.random.default_rng([seed, h, w])
    f = np.float32
    r_b = f(r_b)
    u = rng.random((h, w), dtype=f)
    below = np.array([0.0, -0.0, -0.5, np.nextafter(r_b, f(0))], f)
    above = np.array([r_b, 1.0, 2.0, np.inf, np.nan], f)
    pick = rng.integers(0, 8, (h, w))
    lo = np.where(pick < 4, below[pick % 4], (u * np.nextafter(r_b, f(0))).astype(f)).astype(f)
    hi = np.where(pick < 5, above[pick % 5], np.maximum(r_b, r_b + u * (f(1) - r_b))).astype(f)
    cls = (np.arange(w)[None, :] // 4 + np.arange(h)[:, None] // 4) % 3
    return np.where(cls == 0, u * f(1.2) - f(0.1), np.where(cls == 1, lo, hi)).astype(f)


def class_counts(rgba8, ref):
    """-> (empty, mixed, full): the blocks of each class, edge blocks included"""
    n = opaque(bc_ref.blocks(rgba8), ref).sum(-1)
    return int((n == 0).sum()), int(((n > 0) & (n < 16)).sum()), int((n == 16).sum())


def opaque(t, ref):
    """(..., 16, 4) texels -> (..., 16) bool: the alpha byte is at least B"""
    return np.asarray(t)[..., 3] >= ref


def encode_mixed(p, op):
    """The three-colour block.  p: (..., 16, 3) ints 0..255, op: (..., 16) bool with at least one True per block -> (..., 8) uint8"""
    p = np.asarray(p, np.int64)
    o3 = op[..., None]
    lo = np.where(o3, p, 255).min(-2)
    hi = np.where(o3, p, 0).max(-2)
    k = np.argmax(hi - lo, -1)  # the first channel of the largest range
    ck = np.take_along_axis(p, k[..., None, None], -1)[..., 0]
    lok = np.take_along_axis(lo, k[..., None], -1)
    hik = np.take_along_axis(hi, k[..., None], -1)
    s = (np.where(op, 2 * ck - lok - hik, 0)[..., None] * (2 * p - lo[..., None, :] - hi[..., None, :])).sum(-2)
    m = (hi - lo) >> 3
    a, b = hi - m, lo + m
    neg = s < 0
    a, b = np.where(neg, b, a), np.where(neg, a, b)
    c0, c1 = _pack565(a), _pack565(b)
    c0, c1 = np.minimum(c0, c1), np.maximum(c0, c1)
    e0, e1 = expand565(c0), expand565(c1)
    pal = np.stack([e0, e1, (e0 + e1) // 2], -2)  # (..., 3, 3)
    err = ((p[..., :, None, :] - pal[..., None, :, :]) ** 2).sum(-1)  # (..., 16, 3)
    idx = np.where(op, np.argmin(err, -1), 3)  # the lowest j on a tie
    word = (idx.astype(np.uint64) << (2 * np.arange(16, dtype=np.uint64))).sum(-1, dtype=np.uint64)
    out = np.empty(p.shape[:-2] + (8,), np.uint8)
    out[..., 0] = c0 & 0xff
    out[..., 1] = c0 >> 8
    out[..., 2] = c1 & 0xff
    out[..., 3] = c1 >> 8
    for i in range(4):
        out[..., 4 + i] = (word >> np.uint64(8 * i)) & np.uint64(0xff)
    return out


def encode_blocks(t, ref):
    """t: (..., 16, 4) texels -> (..., 8) uint8"""
    t = np.asarray(t, np.int64)
    op = opaque(t, ref)
    n = op.sum(-1)
    some = np.where((n == 0)[..., None], True, op)  # an empty block takes the fixed bytes below: any mask will do here
    out = encode_mixed(t[..., :3], some)
    out = np.where((n == 16)[..., None], bc_ref.encode_bc1(t[..., :3]), out)
    return np.where((n == 0)[..., None], EMPTY, out).astype(np.uint8)


def encode(rgba8, ref):
    """rgba8: uint8 (h, w, 4) as kc_image_to_u8 writes it -> uint8 (by, bx, 8)"""
    assert 1 <= ref <= 255
    return encode_blocks(bc_ref.blocks(rgba8), ref)


def decode(blk, h, w):
    """(by, bx, 8) blocks -> (h, w, 4) ints: BC1 as a decoder reads it, index 3 of a three-colour block transparent black"""
    b = np.asarray(blk, np.uint8).astype(np.int64)
    c0 = b[..., 0] | (b[..., 1] << 8)
    c1 = b[..., 2] | (b[..., 3] << 8)
    word = b[..., 4] | (b[..., 5] << 8) | (b[..., 6] << 16) | (b[..., 7] << 24)
    idx = (word[..., None] >> (2 * np.arange(16))) & 3
    clear = (c0 <= c1)[..., None] & (idx == 3)
    rgb = bc_ref.decode_bc1(blk)
    t = np.concatenate([rgb, np.where(clear, 0, 255)[..., None]], -1)
    return bc_ref.unblock(t, h, w)


def error_sums(rgba8, blk, ref):
    """-> (sse[4], max_abs[4]) as kc_bc_error reports them under the flag: alpha against 255 where the source is opaque and 0
    elsewhere; a pixel whose source texel is not opaque contributes nothing to R, G, B"""
    a = np.asarray(rgba8).astype(np.int64)
    h, w = a.shape[:2]
    dec = decode(blk, h, w)
    op = a[..., 3] >= ref
    src = np.concatenate([a[..., :3], np.where(op, 255, 0)[..., None]], -1)
    d = np.abs(dec - src)
    d[..., :3] *= op[..., None]
    return (d * d).reshape(-1, 4).sum(0), d.reshape(-1, 4).max(0)
