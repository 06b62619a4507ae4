"""Numpy reference of the BC1 / BC3 / BC4 / BC5 encoder contract (include/kanter_core_amd.h, kc_image_to_bc), vectorised over
blocks, and a decoder for the quality checks.  Input: the RGBA8 bytes kc_image_to_u8 writes, uint8 (h, w, 4).  Output: uint8
(by, bx, block_bytes), block rows tightly packed.  Imports nothing from the product."""
import numpy as np

BLOCK_BYTES = {1: 8, 3: 16, 4: 8, 5: 16}


def blocks(rgba8):
    """(h, w, C) -> (by, bx, 16, C) int64: texel t = 4y + x of block (i, j) is pixel (min(4i+x, w-1), min(4j+y, h-1))."""
    a = np.asarray(rgba8)
    h, w = a.shape[:2]
    by, bx = (h + 3) // 4, (w + 3) // 4
    ys = np.minimum(np.arange(4 * by), h - 1)
    xs = np.minimum(np.arange(4 * bx), w - 1)
    g = a[ys][:, xs].astype(np.int64)  # (4by, 4bx, C)
    g = g.reshape(by, 4, bx, 4, -1).transpose(0, 2, 1, 3, 4)  # (by, bx, y, x, C)
    return g.reshape(by, bx, 16, -1)


def encode_bc4(v):
    """v: (..., 16) ints 0..255 -> (..., 8) uint8"""
    v = np.asarray(v, np.int64)
    e0 = v.max(-1)
    e1 = v.min(-1)
    d = e0 - e1
    dd = np.where(d == 0, 1, d)[..., None]
    r = (14 * (v - e1[..., None]) + dd) // (2 * dd)
    idx = np.where(r == 7, 0, np.where(r == 0, 1, 8 - r))
    idx = np.where((d == 0)[..., None], 0, idx)
    word = (idx.astype(np.uint64) << (3 * np.arange(16, dtype=np.uint64))).sum(-1, dtype=np.uint64)
    out = np.empty(v.shape[:-1] + (8,), np.uint8)
    out[..., 0] = e0
    out[..., 1] = e1
    for k in range(6):
        out[..., 2 + k] = (word >> np.uint64(8 * k)) & np.uint64(0xff)
    return out


def _pack565(c):
    q5 = lambda x: (31 * x + 127) // 255
    q6 = lambda x: (63 * x + 127) // 255
    return (q5(c[..., 0]) << 11) | (q6(c[..., 1]) << 5) | q5(c[..., 2])


def expand565(c):
    """(...,) 565 words -> (..., 3) 8-bit colours by bit replication"""
    c = np.asarray(c, np.int64)
    r5, g6, b5 = c >> 11, (c >> 5) & 63, c & 31
    return np.stack([(r5 << 3) | (r5 >> 2), (g6 << 2) | (g6 >> 4), (b5 << 3) | (b5 >> 2)], -1)


def encode_bc1(p, swap=True):
    """p: (..., 16, 3) ints 0..255 -> (..., 8) uint8.  swap=False drops step 4's anti-diagonal swap (the worked-example
    foil only)."""
    p = np.asarray(p, np.int64)
    lo = p.min(-2)
    hi = p.max(-2)
    k = np.argmax(hi - lo, -1)  # the first channel of the largest range
    ck = np.take_along_axis(p, k[..., None, None], -1)[..., 0]  # (..., 16)
    lok = np.take_along_axis(lo, k[..., None], -1)
    hik = np.take_along_axis(hi, k[..., None], -1)
    s = ((2 * ck - lok - hik)[..., None] * (2 * p - lo[..., None, :] - hi[..., None, :])).sum(-2)  # (..., 3)
    m = (hi - lo) >> 4
    a = hi - m
    b = lo + m
    if swap:
        neg = s < 0
        a, b = np.where(neg, b, a), np.where(neg, a, b)
    c0 = _pack565(a)
    c1 = _pack565(b)
    c0, c1 = np.maximum(c0, c1), np.minimum(c0, c1)
    e0, e1 = expand565(c0), expand565(c1)
    pal = np.stack([3 * e0, 3 * e1, 2 * e0 + e1, e0 + 2 * e1], -2)  # (..., 4, 3)
    err = ((3 * p[..., :, None, :] - pal[..., None, :, :]) ** 2).sum(-1)  # (..., 16, 4)
    idx = np.argmin(err, -1)  # the lowest j on a tie
    idx = np.where((c0 == c1)[..., None], 0, idx)
    word = (idx.astype(np.uint64) << (2 * np.arange(16, dtype=np.uint64))).sum(-1, dtype=np.uint64)
    out = np.empty(p.shape[:-2] + (8,), np.uint8)
    out[..., 0] = c0 & 0xff
    out[..., 1] = c0 >> 8
    out[..., 2] = c1 & 0xff
    out[..., 3] = c1 >> 8
    for k in range(4):
        out[..., 4 + k] = (word >> np.uint64(8 * k)) & np.uint64(0xff)
    return out


def encode(rgba8, fmt):
    """rgba8: uint8 (h, w, 4) as kc_image_to_u8 writes it -> uint8 (by, bx, BLOCK_BYTES[fmt])"""
    t = blocks(rgba8)
    if fmt == 1:
        return encode_bc1(t[..., :3])
    if fmt == 3:
        return np.concatenate([encode_bc4(t[..., 3]), encode_bc1(t[..., :3])], -1)
    if fmt == 4:
        return encode_bc4(t[..., 0])
    if fmt == 5:
        return np.concatenate([encode_bc4(t[..., 0]), encode_bc4(t[..., 1])], -1)
    raise ValueError("unknown BC format %r" % (fmt,))


def _indices(words, bits):
    return (words[..., None] >> (bits * np.arange(16, dtype=np.uint64))) & np.uint64((1 << bits) - 1)


def decode_bc4(blk):
    """(..., 8) uint8 -> (..., 16) ints"""
    blk = np.asarray(blk, np.uint8)
    e0 = blk[..., 0].astype(np.int64)
    e1 = blk[..., 1].astype(np.int64)
    word = np.zeros(blk.shape[:-1], np.uint64)
    for k in range(6):
        word |= blk[..., 2 + k].astype(np.uint64) << np.uint64(8 * k)
    idx = _indices(word, 3).astype(np.int64)
    i = np.arange(8)
    e0b, e1b = e0[..., None], e1[..., None]
    eight = np.where(i >= 2, ((8 - i) * e0b + (i - 1) * e1b + 3) // 7, 0)
    six = np.where((i >= 2) & (i <= 5), ((6 - i) * e0b + (i - 1) * e1b + 2) // 5, np.where(i == 6, 0, 255))
    pal = np.where((e0 > e1)[..., None], eight, six)
    pal[..., 0], pal[..., 1] = e0, e1
    return np.take_along_axis(pal, idx, -1)


def decode_bc1(blk):
    """(..., 8) uint8 -> (..., 16, 3) ints (four-colour mode when c0 > c1, else three colours and black)"""
    blk = np.asarray(blk, np.uint8).astype(np.int64)
    c0 = blk[..., 0] | (blk[..., 1] << 8)
    c1 = blk[..., 2] | (blk[..., 3] << 8)
    word = np.zeros(blk.shape[:-1], np.uint64)
    for k in range(4):
        word |= blk[..., 4 + k].astype(np.uint64) << np.uint64(8 * k)
    idx = _indices(word, 2).astype(np.int64)
    a, b = expand565(c0), expand565(c1)
    four = (c0 > c1)[..., None]
    p2 = np.where(four, (2 * a + b + 1) // 3, (a + b) // 2)
    p3 = np.where(four, (a + 2 * b + 1) // 3, 0)
    pal = np.stack([a, b, p2, p3], -2)  # (..., 4, 3)
    return np.take_along_axis(pal, idx[..., None], -2)


def unblock(t, h, w):
    """(by, bx, 16, C) texels -> (h, w, C)"""
    by, bx = t.shape[:2]
    g = t.reshape(by, bx, 4, 4, -1).transpose(0, 2, 1, 3, 4).reshape(4 * by, 4 * bx, -1)
    return g[:h, :w]


def psnr_bc1(rgba8):
    """PSNR (dB) of BC1 over R, G and B of every pixel"""
    a = np.asarray(rgba8)
    h, w = a.shape[:2]
    dec = unblock(decode_bc1(encode(a, 1)), h, w)
    mse = ((dec - a[..., :3].astype(np.int64)) ** 2).mean()
    return 10 * np.log10(255.0 ** 2 / mse)
