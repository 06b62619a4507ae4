"""Numpy reference of the BC7 encoder contract (include/kanter_core_amd.h, kc_image_to_bc with KC_BC7): the single-subset modes
6 and 5 (rotation 0), vectorised over blocks and worked in chunks, and a decoder of those two modes.  Input: the RGBA8 bytes
kc_image_to_u8 writes, uint8 (h, w, 4).  Output: uint8 (by, bx, 16), block rows tightly packed.  Imports nothing from the
product."""
import numpy as np

from bc_ref import blocks, unblock  # noqa: F401  (unblock: for the callers)

BC7 = 98
W4 = np.array([0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64], np.int64)
W2 = np.array([0, 21, 43, 64], np.int64)
CHUNK = 4096


def interp(e0, e1, w):
    return ((64 - w) * e0 + w * e1 + 32) >> 6


def axis(p):
    """p: (n, 16, C) -> e0, e1 (n, C): the box diagonal the covariance signs against the widest channel choose, no inset"""
    lo, hi = p.min(1), p.max(1)
    k = np.argmax(hi - lo, -1)  # the first channel of the largest range
    c = 2 * p - lo[:, None, :] - hi[:, None, :]
    a = np.take_along_axis(c, k[:, None, None], -1)  # (n, 16, 1)
    s = (a * c).sum(1)
    neg = s < 0
    return np.where(neg, hi, lo), np.where(neg, lo, hi)


def search(p, v0, v1, w):
    """p: (n, 16, C), endpoints (n, C), weights (m,) -> indices (n, 16), their squared distances (n, 16)"""
    pal = interp(v0[:, None, :], v1[:, None, :], w[None, :, None])  # (n, m, C)
    d = ((p[:, :, None, :] - pal[:, None, :, :]) ** 2).sum(-1)  # (n, 16, m)
    idx = np.argmin(d, -1)  # the lowest index on a tie
    return idx, np.take_along_axis(d, idx[..., None], -1)[..., 0]


def quant6(e):
    """(n, 4) endpoint -> q (n, 4) 7-bit, pb (n,): the p-bit is shared by the endpoint's four channels"""
    best = None
    for pb in (0, 1):
        q = np.clip((e - pb + 1) >> 1, 0, 127)
        cost = ((2 * q + pb - e) ** 2).sum(-1)
        if best is None:
            best = (q, np.zeros(len(e), np.int64), cost)
        else:
            take = cost < best[2]  # pb = 1 only if strictly better
            best = (np.where(take[:, None], q, best[0]), np.where(take, 1, best[1]), np.minimum(cost, best[2]))
    return best[0], best[1]


def quant5(e):
    q = (127 * e + 127) // 255
    return q, (q << 1) | (q >> 6)


def _put(bits, at, value, n):
    """value (n_blocks,) or (n_blocks, k) LSB first into bits[:, at:]"""
    value = np.asarray(value, np.int64)
    if value.ndim == 1:
        value = value[:, None]
    for j in range(value.shape[1]):
        for b in range(n):
            bits[:, at + j * n + b] = (value[:, j] >> b) & 1
    return at + value.shape[1] * n


def _pack(bits):
    return (bits.reshape(len(bits), 16, 8) << np.arange(8)).sum(-1).astype(np.uint8)


def encode_blocks_detail(p):
    """p: (n, 16, 4) ints 0..255 -> dict(blocks (n, 16) uint8, mode (n,), err (n,) of the chosen mode, err5, err6, and whether
    the anchor swapped mode 6's endpoints (swap6), mode 5's colour set (swap5c) and its alpha set (swap5a))"""
    p = np.asarray(p, np.int64)
    n = len(p)
    # mode 6
    e0, e1 = axis(p)
    q0, p0 = quant6(e0)
    q1, p1 = quant6(e1)
    i6, d6 = search(p, 2 * q0 + p0[:, None], 2 * q1 + p1[:, None], W4)
    err6 = d6.sum(-1)
    sw = i6[:, 0] >= 8
    i6 = np.where(sw[:, None], 15 - i6, i6)
    q0, q1 = np.where(sw[:, None], q1, q0), np.where(sw[:, None], q0, q1)
    p0, p1 = np.where(sw, p1, p0), np.where(sw, p0, p1)
    b6 = np.zeros((n, 128), np.int64)
    at = _put(b6, 0, np.full(n, 64), 7)
    at = _put(b6, at, np.stack([q0, q1], -1).reshape(n, 8), 7)  # R0 R1 G0 G1 B0 B1 A0 A1
    at = _put(b6, at, p0, 1)
    at = _put(b6, at, p1, 1)
    at = _put(b6, at, i6[:, 0], 3)
    at = _put(b6, at, i6[:, 1:], 4)
    assert at == 128
    # mode 5
    c0, c1 = axis(p[..., :3])
    r0, v0 = quant5(c0)
    r1, v1 = quant5(c1)
    ic, dc = search(p[..., :3], v0, v1, W2)
    a0, a1 = p[..., 3].min(-1), p[..., 3].max(-1)
    ia, da = search(p[..., 3:], a0[:, None], a1[:, None], W2)
    err5 = dc.sum(-1) + da.sum(-1)
    sc = ic[:, 0] >= 2
    ic = np.where(sc[:, None], 3 - ic, ic)
    r0, r1 = np.where(sc[:, None], r1, r0), np.where(sc[:, None], r0, r1)
    sa = ia[:, 0] >= 2
    ia = np.where(sa[:, None], 3 - ia, ia)
    a0, a1 = np.where(sa, a1, a0), np.where(sa, a0, a1)
    b5 = np.zeros((n, 128), np.int64)
    at = _put(b5, 0, np.full(n, 32), 6)
    at = _put(b5, at, np.zeros(n), 2)
    at = _put(b5, at, np.stack([r0, r1], -1).reshape(n, 6), 7)
    at = _put(b5, at, np.stack([a0, a1], -1), 8)
    at = _put(b5, at, ic[:, 0], 1)
    at = _put(b5, at, ic[:, 1:], 2)
    at = _put(b5, at, ia[:, 0], 1)
    at = _put(b5, at, ia[:, 1:], 2)
    assert at == 128
    m5 = err5 < err6
    return dict(blocks=_pack(np.where(m5[:, None], b5, b6)), mode=np.where(m5, 5, 6), err=np.where(m5, err5, err6), err5=err5,
                err6=err6, swap6=sw, swap5c=sc, swap5a=sa)


def encode_detail(p):
    """encode_blocks_detail in chunks: the exhaustive search over a whole image at once does not fit memory"""
    p = np.asarray(p).reshape(-1, 16, 4)
    parts = [encode_blocks_detail(p[i:i + CHUNK]) for i in range(0, len(p), CHUNK)]
    return {k: np.concatenate([x[k] for x in parts]) for k in parts[0]}


def encode_blocks(p):
    """p: (..., 16, 4) -> (..., 16) uint8"""
    p = np.asarray(p)
    return encode_detail(p)["blocks"].reshape(p.shape[:-2] + (16,))


def encode(rgba8, fmt=BC7):
    """rgba8: uint8 (h, w, 4) as kc_image_to_u8 writes it -> uint8 (by, bx, 16)"""
    if fmt != BC7:
        raise ValueError("unknown BC format %r" % (fmt,))
    return encode_blocks(blocks(rgba8))


def _bits(blk):
    blk = np.asarray(blk, np.uint8).reshape(-1, 16)
    return ((blk[:, :, None] >> np.arange(8)) & 1).reshape(len(blk), 128).astype(np.int64)


def _get(bits, at, n, count=1):
    v = (bits[:, at:at + n * count].reshape(len(bits), count, n) << np.arange(n)).sum(-1)
    return v, at + n * count


def fields(blk):
    """(n, 16) uint8 -> dict of the raw fields: mode (5, 6 or -1), rot, ep (n, 2, 4) decoded endpoints, p (n, 2), idx, idx_a"""
    b = _bits(blk)
    n = len(b)
    is6 = (_get(b, 0, 7)[0][:, 0] == 64)
    is5 = (_get(b, 0, 6)[0][:, 0] == 32)
    # mode 6
    q, at = _get(b, 7, 7, 8)
    pp, at = _get(b, at, 1, 2)
    i0, at = _get(b, at, 3)
    ir, at = _get(b, at, 4, 15)
    ep6 = 2 * q.reshape(n, 4, 2).transpose(0, 2, 1) + pp[:, :, None]
    idx6 = np.concatenate([i0, ir], -1)
    # mode 5
    rot, at = _get(b, 6, 2)
    q, at = _get(b, at, 7, 6)
    al, at = _get(b, at, 8, 2)
    c0, at = _get(b, at, 1)
    cr, at = _get(b, at, 2, 15)
    a0, at = _get(b, at, 1)
    ar, at = _get(b, at, 2, 15)
    q = q.reshape(n, 3, 2).transpose(0, 2, 1)
    ep5 = np.concatenate([(q << 1) | (q >> 6), al[:, :, None]], -1)
    s = is6[:, None, None]
    return dict(mode=np.where(is6, 6, np.where(is5, 5, -1)), rot=np.where(is6, 0, rot[:, 0]), ep=np.where(s, ep6, ep5),
                p=np.where(is6[:, None], pp, 0), idx=np.where(is6[:, None], idx6, np.concatenate([c0, cr], -1)),
                idx_a=np.where(is6[:, None], idx6, np.concatenate([a0, ar], -1)))


def decode_blocks(blk):
    """(..., 16) uint8 of modes 5 (rotation 0) and 6 -> (..., 16, 4) ints"""
    blk = np.asarray(blk, np.uint8)
    f = fields(blk)
    assert ((f["mode"] > 0) & (f["rot"] == 0)).all(), "only modes 5 (rotation 0) and 6 are decoded"
    is6 = f["mode"] == 6
    wc = np.where(is6[:, None], W4[f["idx"]], W2[f["idx"] & 3])
    wa = np.where(is6[:, None], W4[f["idx_a"]], W2[f["idx_a"] & 3])
    w = np.concatenate([np.repeat(wc[..., None], 3, -1), wa[..., None]], -1)  # (n, 16, 4)
    out = interp(f["ep"][:, 0, None, :], f["ep"][:, 1, None, :], w)
    return out.reshape(blk.shape[:-1] + (16, 4))


def decode(blk, h, w):
    """(by, bx, 16) uint8 -> (h, w, 4) ints"""
    return unblock(decode_blocks(blk), h, w)


def psnr_rgb(rgba8):
    """PSNR (dB) of BC7 over R, G and B of every pixel"""
    a = np.asarray(rgba8)
    h, w = a.shape[:2]
    mse = ((decode(encode(a), h, w)[..., :3] - a[..., :3].astype(np.int64)) ** 2).mean()
    return 10 * np.log10(255.0 ** 2 / mse)
