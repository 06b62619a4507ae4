"""Numpy reference of the BC6H contract (include/kanter_core_amd.h, KC_BC6H = 95, DXGI_FORMAT_BC6H_UF16): the source
quantisation to half bit patterns, the mode-11 encoder, the decoder of the four single-subset modes 11-14 (the two-subset
modes 1-10 are not decoded, the reserved mode values decode to zero), and the error record over half bit patterns.  Planes are
f32 (h, w), texels integers 0..31743 (the bit patterns of the finite non-negative halves), blocks uint8 (by, bx, 16).
Imports nothing from the product.

The rounding term of interp: the format defines interp(a, b, w) = ((64 - w) a + w b + 32) >> 6 and the contract keeps the
+ 32.  Pillow 12's BC6H decoder leaves it out, so decode(..., round_term=0) is the form that equals Pillow's bytes exactly; with
the contract's round_term=32 about 0.14 % of Pillow's bytes are one off."""
import numpy as np

from bc_ref import blocks, unblock  # noqa: F401  (unblock: for the callers)

BC6H = 95
HALF_MAX = 0x7BFF  # 65504
W4 = np.array([0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64], np.int64)
CHUNK = 2048
# mode -> (the 5-bit (2-bit: modes 1, 2) mode field, bits of endpoint 0, bits of the delta; 0: endpoint 1 is stored whole)
FIELD = {1: 0, 2: 1, 3: 2, 4: 6, 5: 10, 6: 14, 7: 18, 8: 22, 9: 26, 10: 30, 11: 3, 12: 7, 13: 11, 14: 15}
RESERVED = (19, 23, 27, 31)
SINGLE = {11: (10, 0), 12: (11, 9), 13: (12, 8), 14: (16, 4)}


def quant_half(v):
    """f32 -> the bit pattern of f16_rne(min(max(v, 0), 65504)), int64: NaN, negatives, -0 and -inf give 0, +inf and everything
    >= 65504 give 0x7BFF; denormal halves are kept"""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        x = np.where(v > 0, v, np.float32(0))  # NaN and -0 fail the comparison
    x = np.minimum(x, np.float32(65504.0))
    return x.astype(np.float16).view(np.uint16).astype(np.int64)


def half_value(bits):
    """half bit patterns -> their exact f32 values"""
    return np.asarray(bits).astype(np.uint16).view(np.float16).astype(np.float32)


def texels(planes):
    """1 (Gray: (v, v, v)) or >= 3 f32 planes (h, w) -> (h, w, 3) half bit patterns; alpha is never read"""
    planes = [np.asarray(p, np.float32) for p in planes]
    if len(planes) == 1:
        planes = planes * 3
    return np.stack([quant_half(p) for p in planes[:3]], -1)


def interp(a, b, w, round_term=32):
    return ((64 - w) * a + w * b + round_term) >> 6


def fin(x):
    return (31 * x) >> 6


def unq(x, n):
    """the n-bit endpoint x -> 16 bits"""
    x = np.asarray(x, np.int64)
    if n == 16:
        return x
    return np.where(x == 0, 0, np.where(x == (1 << n) - 1, 0xFFFF, ((x << 16) + 0x8000) >> n))


E10 = fin(unq(np.arange(1024), 10))  # what a 10-bit endpoint decodes to at weight 0: 0, 46, 77, ..., 31697, 31743


_Q10 = []


def q10(e):
    """the smallest q in 0..1023 minimising |E10[q] - e|: the exhaustive arg-min, tabulated once for every e in 0..31743"""
    if not _Q10:
        every = np.arange(HALF_MAX + 1).reshape(-1, 1024, 1)
        _Q10.append(np.concatenate([np.argmin(np.abs(E10[None, :] - part), -1) for part in every]))
    return _Q10[0][np.asarray(e, np.int64)]


def axis(p):
    """p: (n, 16, 3) -> e0, e1 (n, 3): BC7's covariance-sign diagonal of the box.  |s| reaches 2^34: int64"""
    lo, hi = p.min(1), p.max(1)
    k = np.argmax(hi - lo, -1)  # the first channel of the largest range
    c = 2 * p - lo[:, None, :] - hi[:, None, :]
    a = np.take_along_axis(c, k[:, None, None], -1)
    neg = (a * c).sum(1) < 0
    return np.where(neg, hi, lo), np.where(neg, lo, hi)


def palette(q0, q1, round_term=32):
    """10-bit endpoints (n, 3) -> (n, 16, 3) half bit patterns"""
    u0, u1 = unq(q0, 10), unq(q1, 10)
    return fin(interp(u0[:, None, :], u1[:, None, :], W4[None, :, None], round_term))


def _put(bits, at, value, n):
    value = np.asarray(value, np.int64)
    if value.ndim == 1:
        value = value[:, None]
    for j in range(value.shape[1]):
        for b in range(n):
            bits[:, at + j * n + b] = (value[:, j] >> b) & 1
    return at + value.shape[1] * n


def _pack(bits):
    return (bits.reshape(len(bits), 16, 8) << np.arange(8)).sum(-1).astype(np.uint8)


def _bits(blk):
    blk = np.asarray(blk, np.uint8).reshape(-1, 16)
    return ((blk[:, :, None] >> np.arange(8)) & 1).reshape(len(blk), 128).astype(np.int64)


def _get(bits, at, n, count=1):
    return (bits[:, at:at + n * count].reshape(len(bits), count, n) << np.arange(n)).sum(-1)


def encode_blocks_detail(p):
    """p: (n, 16, 3) half bit patterns -> dict(blocks (n, 16) uint8, q0, q1 (n, 3) as stored, idx (n, 16) as stored, swap (n,))"""
    p = np.asarray(p, np.int64)
    n = len(p)
    e0, e1 = axis(p)
    q0, q1 = q10(e0), q10(e1)
    pal = palette(q0, q1)
    d = ((p[:, :, None, :] - pal[:, None, :, :]) ** 2).sum(-1)  # (n, 16 texels, 16 entries), below 3 * 31743^2
    idx = np.argmin(d, -1)  # the lowest index on a tie
    sw = idx[:, 0] >= 8
    idx = np.where(sw[:, None], 15 - idx, idx)
    q0, q1 = np.where(sw[:, None], q1, q0), np.where(sw[:, None], q0, q1)
    b = np.zeros((n, 128), np.int64)
    at = _put(b, 0, np.full(n, 3), 5)
    at = _put(b, at, q0, 10)  # R0 G0 B0
    at = _put(b, at, q1, 10)  # R1 G1 B1
    at = _put(b, at, idx[:, 0], 3)
    at = _put(b, at, idx[:, 1:], 4)
    assert at == 128
    return dict(blocks=_pack(b), q0=q0, q1=q1, idx=idx, swap=sw)


def encode_detail(p):
    p = np.asarray(p).reshape(-1, 16, 3)
    parts = [encode_blocks_detail(p[i:i + CHUNK]) for i in range(0, len(p), CHUNK)]
    return {k: np.concatenate([x[k] for x in parts]) for k in parts[0]}


def encode_texels(t):
    """(h, w, 3) half bit patterns -> uint8 (by, bx, 16)"""
    g = blocks(t)
    return encode_detail(g)["blocks"].reshape(g.shape[:2] + (16,))


def encode(planes):
    """1 or >= 3 f32 planes (h, w) -> uint8 (by, bx, 16): mode 11 blocks"""
    return encode_texels(texels(planes))


def modes(blk):
    """(n, 16) uint8 -> mode 1..14 of each block, 0 for the four reserved values of the mode field"""
    b0 = np.asarray(blk, np.uint8).reshape(-1, 16)[:, 0].astype(np.int64)
    out = np.zeros(len(b0), np.int64)
    two = (b0 & 2) == 0
    out[two] = (b0[two] & 1) + 1
    for m, f in FIELD.items():
        if m > 2:
            out[~two & ((b0 & 31) == f)] = m
    return out


def undecoded(mode):
    return (mode >= 1) & (mode <= 10)


def decode_blocks(blk, round_term=32):
    """(..., 16) uint8 -> texels (..., 16, 3) half bit patterns (all <= 0x7BFF), modes (...,).  Two-subset and reserved blocks
    give (0, 0, 0)."""
    blk = np.asarray(blk, np.uint8)
    lead = blk.shape[:-1]
    bits = _bits(blk)
    n = len(bits)
    mode = modes(blk)
    low = _get(bits, 5, 10, 3)                       # the low 10 bits of R0, G0, B0
    grp = _get(bits, 35, 10, 3)                      # per channel: endpoint 1 (mode 11), or delta and the high bits of endpoint 0
    gb = (grp[:, :, None] >> np.arange(10)) & 1      # (n, 3, 10)
    idx = np.concatenate([_get(bits, 65, 3), _get(bits, 68, 4, 15)], -1)
    out = np.zeros((n, 16, 3), np.int64)
    for m, (nb, db) in SINGLE.items():
        if db == 0:
            e0, e1 = low, grp
        else:
            # bit 9 of the group is e0[10], bit 8 e0[11], ... down to the first bit after the delta
            high = sum(gb[:, :, 9 - j] << (10 + j) for j in range(nb - 10))
            e0 = low | high
            delta = grp & ((1 << db) - 1)
            delta = delta - ((delta >> (db - 1)) << db)  # sign extension
            e1 = (e0 + delta) & ((1 << nb) - 1)
        u0, u1 = unq(e0, nb), unq(e1, nb)
        t = fin(interp(u0[:, None, :], u1[:, None, :], W4[idx][:, :, None], round_term))
        out[mode == m] = t[mode == m]
    return out.reshape(lead + (16, 3)), mode.reshape(lead)


def decode(blk, h, w, round_term=32):
    """(by, bx, 16) uint8 -> half bit patterns (h, w, 3), the modes (by, bx), the count of undecoded (two-subset) blocks"""
    t, mode = decode_blocks(blk, round_term)
    return unblock(t, h, w), mode, int(undecoded(mode).sum())


def decode_planes(blk, h, w):
    """the f32 planes kc_image_from_bc makes: R, G, B the halves' exact values, A = 1"""
    px = decode(blk, h, w)[0]
    return [half_value(px[..., c]) for c in range(3)] + [np.ones((h, w), np.float32)]


def pillow_bytes(px):
    """half bit patterns -> the bytes Pillow shows for them: floor(255 clamp(v, 0, 1)) in f32"""
    v = half_value(px)
    return np.floor(np.float32(255.0) * np.clip(v, np.float32(0), np.float32(1))).astype(np.uint8)


def compare(planes, blk):
    """kc_bc_error of the blocks against the image's planes, as a dict: integer differences of half bit patterns"""
    src = texels(planes)
    h, w = src.shape[:2]
    px, mode, n = decode(blk, h, w)
    d = np.abs(px - src)
    return dict(format=BC6H, channel_mask=0x7, pixels=h * w, sse=[int(v) for v in (d ** 2).sum((0, 1))] + [0],
                max_abs=[int(v) for v in d.max((0, 1))] + [0], undecoded_blocks=n, bc7_mode_blocks=[0] * 8)


def psnr(rec, channels=None):
    chans = [c for c in range(4) if (rec["channel_mask"] >> c) & 1 and (channels is None or c in channels)]
    sse = sum(rec["sse"][c] for c in chans)
    return float("inf") if sse == 0 else 10 * np.log10(31743.0 ** 2 * rec["pixels"] * len(chans) / sse)


# ------------------------------------------------------------------ random blocks that reach every branch
CYCLE = np.array([11, 12, 13, 14] * 4 + list(range(1, 11)) + [-19, -23, -27, -31])  # negative: a reserved field value


def force_mode(blk, mode):
    """(n, 16) uint8 random bytes -> the same with the mode field of `mode` (1..14; -f: the reserved field value f)"""
    blk = np.array(blk, np.uint8).reshape(-1, 16)
    mode = np.broadcast_to(np.asarray(mode, np.int64), (len(blk),))
    field = np.array([-m if m < 0 else FIELD[m] for m in mode], np.int64)
    keep = np.where((mode == 1) | (mode == 2), 0xfc, 0xe0)
    blk[:, 0] = (blk[:, 0] & keep) | field
    return blk


def clear_top_bit_of_endpoint0(blk):
    """mode 11-14 blocks with the top bit of every channel's endpoint 0 cleared: endpoint 0 decodes below 1.0"""
    blk = np.array(blk, np.uint8).reshape(-1, 16)
    top = {11: 14, 12: 44, 13: 43, 14: 39}  # R's bit; G's and B's are 10 and 20 further on
    m = modes(blk)
    for mode, at in top.items():
        for c in range(3):
            bit = at + 10 * c
            blk[m == mode, bit >> 3] &= 0xff ^ (1 << (bit & 7))
    return blk


def random_blocks(n, seed=0, only=None, low=False):
    """n random blocks, (n, 16) uint8.  Modes 11-14 take turns four times, then one block of each two-subset mode 1-10 and of
    each reserved field value: a cycle of 30.  only: a mode that every block takes instead.  low: endpoint 0 below half of its
    range, so that most texels decode inside [0, 1]."""
    rng = np.random.default_rng(seed + 1000 * BC6H)
    blk = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    blk = force_mode(blk, CYCLE[np.arange(n) % len(CYCLE)] if only is None else only)
    return clear_top_bit_of_endpoint0(blk) if low else blk


def random_image_blocks(h, w, seed=0):
    by, bx = (h + 3) // 4, (w + 3) // 4
    return random_blocks(by * bx, seed + 7 * h + w).reshape(by, bx, 16)
