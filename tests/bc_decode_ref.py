"""Numpy reference of the block decode contract (include/kanter_core_amd.h, kc_image_from_bc): BC1, BC3, BC4, BC5 and the
single-subset BC7 modes 4, 5 and 6 with every rotation and both index selections, the reserved block and the partitioned modes
that are not decoded; the error record of kc_image_bc_compare; and kc_dds_parse.  Blocks are uint8 (by, bx, block bytes),
pixels uint8 (h, w, 4).  Imports nothing from the product."""
import struct

import numpy as np

import bc_ref
import bc7_ref
from bc7_ref import W2, W4, interp

BC7 = 98
FORMATS = (1, 3, 4, 5, BC7)
BLOCK_BYTES = {1: 8, 3: 16, 4: 8, 5: 16, BC7: 16}
CHANNEL_MASK = {1: 0x7, 3: 0xF, 4: 0x1, 5: 0x3, BC7: 0xF}
W3 = np.array([0, 9, 18, 27, 37, 46, 55, 64], np.int64)
BC_SRGB, BC_GRAY = 1, 4
KC_OK, KC_ERR_IO, KC_ERR_NO_DEVICE, KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 0, 18, 101, 102, 104
DXGI = {(1, 0): 71, (1, 1): 72, (3, 0): 77, (3, 1): 78, (4, 0): 80, (5, 0): 83, (BC7, 0): 98, (BC7, 1): 99}


def as_rgba8(a):
    """a decoded PNG (h, w, 1..4) uint8 -> the RGBA8 bytes to_u8 of its image writes: Gray is (v, v, v, 255), opaque without alpha"""
    a = np.asarray(a)
    if a.shape[2] < 3:
        a = np.concatenate([np.repeat(a[..., :1], 3, -1), a[..., 1:]], -1)
    if a.shape[2] == 3:
        a = np.concatenate([a, np.full(a.shape[:2] + (1,), 255, a.dtype)], -1)
    return a


def _get(bits, at, n, count=1):
    """count fields of n bits from bit `at`, LSB first -> (blocks, count)"""
    return (bits[:, at:at + n * count].reshape(len(bits), count, n) << np.arange(n)).sum(-1)


def _anchored(bits, at, n):
    """an index set of n-bit indices whose texel 0 has n - 1 bits -> (blocks, 16)"""
    return np.concatenate([_get(bits, at, n - 1), _get(bits, at + n - 1, n, 15)], -1)


def bc7_modes(blk):
    """(n, 16) uint8 -> the mode of each block: the lowest set bit of byte 0, 8 for the reserved block"""
    b0 = np.asarray(blk, np.uint8).reshape(-1, 16)[:, 0].astype(np.int64)
    low = b0 & -b0
    return np.where(b0 == 0, 8, np.log2(np.maximum(low, 1)).astype(np.int64))


def decode_bc7(blk):
    """(n, 16) uint8 -> texels (n, 16, 4) int64, modes (n,).  Modes 0-3, 7 and the reserved block give (0, 0, 0, 0)."""
    blk = np.asarray(blk, np.uint8).reshape(-1, 16)
    n = len(blk)
    bits = ((blk[:, :, None] >> np.arange(8)) & 1).reshape(n, 128).astype(np.int64)
    mode = bc7_modes(blk)
    out = np.zeros((n, 16, 4), np.int64)

    def finish(ep0, ep1, wc, wa, rot):
        w = np.concatenate([np.repeat(wc[..., None], 3, -1), wa[..., None]], -1)  # (n, 16, 4)
        px = interp(ep0[:, None, :], ep1[:, None, :], w)
        res = px.copy()
        for r in (1, 2, 3):  # alpha and channel r - 1 change places
            m = rot == r
            res[m, :, 3] = px[m, :, r - 1]
            res[m, :, r - 1] = px[m, :, 3]
        return res

    # mode 6
    q = _get(bits, 7, 7, 8).reshape(n, 4, 2)
    p = _get(bits, 63, 1, 2)
    ep = 2 * q + p[:, None, :]
    w = W4[np.concatenate([_get(bits, 65, 3), _get(bits, 68, 4, 15)], -1)]
    d6 = finish(ep[:, :, 0], ep[:, :, 1], w, w, np.zeros(n, np.int64))
    # mode 5
    q = _get(bits, 8, 7, 6).reshape(n, 3, 2)
    col = (q << 1) | (q >> 6)
    al = _get(bits, 50, 8, 2)
    ep0 = np.concatenate([col[:, :, 0], al[:, :1]], -1)
    ep1 = np.concatenate([col[:, :, 1], al[:, 1:]], -1)
    d5 = finish(ep0, ep1, W2[_anchored(bits, 66, 2)], W2[_anchored(bits, 97, 2)], _get(bits, 6, 2)[:, 0])
    # mode 4
    q = _get(bits, 8, 5, 6).reshape(n, 3, 2)
    col = (q << 3) | (q >> 2)
    a = _get(bits, 38, 6, 2)
    al = (a << 2) | (a >> 4)
    ep0 = np.concatenate([col[:, :, 0], al[:, :1]], -1)
    ep1 = np.concatenate([col[:, :, 1], al[:, 1:]], -1)
    w2, w3 = W2[_anchored(bits, 50, 2)], W3[_anchored(bits, 81, 3)]
    sel = (_get(bits, 7, 1)[:, 0] == 1)[:, None]
    d4 = finish(ep0, ep1, np.where(sel, w3, w2), np.where(sel, w2, w3), _get(bits, 5, 2)[:, 0])
    for m, d in ((4, d4), (5, d5), (6, d6)):
        out[mode == m] = d[mode == m]
    return out, mode


def undecoded(mode):
    return (mode < 4) | (mode == 7)


def decode_blocks(blk, fmt):
    """(..., block bytes) uint8 -> texels (..., 16, 4) int64 by the RGBA rule, modes (...,) (8 outside BC7)"""
    blk = np.asarray(blk, np.uint8)
    lead = blk.shape[:-1]
    mode = np.full(lead, 8, np.int64)
    full = np.full(lead + (16, 1), 255, np.int64)
    zero = np.zeros(lead + (16, 1), np.int64)
    if fmt == 1:
        c0 = blk[..., 0].astype(np.int64) | (blk[..., 1].astype(np.int64) << 8)
        c1 = blk[..., 2].astype(np.int64) | (blk[..., 3].astype(np.int64) << 8)
        word = blk[..., 4:8].astype(np.int64)
        idx = ((word[..., None, :] << (8 * np.arange(4))).sum(-1) >> (2 * np.arange(16))) & 3
        alpha = np.where((c0 <= c1)[..., None] & (idx == 3), 0, 255)
        t = np.concatenate([bc_ref.decode_bc1(blk), alpha[..., None]], -1)
    elif fmt == 3:
        col = blk[..., 8:].copy()
        # always four-colour mode: the colours of the block with c0 > c1 forced do not depend on the order otherwise
        c0 = col[..., 0].astype(np.int64) | (col[..., 1].astype(np.int64) << 8)
        c1 = col[..., 2].astype(np.int64) | (col[..., 3].astype(np.int64) << 8)
        a, b = bc_ref.expand565(c0), bc_ref.expand565(c1)
        pal = np.stack([a, b, (2 * a + b + 1) // 3, (a + 2 * b + 1) // 3], -2)
        word = col[..., 4:8].astype(np.int64)
        idx = ((word[..., None, :] << (8 * np.arange(4))).sum(-1) >> (2 * np.arange(16))) & 3
        rgb = np.take_along_axis(pal, idx[..., None], -2)
        t = np.concatenate([rgb, bc_ref.decode_bc4(blk[..., :8])[..., None]], -1)
    elif fmt == 4:
        t = np.concatenate([bc_ref.decode_bc4(blk)[..., None], zero, zero, full], -1)
    elif fmt == 5:
        t = np.concatenate([bc_ref.decode_bc4(blk[..., :8])[..., None], bc_ref.decode_bc4(blk[..., 8:])[..., None], zero, full], -1)
    elif fmt == BC7:
        t, m = decode_bc7(blk.reshape(-1, 16))
        t, mode = t.reshape(lead + (16, 4)), m.reshape(lead)
    else:
        raise ValueError("unknown BC format %r" % (fmt,))
    return t.astype(np.int64), mode


def decode(blk, fmt, h, w):
    """(by, bx, block bytes) -> pixels uint8 (h, w, 4), the count of undecoded blocks"""
    t, mode = decode_blocks(blk, fmt)
    return bc_ref.unblock(t, h, w).astype(np.uint8), int(undecoded(mode).sum())


def error_record(src, blk, fmt):
    """kc_bc_error of the blocks against the RGBA8 bytes `src` (h, w, 4), as a dict"""
    src = np.asarray(src)
    h, w = src.shape[:2]
    t, mode = decode_blocks(blk, fmt)
    d = np.abs(bc_ref.unblock(t, h, w) - src.astype(np.int64))
    mask = CHANNEL_MASK[fmt]
    on = np.array([(mask >> c) & 1 for c in range(4)], np.int64)
    return dict(format=fmt, channel_mask=mask, pixels=h * w, sse=[int(v) for v in (d ** 2).sum((0, 1)) * on],
                max_abs=[int(v) for v in d.max((0, 1)) * on], undecoded_blocks=int(undecoded(mode).sum()),
                bc7_mode_blocks=[int((mode == k).sum()) for k in range(8)])


def psnr(rec, channels=None):
    chans = [c for c in range(4) if (rec["channel_mask"] >> c) & 1 and (channels is None or c in channels)]
    sse = sum(rec["sse"][c] for c in chans)
    return float("inf") if sse == 0 else 10 * np.log10(255.0 ** 2 * rec["pixels"] * len(chans) / sse)


# ------------------------------------------------------------------ random blocks that reach every branch
def force_mode(blk, mode):
    """(n, 16) uint8 random bytes -> the same with byte 0 made a block of `mode` (8: the reserved block)"""
    blk = np.array(blk, np.uint8).reshape(-1, 16)
    mode = np.broadcast_to(np.asarray(mode, np.int64), (len(blk),))
    keep = (0xff << (np.minimum(mode, 7) + 1)) & 0xff
    blk[:, 0] = np.where(mode == 8, 0, (blk[:, 0] & keep) | (1 << np.minimum(mode, 7)))
    return blk


def random_blocks(fmt, n, seed=0):
    """n random blocks of a format, (n, block bytes) uint8.  BC7: modes 4, 5 and 6 take turns, with one block each of modes 0,
    1, 2, 3, 7 and the reserved block after every 18 (n >= 24 holds them all); the rotation and the index selection are the
    random bits they are.  BC1 / BC4: endpoints in both orders, and equal ones in every eighth block."""
    rng = np.random.default_rng(seed + 1000 * fmt)
    blk = rng.integers(0, 256, (n, BLOCK_BYTES[fmt]), dtype=np.uint8)
    if fmt == BC7:
        cycle = np.array([4, 5, 6] * 6 + [0, 1, 2, 3, 7, 8])
        blk = force_mode(blk, cycle[np.arange(n) % len(cycle)])
    else:
        for at in ((0,) if fmt in (1, 4) else (0, 8)):
            # BC1's endpoints are the u16 at +0 and +2 (in BC3 at +8 and +10), BC4's the bytes at +0 and +1
            if fmt == 1 or (fmt == 3 and at == 8):
                blk[::8, at + 2:at + 4] = blk[::8, at:at + 2]
            else:
                blk[::8, at + 1] = blk[::8, at]
    return blk


def random_image_blocks(fmt, h, w, seed=0):
    by, bx = (h + 3) // 4, (w + 3) // 4
    return random_blocks(fmt, by * bx, seed + 7 * h + w).reshape(by, bx, BLOCK_BYTES[fmt])


# ------------------------------------------------------------------ .dds
class DdsError(Exception):
    def __init__(self, code, what):
        Exception.__init__(self, what)
        self.code = code


def _levels(w, h):
    return 1 + int(np.floor(np.log2(max(w, h))))


def chain_bytes(w, h, fmt, levels):
    return sum(((max(1, w >> k) + 3) // 4) * ((max(1, h >> k) + 3) // 4) * BLOCK_BYTES[fmt] for k in range(levels))


def dds_parse(data):
    """kc_dds_parse -> dict(width, height, format, flags, levels, data_offset, data_bytes); DdsError(code) otherwise"""
    data = bytes(data)
    if len(data) < 128:
        raise DdsError(KC_ERR_INVALID_ARG, "short")
    d = struct.unpack("<32I", data[:128])
    if d[0] != 0x20534444 or d[1] != 124 or d[19] != 32 or d[3] == 0 or d[4] == 0:
        raise DdsError(KC_ERR_INVALID_ARG, "malformed")
    h, w = d[3], d[4]
    dx10 = bool(d[20] & 4) and d[21] == 0x30315844
    if dx10 and len(data) < 148:
        raise DdsError(KC_ERR_INVALID_ARG, "short DX10 header")
    if not d[20] & 4:
        raise DdsError(KC_ERR_UNSUPPORTED, "uncompressed")
    if d[28] & 0x200 or d[28] & 0x200000 or (d[2] & 0x800000 and d[6] > 1):
        raise DdsError(KC_ERR_UNSUPPORTED, "cube map or volume")
    flags = 0
    if dx10:
        x = struct.unpack("<5I", data[128:148])
        by_dxgi = {v: k for k, v in DXGI.items()}
        if x[0] not in by_dxgi or x[1] != 3 or x[2] & 4 or x[3] != 1:
            raise DdsError(KC_ERR_UNSUPPORTED, "dxgi format, dimension, cube or array")
        fmt, srgb = by_dxgi[x[0]]
        flags = BC_SRGB if srgb else 0
    else:
        cc = {b"DXT1": 1, b"DXT5": 3, b"ATI1": 4, b"BC4U": 4, b"ATI2": 5, b"BC5U": 5}
        name = struct.pack("<I", d[21])
        if name not in cc:
            raise DdsError(KC_ERR_UNSUPPORTED, "FourCC")
        fmt = cc[name]
    levels = d[7] if d[2] & 0x20000 and d[7] else 1
    if levels > _levels(w, h):
        raise DdsError(KC_ERR_INVALID_ARG, "levels")
    off = 148 if dx10 else 128
    nbytes = chain_bytes(w, h, fmt, levels)
    if len(data) - off < nbytes:
        raise DdsError(KC_ERR_INVALID_ARG, "short payload")
    return dict(width=w, height=h, format=fmt, flags=flags, levels=levels, data_offset=off, data_bytes=nbytes)


def legacy_header(w, h, fourcc, levels=1):
    """the 128 bytes of a legacy FourCC header"""
    d = [0] * 32
    d[0], d[1] = 0x20534444, 124
    d[2] = 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000 | (0x20000 if levels > 1 else 0)
    d[3], d[4], d[7] = h, w, levels
    d[19], d[20], d[21] = 32, 4, struct.unpack("<I", fourcc)[0]
    d[27] = 0x1000 | (0x400008 if levels > 1 else 0)
    return struct.pack("<32I", *d)
