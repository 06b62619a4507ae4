"""Numpy reference of the all-modes decode contract (include/kanter_core_amd.h, KC_BC_ALL_MODES): every BC7 mode 0-7 and every
unsigned BC6H mode 1-14, the partition and anchor tables included; the error record of kc_image_bc_compare under the flag; and
random blocks that walk every (mode, partition) pair.  The tables and bit layouts are the formats' own (the BC7 and BC6H
definitions of Direct3D 11 / BPTC).  BC7 texels are (n, 16, 4) integers 0..255, BC6H texels (n, 16, 3) half bit patterns.
On modes 4, 5, 6 and 11-14 this file and bc_decode_ref / bc6h_ref agree: it is a superset.  Imports nothing from the product."""
import numpy as np

import bc6h_ref
import bc_decode_ref
from bc6h_ref import fin, unq
from bc7_ref import W2, W4, interp
from bc_decode_ref import W3, bc7_modes
from bc_ref import unblock

BC7, BC6H = 98, 95
BC_ALL_MODES = 16
WEIGHTS = {2: W2, 3: W3, 4: W4}

# ------------------------------------------------------------------ the partition tables
# Two subsets: bit t of entry p = the subset of texel t (t = 4 y + x).  BC6H uses the first 32.
P2 = np.array([
    0xCCCC, 0x8888, 0xEEEE, 0xECC8, 0xC880, 0xFEEC, 0xFEC8, 0xEC80, 0xC800, 0xFFEC, 0xFE80, 0xE800, 0xFFE8, 0xFF00, 0xFFF0, 0xF000,
    0xF710, 0x008E, 0x7100, 0x08CE, 0x008C, 0x7310, 0x3100, 0x8CCE, 0x088C, 0x3110, 0x6666, 0x366C, 0x17E8, 0x0FF0, 0x718E, 0x399C,
    0xAAAA, 0xF0F0, 0x5A5A, 0x33CC, 0x3C3C, 0x55AA, 0x9696, 0xA55A, 0x73CE, 0x13C8, 0x324C, 0x3BDC, 0x6996, 0xC33C, 0x9966, 0x0660,
    0x0272, 0x04E4, 0x4E40, 0x2720, 0xC936, 0x936C, 0x39C6, 0x639C, 0x9336, 0x9CC6, 0x817E, 0xE718, 0xCCF0, 0x0FCC, 0x7744, 0xEE22], np.int64)
# Three subsets: bits 2t..2t+1 of entry p = the subset of texel t
P3 = np.array([
    0xAA685050, 0x6A5A5040, 0x5A5A4200, 0x5450A0A8, 0xA5A50000, 0xA0A05050, 0x5555A0A0, 0x5A5A5050,
    0xAA550000, 0xAA555500, 0xAAAA5500, 0x90909090, 0x94949494, 0xA4A4A4A4, 0xA9A59450, 0x2A0A4250,
    0xA5945040, 0x0A425054, 0xA5A5A500, 0x55A0A0A0, 0xA8A85454, 0x6A6A4040, 0xA4A45000, 0x1A1A0500,
    0x0050A4A4, 0xAAA59090, 0x14696914, 0x69691400, 0xA08585A0, 0xAA821414, 0x50A4A450, 0x6A5A0200,
    0xA9A58000, 0x5090A0A8, 0xA8A09050, 0x24242424, 0x00AA5500, 0x24924924, 0x24499224, 0x50A50A50,
    0x500AA550, 0xAAAA4444, 0x66660000, 0xA5A0A5A0, 0x50A050A0, 0x69286928, 0x44AAAA44, 0x66666600,
    0xAA444444, 0x54A854A8, 0x95809580, 0x96969600, 0xA85454A8, 0x80959580, 0xAA141414, 0x96960000,
    0xAAAA1414, 0xA05050A0, 0xA0A5A5A0, 0x96000000, 0x40804080, 0xA9A8A9A8, 0xAAAAAA44, 0x2A4A5254], np.int64)
# The anchor texels: of subset 1 with two subsets, of subsets 1 and 2 with three.  Texel 0 is always the anchor of subset 0.
A2 = np.array([
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
    15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6, 6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15], np.int64)
A3_1 = np.array([
    3, 3, 15, 15, 8, 3, 15, 15, 8, 8, 6, 6, 6, 5, 3, 3, 3, 3, 8, 15, 3, 3, 6, 10, 5, 8, 8, 6, 8, 5, 15, 15,
    8, 15, 3, 5, 6, 10, 8, 15, 15, 3, 15, 5, 15, 15, 15, 15, 3, 15, 5, 5, 5, 8, 5, 10, 5, 10, 8, 13, 15, 12, 3, 3], np.int64)
A3_2 = np.array([
    15, 8, 8, 3, 15, 15, 3, 8, 15, 15, 15, 15, 15, 15, 15, 8, 15, 8, 15, 3, 15, 8, 15, 8, 3, 15, 6, 10, 15, 15, 10, 8,
    15, 3, 15, 10, 10, 8, 9, 10, 6, 15, 8, 15, 3, 6, 6, 8, 15, 3, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 3, 15, 15, 8], np.int64)


def subsets2(p):
    """partition indices (n,) -> the subset of every texel (n, 16), two subsets"""
    return (P2[np.asarray(p)][:, None] >> np.arange(16)) & 1


def subsets3(p):
    return (P3[np.asarray(p)][:, None] >> (2 * np.arange(16))) & 3


# ------------------------------------------------------------------ BC7
# mode -> subsets, partition bits, rotation bits, index selection bits, colour bits, alpha bits, p-bits (0 none, 1 one per
# endpoint, 2 one per subset), index bits, second index set's bits
BC7_MODES = {
    0: (3, 4, 0, 0, 4, 0, 1, 3, 0),
    1: (2, 6, 0, 0, 6, 0, 2, 3, 0),
    2: (3, 6, 0, 0, 5, 0, 0, 2, 0),
    3: (2, 6, 0, 0, 7, 0, 1, 2, 0),
    4: (1, 0, 2, 1, 5, 6, 0, 2, 3),
    5: (1, 0, 2, 0, 7, 8, 0, 2, 2),
    6: (1, 0, 0, 0, 7, 7, 1, 4, 0),
    7: (2, 6, 0, 0, 5, 5, 1, 2, 0),
}
BC7_CYCLE = [(0, p) for p in range(16)] + [(m, p) for m in (1, 2, 3, 7) for p in range(64)] + [(4, 0), (5, 0), (6, 0), (8, 0)]
assert len(BC7_CYCLE) == 276


def _bits(blk):
    blk = np.asarray(blk, np.uint8).reshape(-1, 16)
    return ((blk[:, :, None] >> np.arange(8)) & 1).reshape(len(blk), 128).astype(np.int64)


def _pack(bits):
    return (bits.reshape(len(bits), 16, 8) << np.arange(8)).sum(-1).astype(np.uint8)


def _get(bits, at, n, count=1):
    return (bits[:, at:at + n * count].reshape(len(bits), count, n) << np.arange(n)).sum(-1)


def _indices(bits, base, n, anchors):
    """(blocks, 16) n-bit indices from bit `base`; the texels of `anchors` (blocks, k) store one bit less: texel t lies at
    base + n t - (anchors below t)"""
    rows = np.arange(len(bits))
    t = np.arange(16)
    below = (anchors[:, None, :] < t[None, :, None]).sum(-1)
    is_anchor = (anchors[:, None, :] == t[None, :, None]).any(-1)
    at = base + n * t[None, :] - below
    out = np.zeros((len(bits), 16), np.int64)
    for k in range(n):
        use = ~is_anchor | (k < n - 1)
        out += np.where(use, bits[rows[:, None], np.minimum(at + k, 127)], 0) << k
    return out


def _bc7_mode(bits, m):
    """every block read as mode m -> texels (n, 16, 4)"""
    ns, pb, rb, isb, cb, ab, pk, ib, ib2 = BC7_MODES[m]
    n = len(bits)
    at = m + 1
    part = _get(bits, at, pb)[:, 0] if pb else np.zeros(n, np.int64)
    at += pb
    rot = _get(bits, at, rb)[:, 0] if rb else np.zeros(n, np.int64)
    at += rb
    sel = _get(bits, at, isb)[:, 0] if isb else np.zeros(n, np.int64)
    at += isb
    ne = 2 * ns
    col = _get(bits, at, cb, 3 * ne).reshape(n, 3, ne)  # all R, then all G, then all B; endpoint e = 2 subset + (0 | 1)
    at += 3 * ne * cb
    if ab:
        al = _get(bits, at, ab, ne).reshape(n, 1, ne)
        at += ne * ab
    else:
        al = np.zeros((n, 1, ne), np.int64)
    if pk == 1:
        p = _get(bits, at, 1, ne)
        at += ne
    elif pk == 2:
        p = np.repeat(_get(bits, at, 1, ns), 2, -1)
        at += ns
    # to 8 bits: the p-bit below the stored bits, then the top bits repeated below
    def expand(q, nb):
        if nb == 0:
            return np.full(q.shape, 255, np.int64)
        if pk:
            q, nb = (q << 1) | p[:, None, :], nb + 1
        v = q << (8 - nb)
        return v | (v >> nb)
    ep = np.concatenate([expand(col, cb), expand(al, ab)], 1)  # (n, 4, ne)
    if ns == 1:
        sub = np.zeros((n, 16), np.int64)
        anchors = np.zeros((n, 1), np.int64)
    elif ns == 2:
        sub = subsets2(part)
        anchors = np.stack([np.zeros(n, np.int64), A2[part]], -1)
    else:
        sub = subsets3(part)
        anchors = np.stack([np.zeros(n, np.int64), A3_1[part], A3_2[part]], -1)
    i1 = _indices(bits, at, ib, anchors)
    at += 16 * ib - ns
    w1 = WEIGHTS[ib][i1]
    if ib2:
        i2 = _indices(bits, at, ib2, anchors)
        at += 16 * ib2 - ns
        w2 = WEIGHTS[ib2][i2]
    else:
        w2 = w1
    assert at == 128, (m, at)
    s = (sel == 1)[:, None]
    wc, wa = np.where(s, w2, w1), np.where(s, w1, w2)
    w = np.concatenate([np.repeat(wc[..., None], 3, -1), wa[..., None]], -1)  # (n, 16, 4)
    e0 = np.take_along_axis(ep, (2 * sub)[:, None, :], 2).transpose(0, 2, 1)
    e1 = np.take_along_axis(ep, (2 * sub + 1)[:, None, :], 2).transpose(0, 2, 1)
    px = interp(e0, e1, w)
    if ab == 0:
        px[..., 3] = 255
    res = px.copy()
    for r in (1, 2, 3):  # alpha and channel r - 1 change places
        k = rot == r
        res[k, :, 3] = px[k, :, r - 1]
        res[k, :, r - 1] = px[k, :, 3]
    return res


def decode_bc7(blk):
    """(..., 16) uint8 -> texels (..., 16, 4) int64, modes (...,); only the reserved block (mode 8) gives (0, 0, 0, 0)"""
    blk = np.asarray(blk, np.uint8)
    lead = blk.shape[:-1]
    bits = _bits(blk)
    mode = bc7_modes(blk)
    out = np.zeros((len(bits), 16, 4), np.int64)
    for m in BC7_MODES:
        k = mode == m
        if k.any():
            out[k] = _bc7_mode(bits[k], m)
    return out.reshape(lead + (16, 4)), mode.reshape(lead)


# ------------------------------------------------------------------ BC6H
# The header of a two-subset mode, field by field from bit 0, as the format definition lists it: endpoint e of a channel is
# r0..r3 (the definition's rw, rx, ry, rz), d the partition index.  mode -> (bits of endpoint 0, (delta bits of R, G, B), fields)
BC6H_TWO = {
    1: (10, (5, 5, 5), "m[1:0] g2[4] b2[4] b3[4] r0[9:0] g0[9:0] b0[9:0] r1[4:0] g3[4] g2[3:0] g1[4:0] b3[0] g3[3:0] b1[4:0] b3[1] "
                       "b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3] d[4:0]"),
    2: (7, (6, 6, 6), "m[1:0] g2[5] g3[4] g3[5] r0[6:0] b3[0] b3[1] b2[4] g0[6:0] b2[5] b3[2] g2[4] b0[6:0] b3[3] b3[5] b3[4] "
                      "r1[5:0] g2[3:0] g1[5:0] g3[3:0] b1[5:0] b2[3:0] r2[5:0] r3[5:0] d[4:0]"),
    3: (11, (5, 4, 4), "m[4:0] r0[9:0] g0[9:0] b0[9:0] r1[4:0] r0[10] g2[3:0] g1[3:0] g0[10] b3[0] g3[3:0] b1[3:0] b0[10] b3[1] "
                       "b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3] d[4:0]"),
    4: (11, (4, 5, 4), "m[4:0] r0[9:0] g0[9:0] b0[9:0] r1[3:0] r0[10] g3[4] g2[3:0] g1[4:0] g0[10] g3[3:0] b1[3:0] b0[10] b3[1] "
                       "b2[3:0] r2[3:0] b3[0] b3[2] r3[3:0] g2[4] b3[3] d[4:0]"),
    5: (11, (4, 4, 5), "m[4:0] r0[9:0] g0[9:0] b0[9:0] r1[3:0] r0[10] b2[4] g2[3:0] g1[3:0] g0[10] b3[0] g3[3:0] b1[4:0] b0[10] "
                       "b2[3:0] r2[3:0] b3[1] b3[2] r3[3:0] b3[4] b3[3] d[4:0]"),
    6: (9, (5, 5, 5), "m[4:0] r0[8:0] b2[4] g0[8:0] g2[4] b0[8:0] b3[4] r1[4:0] g3[4] g2[3:0] g1[4:0] b3[0] g3[3:0] b1[4:0] b3[1] "
                      "b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3] d[4:0]"),
    7: (8, (6, 5, 5), "m[4:0] r0[7:0] g3[4] b2[4] g0[7:0] b3[2] g2[4] b0[7:0] b3[3] b3[4] r1[5:0] g2[3:0] g1[4:0] b3[0] g3[3:0] "
                      "b1[4:0] b3[1] b2[3:0] r2[5:0] r3[5:0] d[4:0]"),
    8: (8, (5, 6, 5), "m[4:0] r0[7:0] b3[0] b2[4] g0[7:0] g2[5] g2[4] b0[7:0] g3[5] b3[4] r1[4:0] g3[4] g2[3:0] g1[5:0] g3[3:0] "
                      "b1[4:0] b3[1] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3] d[4:0]"),
    9: (8, (5, 5, 6), "m[4:0] r0[7:0] b3[1] b2[4] g0[7:0] b2[5] g2[4] b0[7:0] b3[5] b3[4] r1[4:0] g3[4] g2[3:0] g1[4:0] b3[0] "
                      "g3[3:0] b1[5:0] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3] d[4:0]"),
    10: (6, (0, 0, 0), "m[4:0] r0[5:0] g3[4] b3[0] b3[1] b2[4] g0[5:0] g2[5] b2[5] b3[2] g2[4] b0[5:0] g3[5] b3[3] b3[5] b3[4] "
                       "r1[5:0] g2[3:0] g1[5:0] g3[3:0] b1[5:0] b2[3:0] r2[5:0] r3[5:0] d[4:0]"),
}
BC6H_CYCLE = [(m, p) for m in range(1, 11) for p in range(32)] + [(m, 0) for m in (11, 12, 13, 14)] + [(-f, 0) for f in bc6h_ref.RESERVED]
assert len(BC6H_CYCLE) == 328


def bc6h_fields(mode):
    """mode 1..10 -> [(name, lowest value bit, bits, block bit)] in block order; the header is 82 bits"""
    out, at = [], 0
    for tok in BC6H_TWO[mode][2].split():
        name, rng = tok[:-1].split("[")
        hi, lo = (int(v) for v in rng.split(":")) if ":" in rng else (int(rng), int(rng))
        out.append((name, lo, hi - lo + 1, at))
        at += hi - lo + 1
    assert at == 82, (mode, at)
    return out


def _bc6h_two(bits, m, round_term):
    nb, delta, _ = BC6H_TWO[m]
    n = len(bits)
    val = {}
    for name, lo, cnt, at in bc6h_fields(m):
        val[name] = val.get(name, np.zeros(n, np.int64)) | (_get(bits, at, cnt)[:, 0] << lo)
    part = val["d"]
    ep = np.zeros((n, 3, 4), np.int64)
    for c, ch in enumerate("rgb"):
        e0 = val[ch + "0"]
        ep[:, c, 0] = e0
        for e in (1, 2, 3):
            x = val[ch + str(e)]
            if delta[c]:  # a signed delta, added modulo 2^nb
                x = (e0 + x - ((x >> (delta[c] - 1)) << delta[c])) & ((1 << nb) - 1)
            ep[:, c, e] = x
    u = unq(ep, nb)
    sub = subsets2(part)
    idx = _indices(bits, 82, 3, np.stack([np.zeros(n, np.int64), A2[part]], -1))
    u0 = np.take_along_axis(u, (2 * sub)[:, None, :], 2).transpose(0, 2, 1)  # (n, 16, 3)
    u1 = np.take_along_axis(u, (2 * sub + 1)[:, None, :], 2).transpose(0, 2, 1)
    return fin(bc6h_ref.interp(u0, u1, W3[idx][:, :, None], round_term))


def decode_bc6h(blk, round_term=32):
    """(..., 16) uint8 -> texels (..., 16, 3) half bit patterns, modes (...,) (0: a reserved mode field, which gives (0, 0, 0))"""
    blk = np.asarray(blk, np.uint8)
    lead = blk.shape[:-1]
    flat = blk.reshape(-1, 16)
    out, mode = bc6h_ref.decode_blocks(flat, round_term)  # modes 11-14; zero elsewhere
    out = out.copy()
    bits = _bits(flat)
    for m in BC6H_TWO:
        k = mode == m
        if k.any():
            out[k] = _bc6h_two(bits[k], m, round_term)
    return out.reshape(lead + (16, 3)), mode.reshape(lead)


# ------------------------------------------------------------------ images and records
def decode(blk, fmt, h, w):
    """(by, bx, 16) -> BC7: pixels uint8 (h, w, 4); BC6H: half bit patterns (h, w, 3).  Nothing is undecoded."""
    if fmt == BC7:
        return unblock(decode_bc7(blk)[0], h, w).astype(np.uint8)
    return unblock(decode_bc6h(blk)[0], h, w)


def decode_planes(blk, h, w):
    """the f32 planes kc_image_from_bc makes of BC6H blocks under the flag: R, G, B the halves' exact values, A = 1"""
    px = decode(blk, BC6H, h, w)
    return [bc6h_ref.half_value(px[..., c]) for c in range(3)] + [np.ones((h, w), np.float32)]


def error_record(src, blk, fmt):
    """kc_bc_error under the flag.  BC7: src the RGBA8 bytes (h, w, 4); BC6H: src the image's f32 planes"""
    if fmt == BC7:
        src = np.asarray(src)
        h, w = src.shape[:2]
        t, mode = decode_bc7(blk)
        d = np.abs(unblock(t, h, w) - src.astype(np.int64))
        return dict(format=BC7, channel_mask=0xF, pixels=h * w, sse=[int(v) for v in (d ** 2).sum((0, 1))],
                    max_abs=[int(v) for v in d.max((0, 1))], undecoded_blocks=0, bc7_mode_blocks=[int((mode == k).sum()) for k in range(8)])
    tx = bc6h_ref.texels(src)
    h, w = tx.shape[:2]
    d = np.abs(unblock(decode_bc6h(blk)[0], h, w) - tx)
    return dict(format=BC6H, channel_mask=0x7, pixels=h * w, sse=[int(v) for v in (d ** 2).sum((0, 1))] + [0],
                max_abs=[int(v) for v in d.max((0, 1))] + [0], undecoded_blocks=0, bc7_mode_blocks=[0] * 8)


# ------------------------------------------------------------------ random blocks that walk every (mode, partition) pair
def set_field(blk, at, n, value):
    """(k, 16) uint8, in place: the n bits from bit `at` = value (k,)"""
    value = np.broadcast_to(np.asarray(value, np.int64), (len(blk),))
    for b in range(n):
        byte, bit = (at + b) >> 3, (at + b) & 7
        blk[:, byte] = (blk[:, byte] & (0xff ^ (1 << bit))) | (((value >> b) & 1) << bit).astype(np.uint8)


def low_endpoint0(blk):
    """BC6H blocks with the top bit of every channel's endpoint 0 cleared (mode 10, whose four endpoints are all plain: of every
    endpoint), so that most texels decode inside [0, 1]; modes 11-14 as bc6h_ref.clear_top_bit_of_endpoint0"""
    blk = bc6h_ref.clear_top_bit_of_endpoint0(blk)
    mode = bc6h_ref.modes(blk)
    for m, (nb, _, _) in BC6H_TWO.items():
        k = mode == m
        if not k.any():
            continue
        part = blk[k]
        for name, lo, cnt, at in bc6h_fields(m):
            if name[0] in "rgb" and (name[1] == "0" or m == 10) and lo <= nb - 1 < lo + cnt:
                set_field(part, at + nb - 1 - lo, 1, 0)
        blk[k] = part
    return blk


def random_blocks(fmt, n, seed=0, low=False):
    """n random blocks (n, 16) uint8 whose (mode, partition) pairs follow the format's cycle -- BC7: 276 blocks, 16 partitions of
    mode 0, 64 each of modes 1, 2, 3 and 7, modes 4, 5 and 6 and the reserved block; BC6H: 328 blocks, 32 partitions of each of
    modes 1-10, modes 11-14 and the four reserved field values -- and whose other bits are random"""
    rng = np.random.default_rng(seed + 1000 * fmt + 77)
    blk = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    cycle = BC7_CYCLE if fmt == BC7 else BC6H_CYCLE
    which = np.arange(n) % len(cycle)
    mode = np.array([cycle[k][0] for k in which], np.int64)
    part = np.array([cycle[k][1] for k in which], np.int64)
    if fmt == BC7:
        blk = bc_decode_ref.force_mode(blk, mode)
        for m in (0, 1, 2, 3, 7):
            k = mode == m
            sub = blk[k]
            set_field(sub, m + 1, BC7_MODES[m][1], part[k])
            blk[k] = sub
        return blk
    blk = bc6h_ref.force_mode(blk, mode)
    k = (mode >= 1) & (mode <= 10)
    sub = blk[k]
    set_field(sub, 77, 5, part[k])
    blk[k] = sub
    return low_endpoint0(blk) if low else blk


def pairs(blk, fmt):
    """the (mode, partition) pair of every block, as the cycles name them: partition 0 for the modes without one; BC7's reserved
    block is mode 8, a reserved BC6H field value f is mode -f"""
    blk = np.asarray(blk, np.uint8).reshape(-1, 16)
    bits = _bits(blk)
    if fmt == BC7:
        mode = bc7_modes(blk)
        part = np.zeros(len(blk), np.int64)
        for m in (0, 1, 2, 3, 7):
            part = np.where(mode == m, _get(bits, m + 1, BC7_MODES[m][1])[:, 0], part)
    else:
        mode = bc6h_ref.modes(blk)
        part = np.where((mode >= 1) & (mode <= 10), _get(bits, 77, 5)[:, 0], 0)
        mode = np.where(mode == 0, -(blk[:, 0].astype(np.int64) & 31), mode)
    return list(zip(mode.tolist(), part.tolist()))


def random_image_blocks(fmt, h, w, seed=0):
    by, bx = (h + 3) // 4, (w + 3) // 4
    return random_blocks(fmt, by * bx, seed + 7 * h + w).reshape(by, bx, 16)
