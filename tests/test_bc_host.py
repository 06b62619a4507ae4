"""Block compression without a device: the contract's worked blocks and quality figures through the numpy reference
(tests/bc_ref.py), properties of random blocks, the ctypes struct against the header, and kc_bc_image_validate's arithmetic
before kc_init."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bc_ref
from pngio import read_png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
KC_OK, KC_ERR_NO_DEVICE, KC_ERR_INVALID_ARG = 0, 101, 102


def hexb(a):
    return np.asarray(a, np.uint8).tobytes().hex(" ")


def two_colour_block():
    return np.array([(255, 0, 0) if t % 4 < 2 else (0, 255, 0) for t in range(16)])


def test_worked_blocks():
    assert hexb(bc_ref.encode_bc1(two_colour_block())) == "80 e8 60 17 50 50 50 50"
    assert hexb(bc_ref.encode_bc1(two_colour_block(), swap=False)) == "60 ef 80 10 aa aa aa aa"
    assert hexb(bc_ref.encode_bc1(np.full((16, 3), 128))) == "10 84 10 84 00 00 00 00"
    assert hexb(bc_ref.encode_bc4(17 * np.arange(16))) == "ff 00 c9 6f b7 e4 26 01"
    assert hexb(bc_ref.encode_bc4(np.full(16, 77))) == "4d 4d 00 00 00 00 00 00"
    # without the swap the block decodes to olive everywhere
    assert (bc_ref.decode_bc1(bc_ref.encode_bc1(two_colour_block(), swap=False)) == (165, 165, 0)).all()


def test_block_layouts_of_bc3_and_bc5():
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, size=(4, 4, 4), dtype=np.uint8)
    t = px.reshape(16, 4).astype(np.int64)
    assert hexb(bc_ref.encode(px, 3)[0, 0]) == hexb(np.concatenate([bc_ref.encode_bc4(t[:, 3]), bc_ref.encode_bc1(t[:, :3])]))
    assert hexb(bc_ref.encode(px, 5)[0, 0]) == hexb(np.concatenate([bc_ref.encode_bc4(t[:, 0]), bc_ref.encode_bc4(t[:, 1])]))
    assert hexb(bc_ref.encode(px, 4)[0, 0]) == hexb(bc_ref.encode_bc4(t[:, 0]))


def test_edge_blocks_repeat_the_last_column_and_row():
    rng = np.random.default_rng(6)
    px = rng.integers(0, 256, size=(5, 3, 4), dtype=np.uint8)
    t = bc_ref.blocks(px)
    assert t.shape == (2, 1, 16, 4)
    for j in range(2):
        for y in range(4):
            for x in range(4):
                assert (t[j, 0, 4 * y + x] == px[min(4 * j + y, 4), min(x, 2)]).all()


@pytest.mark.parametrize("name,with_swap,without_swap", [("clouds.png", 43.19, 43.19), ("image_1.png", 47.47, 47.47),
                                                         ("heart_256.png", 35.15, 34.21), ("image_2.png", 29.74, 28.53)])
def test_bc1_psnr(name, with_swap, without_swap):
    a = read_png(os.path.join(INPUTS, name))
    rgb = (np.repeat(a[..., :1], 3, -1) if a.shape[2] < 3 else a[..., :3]).astype(np.int64)
    h, w = rgb.shape[:2]
    for swap, want in ((True, with_swap), (False, without_swap)):
        dec = bc_ref.unblock(bc_ref.decode_bc1(bc_ref.encode_bc1(bc_ref.blocks(rgb), swap=swap)), h, w)
        mse = ((dec - rgb) ** 2).mean()
        assert round(10 * np.log10(255.0 ** 2 / mse), 2) == want, (name, swap)


def random_blocks(n, seed):
    """uniform, narrow-range and two-level blocks: every branch of the rules"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(n, 16, 4))
    base = rng.integers(0, 240, size=(n, 1, 4))
    b = base + rng.integers(0, 16, size=(n, 16, 4))
    c = np.where(rng.random((n, 16, 1)) < 0.5, rng.integers(0, 256, size=(n, 1, 4)), rng.integers(0, 256, size=(n, 1, 4)))
    d = np.repeat(rng.integers(0, 256, size=(n, 1, 4)), 16, 1)
    return np.concatenate([a, b, c, d])


def test_bc4_error_bound():
    v = random_blocks(4000, 1)[..., 0]
    dec = bc_ref.decode_bc4(bc_ref.encode_bc4(v))
    d = v.max(-1) - v.min(-1)
    assert (14 * np.abs(dec - v) <= d[:, None] + 14).all()


def test_bc1_indices_are_nearest_and_mode_is_four_colour():
    p = random_blocks(4000, 2)[..., :3]
    blk = bc_ref.encode_bc1(p)
    c0 = blk[:, 0].astype(np.int64) | (blk[:, 1].astype(np.int64) << 8)
    c1 = blk[:, 2].astype(np.int64) | (blk[:, 3].astype(np.int64) << 8)
    word = blk[:, 4:].copy().view("<u4")[:, 0].astype(np.int64)
    idx = (word[:, None] >> (2 * np.arange(16))) & 3
    assert (c0[(idx != 0).any(-1)] > c1[(idx != 0).any(-1)]).all()
    e0, e1 = bc_ref.expand565(c0), bc_ref.expand565(c1)
    pal = np.stack([3 * e0, 3 * e1, 2 * e0 + e1, e0 + 2 * e1], 1)  # (n, 4, 3)
    err = ((3 * p[:, :, None, :] - pal[:, None, :, :]) ** 2).sum(-1)  # (n, 16, 4)
    chosen = np.take_along_axis(err, idx[..., None], -1)[..., 0]
    live = c0 != c1
    assert (chosen[live] == err[live].min(-1)).all()
    assert (idx[~live] == 0).all()


# ---- the C ABI without a device
def test_symbols_and_struct_layout(tmp_path):
    from kanter_core_amd import _lib
    L = _lib.load()
    for name in ("kc_bc_image_validate", "kc_image_to_bc", "kc_image_to_bc_device", "kc_live_graph_buffer_bc"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    src = tmp_path / "layout.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "kanter_core_amd.h"
#define F(m) printf(#m " %zu\\n", offsetof(kc_bc_image, m))
int main(void)
{
    printf("sizeof %zu\\n", sizeof(kc_bc_image));
    F(ptr); F(width); F(height); F(format); F(row_pitch_bytes);
    printf("KC_BC1 %d\\nKC_BC3 %d\\nKC_BC4 %d\\nKC_BC5 %d\\nKC_BC_SRGB %u\\n", KC_BC1, KC_BC3, KC_BC4, KC_BC5, KC_BC_SRGB);
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    S = _lib.kc_bc_image
    assert int(got["sizeof"]) == C.sizeof(S)
    for f, _ in S._fields_:
        assert int(got[f]) == getattr(S, f).offset, f
    assert [int(got[k]) for k in ("KC_BC1", "KC_BC3", "KC_BC4", "KC_BC5", "KC_BC_SRGB")] == [1, 3, 4, 5, 1]


def validate(desc):
    from kanter_core_amd import _lib
    ext = C.c_size_t(12345)
    status = _lib.load().kc_bc_image_validate(C.byref(desc), C.byref(ext))
    return status, ext.value


def test_validate_arithmetic_refusals():
    from kanter_core_amd import _lib
    D = _lib.kc_bc_image
    base = 1 << 20
    for d in (D(base, 8, 8, 2, 32),             # unknown format
              D(base, 8, 8, 0, 32),
              D(base, 0, 8, 1, 16),             # zero width
              D(base, 8, 0, 1, 16),             # zero height
              D(None, 8, 8, 1, 16),             # NULL pointer
              D(base + 8, 8, 8, 3, 32),         # pointer not a multiple of 16-byte blocks
              D(base + 4, 8, 8, 1, 16),         # ... of 8-byte blocks
              D(base, 8, 8, 3, 40),             # pitch not a multiple of the block bytes
              D(base, 8, 8, 1, 8),              # pitch below bx * block bytes
              D(base, (1 << 18) + 4, 1 << 17, 4, (1 << 17) * 8),  # 2^31 + 2^15 blocks
              D(base, 4, 4 << 20, 1, 1 << 62),  # the extent overflows
              D((1 << 64) - 16, 4, 8, 3, 16)):  # ptr + extent wraps
        status, _ = validate(d)
        assert status == KC_ERR_INVALID_ARG, (d.format, d.width, d.height, d.row_pitch_bytes)


def test_validate_extent_then_no_device():
    import torch
    from kanter_core_amd import _lib
    D = _lib.kc_bc_image
    gpu = torch.cuda.is_available()
    for d, ext in ((D(1 << 20, 1, 1, 1, 8), 8), (D(1 << 20, 5, 3, 3, 32), 32), (D(1 << 20, 13, 9, 4, 64), 2 * 64 + 32),
                   (D(1 << 20, 1 << 16, 1 << 17, 5, 1 << 18), ((1 << 15) - 1) * (1 << 18) + (1 << 18)),
                   (D(1 << 20, 1 << 17, 1 << 16, 1, 1 << 18), ((1 << 14) - 1) * (1 << 18) + (1 << 18))):
        status, got = validate(d)
        assert got == ext
        if not gpu:  # the not-gpu suite also runs on a machine with a device, which may or may not be initialised
            assert status == KC_ERR_NO_DEVICE
