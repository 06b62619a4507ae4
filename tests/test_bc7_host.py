"""BC7 without a device: the contract's worked blocks through the numpy reference (tests/bc7_ref.py), layout properties of
random blocks, the bit layout against Pillow's decoder, quality against the project's BC1 and BC3 encoders, and the C ABI's
arithmetic entries with format 98 before kc_init."""
import ctypes as C
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bc7_ref
import bc_ref
from pngio import read_png
from test_bc_host import random_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
KC_OK, KC_ERR_NO_DEVICE, KC_ERR_INVALID_ARG, KC_ERR_UNSUPPORTED = 0, 101, 102, 104
BC7, BC_SRGB, MIP_PER_LEVEL = 98, 1, 2
SIZES = [(1, 1), (1, 5), (5, 1), (64, 64), (130, 70), (4096, 64), (4096, 4096)]  # (w, h): test_mip_host.py's
PNGS = ["clouds.png", "image_1.png", "heart_256.png", "image_2.png", "heart_110.png"]


def hexb(a):
    return np.asarray(a, np.uint8).tobytes().hex(" ")


def rgba_of(name):
    """A golden input as the RGBA8 bytes kc_image_to_u8 writes for it: Gray is (v, v, v, 255), RGB gets alpha 255"""
    a = read_png(os.path.join(INPUTS, name))
    if a.shape[2] < 3:
        a = np.repeat(a[..., :1], 3, -1)
    if a.shape[2] == 3:
        a = np.concatenate([a, np.full(a.shape[:2] + (1,), 255, a.dtype)], -1)
    return a


@pytest.fixture(scope="module")
def png_detail():
    """name -> (rgba8, texels (n, 16, 4), bc7_ref's detail): computed once, read by several tests, never changed"""
    out = {}
    for name in PNGS:
        a = rgba_of(name)
        t = bc_ref.blocks(a).reshape(-1, 16, 4)
        out[name] = (a, t, bc7_ref.encode_detail(t))
    return out


@pytest.fixture(scope="module")
def random_detail():
    t = random_blocks(1500, 7)
    return t, bc7_ref.encode_detail(t)


# ------------------------------------------------------------------ worked blocks
def uniform_block():
    return np.tile(np.array([128, 64, 32, 255]), (16, 1))


def two_colour_block():  # test_bc_host.py's, opaque
    return np.array([(255, 0, 0, 255) if t % 4 < 2 else (0, 255, 0, 255) for t in range(16)])


def alpha_ramp_block():
    return np.stack([np.full(16, 200), np.full(16, 100), np.full(16, 50), 17 * np.arange(16)], -1)


def bright_first_block():  # texel 0 sits on e1, so its index 15 forces the anchor swap
    return np.stack([255 - 17 * np.arange(16)] * 3 + [np.full(16, 255)], -1)


@pytest.mark.parametrize("block,want,mode,err", [
    # every endpoint is (128, 64, 32, 255): one odd channel, p-bit 0, so alpha decodes to 254; mode 5's error is 16 too (no less)
    (uniform_block, "40 20 10 04 82 40 fe 7f 00 00 00 00 00 00 00 00", 6, 16),
    # mode 5 holds both colours exactly (q = 0 and 127); texel 0 is on e1 = (255, 0, 0), so the colour set is swapped
    (two_colour_block, "20 7f 00 e0 0f 00 fc ff e3 e1 e1 e1 01 00 00 00", 5, 0),
    # constant colour, alpha 0, 17, .., 255: mode 6's sixteen weights follow the ramp, mode 5's four do not (8696)
    (alpha_ramp_block, "40 32 59 26 cb 64 00 7f 10 32 54 76 98 ba dc fe", 6, 32),
    (bright_first_block, "c0 3f e0 0f f8 03 fe ff 10 32 54 76 98 ba dc fe", 6, 80)])
def test_worked_blocks(block, want, mode, err):
    p = block()
    d = bc7_ref.encode_detail(p[None])
    assert hexb(d["blocks"][0]) == want
    assert (d["mode"][0], d["err"][0]) == (mode, err)
    assert ((bc7_ref.decode_blocks(d["blocks"])[0] - p) ** 2).sum() == err


def test_worked_blocks_take_the_branches_they_stand_for():
    d = bc7_ref.encode_detail(np.stack([uniform_block(), two_colour_block(), alpha_ramp_block(), bright_first_block()]))
    assert list(d["err5"]) == [16, 0, 8696, 26040] and list(d["err6"]) == [16, 32, 32, 80]
    assert list(d["swap5c"][:2]) == [False, True]
    assert [bool(d["swap6"][k]) for k in (0, 2, 3)] == [False, False, True]  # the blocks that mode 6 was chosen for
    f = bc7_ref.fields(d["blocks"])
    assert list(f["p"][3]) == [1, 0]  # (255, 255, 255, 255) takes the p-bit, and after the swap it is endpoint 0
    assert list(f["idx"][3]) == list(range(16)) and list(f["idx"][2]) == list(range(16))


# ------------------------------------------------------------------ layout properties on random blocks
def test_layout_of_random_blocks(random_detail):
    t, d = random_detail
    blk = d["blocks"]
    f = bc7_ref.fields(blk)
    low7 = blk[:, 0] & 0x7f
    assert (((low7 == 64) & (d["mode"] == 6)) | (((blk[:, 0] & 0x3f) == 32) & (d["mode"] == 5))).all()  # exactly one pattern
    assert (f["mode"] == d["mode"]).all()
    assert (f["rot"] == 0).all()
    is6 = f["mode"] == 6
    assert (f["idx"][is6, 0] < 8).all()
    assert (f["idx"][~is6, 0] < 2).all() and (f["idx_a"][~is6, 0] < 2).all()
    dec = bc7_ref.decode_blocks(blk)
    assert (((dec - t) ** 2).sum((1, 2)) == d["err"]).all()
    assert (d["err"] == np.minimum(d["err5"], d["err6"])).all() and ((d["mode"] == 5) == (d["err5"] < d["err6"])).all()


def test_every_chosen_index_is_nearest(random_detail):
    t, d = random_detail
    f = bc7_ref.fields(d["blocks"])
    ep = f["ep"]  # (n, 2, 4) as the decoder sees them
    for mode, w, sets in ((6, bc7_ref.W4, [(slice(0, 4), "idx")]), (5, bc7_ref.W2, [(slice(0, 3), "idx"), (slice(3, 4), "idx_a")])):
        m = f["mode"] == mode
        for ch, key in sets:
            pal = bc7_ref.interp(ep[m, 0, None, ch], ep[m, 1, None, ch], w[None, :, None])  # (n, m, C)
            dist = ((t[m][:, :, None, ch] - pal[:, None, :, :]) ** 2).sum(-1)  # (n, 16, m)
            chosen = np.take_along_axis(dist, f[key][m][..., None], -1)[..., 0]
            assert (chosen == dist.min(-1)).all(), (mode, key)


def test_the_inputs_cover_every_branch(random_detail, png_detail):
    parts = [random_detail[1]] + [png_detail[n][2] for n in PNGS]
    d = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    f = bc7_ref.fields(d["blocks"])
    m6, m5 = d["mode"] == 6, d["mode"] == 5
    assert m6.sum() >= 100 and m5.sum() >= 100
    pairs = set(map(tuple, f["p"][m6]))
    assert pairs == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for m, key in ((m6, "swap6"), (m5, "swap5c"), (m5, "swap5a")):
        assert d[key][m].any() and not d[key][m].all(), key


# ------------------------------------------------------------------ Pillow's decoder
def dx10_header(w, h, dxgi, levels=1):
    mips = levels > 1
    out = b"DDS " + struct.pack("<7I", 124, 0x81007 | (0x20000 if mips else 0), h, w, ((w + 3) // 4) * ((h + 3) // 4) * 16, 0, levels)
    out += struct.pack("<11I", *[0] * 11)
    out += struct.pack("<2I4s5I", 32, 0x4, b"DX10", 0, 0, 0, 0, 0)
    out += struct.pack("<5I", 0x1000 | ((0x8 | 0x400000) if mips else 0), 0, 0, 0, 0)
    out += struct.pack("<5I", dxgi, 3, 0, 1, 0)
    assert len(out) == 148
    return out


def pillow_decode(header, blocks):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(header + np.ascontiguousarray(blocks).tobytes())).convert("RGBA"))


@pytest.mark.parametrize("name", PNGS + ["random"])
def test_pillow_decodes_what_the_reference_decodes(name, png_detail):
    pytest.importorskip("PIL")
    if name == "random":
        rng = np.random.default_rng(11)
        a = np.concatenate([rng.integers(0, 256, size=(37, 53, 4)), 100 + rng.integers(0, 12, size=(37, 53, 4))]).astype(np.uint8)
        blk = bc7_ref.encode(a)
    else:
        a = png_detail[name][0]
        blk = png_detail[name][2]["blocks"].reshape((a.shape[0] + 3) // 4, (a.shape[1] + 3) // 4, 16)
    h, w = a.shape[:2]
    want = bc7_ref.decode(blk, h, w)
    assert np.array_equal(pillow_decode(dx10_header(w, h, 98), blk), want)
    from kanter_core_amd import api
    assert api.dds_header(w, h, BC7, levels=1) == dx10_header(w, h, 98)
    assert np.array_equal(pillow_decode(api.dds_header(w, h, BC7, levels=1), blk), want)


# ------------------------------------------------------------------ quality against the project's older encoders
@pytest.mark.parametrize("name,psnr7,psnr1,err7,err3", [
    ("clouds.png", 59.74, 43.19, 46039, 612852), ("image_1.png", 50.72, 47.47, 108224, 228836),
    ("heart_256.png", 39.93, 35.15, 1328937, 3907725), ("image_2.png", 30.65, 29.74, 11152404, 13659126),
    ("heart_110.png", 32.24, 29.29, 1437603, 2837679)])
def test_quality_against_bc1_and_bc3(name, psnr7, psnr1, err7, err3, png_detail):
    a, t, d = png_detail[name]
    h, w = a.shape[:2]
    by, bx = (h + 3) // 4, (w + 3) // 4
    dec = bc7_ref.decode_blocks(d["blocks"])  # (n, 16, 4)
    pix = bc7_ref.unblock(dec.reshape(by, bx, 16, 4), h, w)
    got7 = 10 * np.log10(255.0 ** 2 / ((pix[..., :3] - a[..., :3].astype(np.int64)) ** 2).mean())
    got1 = bc_ref.psnr_bc1(a)
    bc3 = bc_ref.encode(a, 3).reshape(-1, 16)
    dec3 = np.concatenate([bc_ref.decode_bc1(bc3[:, 8:]), bc_ref.decode_bc4(bc3[:, :8])[..., None]], -1)
    e7, e3 = ((dec - t) ** 2).sum(), ((dec3 - t) ** 2).sum()
    assert e7 == d["err"].sum()
    assert e7 < e3, (e7, e3)  # four channels, over the blocks
    if name != "heart_110.png":
        assert got7 > got1, (got7, got1)
    assert (round(got7, 2), round(got1, 2), e7, e3) == (psnr7, psnr1, err7, err3)


# ------------------------------------------------------------------ the C ABI without a device
@pytest.fixture(scope="module")
def L():
    from kanter_core_amd import _lib
    return _lib.load()


def test_enum_value_through_c(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    src = tmp_path / "bc7.c"
    src.write_text('#include <stdio.h>\n#include "kanter_core_amd.h"\nint main(void) { printf("%d %d\\n", (int)KC_BC7, (int)KC_BC5); return 0; }\n')
    exe = tmp_path / "bc7"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["98", "5"]
    from kanter_core_amd import api
    import kanter_core_amd as kc
    assert api.BC7 == 98 and kc.BC7 == 98 and api.BC_BLOCK_BYTES[98] == 16
    assert api._bc_format("bc7") == 98 and api._bc_format(98) == 98
    with pytest.raises(ValueError):
        api._bc_format(7)


def validate(L, desc):
    ext = C.c_size_t(12345)
    return L.kc_bc_image_validate(C.byref(desc), C.byref(ext)), ext.value


def test_validate_extents_and_alignment(L):
    import torch
    from kanter_core_amd import _lib
    D = _lib.kc_bc_image
    base = 1 << 20
    gpu = torch.cuda.is_available()
    for d, ext in ((D(base, 1, 1, BC7, 16), 16), (D(base, 5, 3, BC7, 32), 32), (D(base, 13, 9, BC7, 64), 2 * 64 + 64),
                   (D(base, 1 << 16, 1 << 17, BC7, 1 << 18), ((1 << 15) - 1) * (1 << 18) + (1 << 18))):
        status, got = validate(L, d)
        assert got == ext
        if not gpu:  # the not-gpu suite also runs on a machine with a device, which may or may not be initialised
            assert status == KC_ERR_NO_DEVICE
    for d in (D(base + 8, 8, 8, BC7, 32),    # pointer not a multiple of the 16-byte blocks
              D(base, 8, 8, BC7, 40),        # pitch not a multiple of them
              D(base, 8, 8, BC7, 16),        # pitch below bx * 16
              D(base, 0, 8, BC7, 32), D(None, 8, 8, BC7, 32),
              D(base, 8, 8, 7, 32), D(base, 8, 8, 97, 32), D(base, 8, 8, 99, 32)):  # 7 is still not a format; nor are 98's neighbours
        assert validate(L, d)[0] == KC_ERR_INVALID_ARG, (d.format, d.width, d.row_pitch_bytes)


@pytest.mark.parametrize("w,h", SIZES)
def test_mip_layout(L, w, h):
    n, total = C.c_uint32(), C.c_size_t()
    levels = 1 + int(np.floor(np.log2(max(w, h))))
    offs = (C.c_size_t * levels)()
    assert L.kc_bc_mip_layout(w, h, BC7, C.byref(n), offs, levels, C.byref(total)) == KC_OK
    sizes = [((max(1, w >> k) + 3) // 4) * ((max(1, h >> k) + 3) // 4) * 16 for k in range(levels)]
    assert n.value == levels and list(offs) == [sum(sizes[:k]) for k in range(levels)] and total.value == sum(sizes)
    assert L.kc_bc_mip_layout(w, h, 7, C.byref(n), offs, levels, C.byref(total)) == KC_ERR_INVALID_ARG
    from kanter_core_amd import api
    assert api.bc_mip_layout(w, h, "bc7") == (list(offs), sum(sizes))


@pytest.mark.parametrize("w,h,flags,levels,dxgi", [(130, 70, 0, 8, 98), (130, 70, BC_SRGB, 8, 99), (64, 64, 0, 1, 98), (5, 3, BC_SRGB, 2, 99)])
def test_dds_header(L, w, h, flags, levels, dxgi):
    out, n = (C.c_uint8 * 148)(), C.c_size_t()
    assert L.kc_dds_header(w, h, BC7, flags, levels, out, C.byref(n)) == KC_OK and n.value == 148
    assert bytes(out) == dx10_header(w, h, dxgi, levels)
    assert L.kc_dds_header(w, h, 7, flags, levels, out, C.byref(n)) == KC_ERR_INVALID_ARG


def test_srgb_is_accepted_where_bc4_and_bc5_are_refused(L, tmp_path):
    from kanter_core_amd import _lib
    img = C.c_void_p(1 << 20)  # never looked at: every call below returns before it would be
    buf = (C.c_uint8 * 64)()
    path = str(tmp_path / "x.dds").encode()
    out = (C.c_uint8 * 148)()
    d = {f: _lib.kc_bc_image(1 << 20, 8, 8, f, 32) for f in (4, 5, BC7)}
    for f in (4, 5):
        assert L.kc_dds_header(8, 8, f, BC_SRGB, 1, out, None) == KC_ERR_UNSUPPORTED
        assert L.kc_image_to_bc(img, f, BC_SRGB, buf, 64) == KC_ERR_UNSUPPORTED
        assert L.kc_image_to_bc_device(img, C.byref(d[f]), BC_SRGB, None) == KC_ERR_UNSUPPORTED
        assert L.kc_image_to_bc_mips(img, f, BC_SRGB, buf, 64) == KC_ERR_UNSUPPORTED
        assert L.kc_image_write_dds(img, path, f, BC_SRGB, 1) == KC_ERR_UNSUPPORTED
    # BC7 passes the flag check: the next check refuses (a NULL argument), and unknown bits are still unsupported
    assert L.kc_dds_header(8, 8, BC7, BC_SRGB, 1, out, None) == KC_OK
    assert L.kc_image_to_bc(img, BC7, BC_SRGB, None, 64) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_device(None, C.byref(d[BC7]), BC_SRGB, None) in (KC_ERR_INVALID_ARG, KC_ERR_NO_DEVICE)
    assert L.kc_image_to_bc_mips(img, BC7, BC_SRGB | MIP_PER_LEVEL, None, 64) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc_mips_device(img, BC7, BC_SRGB, None, 64, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_write_dds(img, None, BC7, BC_SRGB, 1) == KC_ERR_INVALID_ARG
    assert L.kc_live_graph_buffer_bc_mips(None, 0, 0, BC7, BC_SRGB, buf, 64, None) == KC_ERR_INVALID_ARG
    assert L.kc_image_to_bc(img, BC7, 4, buf, 64) == KC_ERR_UNSUPPORTED
    assert L.kc_dds_header(8, 8, BC7, 4, 1, out, None) == KC_ERR_UNSUPPORTED
