// Block compression: kc_bc_image_validate, kc_image_to_bc, kc_image_to_bc_device (include/kanter_core_amd.h).  The host side
// checks the arguments and the caller's descriptor -- arithmetic first, then that its bytes lie in one allocation of the
// library's device -- and launches bc.hip's encoder (KC_BC7: bc7.hip's, KC_BC6H: bc6h.hip's) once per call: on the library's stream, ordered
// against the caller's stream by the two event edges of kc_image_to_device, or into pool staging that is copied to the
// caller's host memory.  The file also holds what the whole BC family's host side shares (bc_decode.cpp, the BC chain of mip_export.cpp):
// the format table, the block count and level bytes, the flag rule and the choice of a format's device unit.
#include "kc_runtime.hpp"

namespace kc {

// What a format is, for the whole host side (kc_runtime.hpp has the fields).  BC6H's blocks are written to .dds and not read back.
static const BcFormat kBcFormats[] = {
    // format  bytes  channels  planes  srgb   counts  dxgi  dxgi_srgb  dds_read  fourcc
    { KC_BC1,  8,     0x7u,     4,      true,  false,  71,   72,        true,     { fourcc('D', 'X', 'T', '1'), 0 } },
    { KC_BC3,  16,    0xfu,     4,      true,  false,  77,   78,        true,     { fourcc('D', 'X', 'T', '5'), 0 } },
    { KC_BC4,  8,     0x1u,     1,      false, false,  80,   0,         true,     { fourcc('A', 'T', 'I', '1'), fourcc('B', 'C', '4', 'U') } },
    { KC_BC5,  16,    0x3u,     2,      false, false,  83,   0,         true,     { fourcc('A', 'T', 'I', '2'), fourcc('B', 'C', '5', 'U') } },
    { KC_BC6H, 16,    0x7u,     3,      false, true,   95,   0,         false,    { 0, 0 } },
    { KC_BC7,  16,    0xfu,     4,      true,  true,   98,   99,        true,     { 0, 0 } },
};

const BcFormat *bc_format(int format)
{
    for (const BcFormat &f : kBcFormats)
        if (f.format == format) return &f;
    return nullptr;
}

const BcFormat *bc_format_of_dds(uint32_t dxgi, uint32_t cc, uint32_t *flags)
{
    for (const BcFormat &f : kBcFormats) {
        if (!f.dds_read) continue;
        const bool srgb = dxgi != 0 && dxgi == f.dxgi_srgb;
        if (srgb || (dxgi != 0 && dxgi == f.dxgi) || (cc != 0 && (cc == f.fourcc[0] || cc == f.fourcc[1]))) {
            *flags = srgb ? KC_BC_SRGB : 0u;
            return &f;
        }
    }
    return nullptr;
}

size_t bc_block_bytes(int format)
{
    const BcFormat *f = bc_format(format);
    return f ? f->block_bytes : 0;
}

size_t bc_level_bytes(uint32_t w, uint32_t h, const BcFormat &f) { return (((size_t)w + 3) / 4) * (((size_t)h + 3) / 4) * f.block_bytes; }

int bc_block_count(uint32_t w, uint32_t h, const char *who, uint64_t *bx, uint64_t *by)
{
    *bx = ((uint64_t)w + 3) / 4;
    *by = ((uint64_t)h + 3) / 4;
    // the kernels' block index is 32-bit, with room for the grid-stride step
    if (*bx * *by > (1ull << 31)) {
        set_error(std::string(who) + ": image too large: more than 2^31 blocks");
        return KC_ERR_INVALID_ARG;
    }
    return KC_OK;
}

static int bc_refuse(const char *what)
{
    set_error(std::string("kc_bc_image: ") + what);
    return KC_ERR_INVALID_ARG;
}

int bc_check_flags(int format, uint32_t flags, uint32_t allowed, const char *who)
{
    if (flags & ~allowed) {
        set_error(std::string(who) + ": unknown flag bits");
        return KC_ERR_UNSUPPORTED;
    }
    const BcFormat *f = bc_format(format);
    // KC_BC_ALL_MODES, where an entry point allows it, goes with every format: a caller who reads arbitrary files can always pass it
    if ((flags & KC_BC_SRGB) && f && !f->srgb) {
        set_error(std::string(who) + ": KC_BC_SRGB is for BC1, BC3 and BC7 only");
        return KC_ERR_UNSUPPORTED;
    }
    // KC_BC_PUNCH_THROUGH, where an entry point allows it: BC1 only, with its reference byte, and not for vectors.  The byte of
    // bits 24-31 belongs to this flag and to KC_MIP_COVERAGE, together or alone; without either it is refused.
    if (allowed & KC_BC_PUNCH_THROUGH) {
        const uint32_t ref = flags >> 24;
        if ((flags & KC_BC_PUNCH_THROUGH) && f && f->format != KC_BC1) {
            set_error(std::string(who) + ": KC_BC_PUNCH_THROUGH is for BC1 only");
            return KC_ERR_UNSUPPORTED;
        }
        if ((flags & (KC_BC_PUNCH_THROUGH | KC_MIP_COVERAGE)) ? ref == 0 : ref != 0) {
            set_error(std::string(who) + ": KC_BC_PUNCH_THROUGH and KC_MIP_COVERAGE go with a reference byte 1..255 in bits 24-31, which goes with one of them");
            return KC_ERR_UNSUPPORTED;
        }
        if ((flags & KC_BC_PUNCH_THROUGH) && (flags & KC_MIP_NORMALS)) {
            set_error(std::string(who) + ": KC_BC_PUNCH_THROUGH with KC_MIP_NORMALS");
            return KC_ERR_UNSUPPORTED;
        }
    }
    return KC_OK;
}

// kc_bc1_punch_through_block: the rule of the header on one block, in plain integers
void bc1_punch_through_block(const uint8_t rgba[64], uint32_t ref, uint8_t block[8])
{
    auto pack = [](const int *p) {
        return (uint32_t)((31 * p[0] + 127) / 255) << 11 | (uint32_t)((63 * p[1] + 127) / 255) << 5 | (uint32_t)((31 * p[2] + 127) / 255);
    };
    auto expand = [](uint32_t c, int *e) {
        const int r5 = (int)(c >> 11), g6 = (int)((c >> 5) & 63u), b5 = (int)(c & 31u);
        e[0] = (r5 << 3) | (r5 >> 2);
        e[1] = (g6 << 2) | (g6 >> 4);
        e[2] = (b5 << 3) | (b5 >> 2);
    };
    int n = 0, lo[3] = { 255, 255, 255 }, hi[3] = { 0, 0, 0 };
    bool opaque[16];
    for (int t = 0; t < 16; ++t) {
        opaque[t] = rgba[4 * t + 3] >= ref;
        if (!opaque[t]) continue;
        ++n;
        for (int c = 0; c < 3; ++c) {
            lo[c] = std::min(lo[c], (int)rgba[4 * t + c]);
            hi[c] = std::max(hi[c], (int)rgba[4 * t + c]);
        }
    }
    uint32_t c0 = 0, c1 = 0, word = 0xffffffffu;
    if (n > 0) {
        const bool three = n < 16;
        int k = 0;
        for (int c = 1; c < 3; ++c)
            if (hi[c] - lo[c] > hi[k] - lo[k]) k = c;  // ties: R, then G, then B
        long long s[3] = { 0, 0, 0 };
        for (int t = 0; t < 16; ++t) {
            if (!opaque[t]) continue;
            const int a = 2 * rgba[4 * t + k] - lo[k] - hi[k];
            for (int c = 0; c < 3; ++c) s[c] += (long long)a * (2 * rgba[4 * t + c] - lo[c] - hi[c]);
        }
        int ea[3], eb[3];
        for (int c = 0; c < 3; ++c) {
            const int m = (hi[c] - lo[c]) >> (three ? 3 : 4);
            const int a = hi[c] - m, b = lo[c] + m;
            ea[c] = s[c] < 0 ? b : a;
            eb[c] = s[c] < 0 ? a : b;
        }
        c0 = pack(ea);
        c1 = pack(eb);
        if (three ? c0 > c1 : c0 < c1) std::swap(c0, c1);
        int q[4][3];
        expand(c0, q[0]);
        expand(c1, q[1]);
        for (int c = 0; c < 3; ++c) {
            q[2][c] = three ? (q[0][c] + q[1][c]) / 2 : 2 * q[0][c] + q[1][c];
            q[3][c] = q[0][c] + 2 * q[1][c];
            if (!three) q[0][c] *= 3, q[1][c] *= 3;  // the four-colour palette, scaled by 3
        }
        word = 0;
        for (int t = 0; t < 16; ++t) {
            uint32_t best_j = 3;
            if (opaque[t] && c0 == c1) best_j = 0;
            else if (opaque[t]) {
                long long best = -1;
                for (int j = 0; j < (three ? 3 : 4); ++j) {
                    long long d = 0;
                    for (int c = 0; c < 3; ++c) {
                        const long long x = (three ? 1 : 3) * (int)rgba[4 * t + c] - q[j][c];
                        d += x * x;
                    }
                    if (best < 0 || d < best) best = d, best_j = (uint32_t)j;
                }
            }
            word |= best_j << (2 * t);
        }
    }
    const uint32_t w0 = c0 | (c1 << 16);
    for (int i = 0; i < 4; ++i) {
        block[i] = (uint8_t)(w0 >> (8 * i));
        block[4 + i] = (uint8_t)(word >> (8 * i));
    }
}

// The arithmetic half of the validation: needs no device.
static int bc_check_arith(const kc_bc_image *d, size_t *extent)
{
    if (!d) return bc_refuse("descriptor is NULL");
    const size_t bb = bc_block_bytes(d->format);
    if (bb == 0) return bc_refuse("unknown format");
    if (!d->ptr || d->width == 0 || d->height == 0) return bc_refuse("NULL pointer or zero extent");
    uint64_t bx = 0, by = 0;
    KC_TRY(bc_block_count(d->width, d->height, "kc_bc_image", &bx, &by));
    if ((uintptr_t)d->ptr % bb || d->row_pitch_bytes % bb) return bc_refuse("pointer and row pitch must be multiples of the block bytes");
    size_t row_bytes = 0, last = 0, ext = 0;
    if (__builtin_mul_overflow((size_t)bx, bb, &row_bytes)) return bc_refuse("extent overflows");
    if (d->row_pitch_bytes < row_bytes) return bc_refuse("row pitch < blocks per row * block bytes");
    if (__builtin_mul_overflow((size_t)(by - 1), d->row_pitch_bytes, &last) || __builtin_add_overflow(last, row_bytes, &ext))
        return bc_refuse("extent overflows");
    if ((uintptr_t)d->ptr + ext < (uintptr_t)d->ptr) return bc_refuse("extent overflows");
    *extent = ext;
    return KC_OK;
}

int bc_image_validate(const kc_bc_image *d, size_t *extent_bytes)
{
    size_t ext = 0;
    KC_TRY(bc_check_arith(d, &ext));
    if (extent_bytes) *extent_bytes = ext;
    return device_extent_check(d->ptr, ext, "kc_bc_image");
}

// ---------------------------------------------------------------- the device unit of a format
// BC6H's three kernels are bc6h.hip's, BC7's encoder bc7.hip's; everything else is bc.hip's and bc_decode.hip's.  all_modes
// (KC_BC_ALL_MODES): the formats with modes that the default decoders leave out -- the table's counts_undecoded, BC7 and BC6H --
// go to bc_modes.hip, which leaves none out and therefore takes no count; for the other formats the flag changes nothing
hipError_t bc_launch_encode(int format, bool srgb, const Operand op[4], int gray, char *dst, uint64_t row_pitch, uint32_t w, uint32_t h,
                            uint32_t nt_mask, hipStream_t s, uint32_t pt_ref)
{
    if (pt_ref) return format == KC_BC1 && !gray ? launch_bc1a_encode(srgb ? 1 : 0, op, pt_ref, dst, row_pitch, w, h, nt_mask, s) : hipErrorInvalidValue;
    if (format == KC_BC6H) return launch_bc6h_encode(op, gray, dst, row_pitch, w, h, nt_mask, s);
    if (format == KC_BC7) return launch_bc7_encode(srgb ? 1 : 0, op, gray, dst, row_pitch, w, h, nt_mask, s);
    return launch_bc_encode(format, srgb ? 1 : 0, op, gray, dst, row_pitch, w, h, nt_mask, s);
}

hipError_t bc_launch_decode(int format, bool all_modes, const BcDecodeArgs &a, bool count, uint32_t nt_mask, uint32_t groups, hipStream_t s)
{
    const BcFormat *f = bc_format(format);
    if (all_modes && f && f->counts_undecoded) return count ? hipErrorInvalidValue : launch_bc_modes_decode(format, a, nt_mask, groups, s);
    if (format == KC_BC6H) return launch_bc6h_decode(a, count, nt_mask, groups, s);
    return launch_bc_decode(format, a, count, nt_mask, groups, s);
}

hipError_t bc_launch_compare(int format, bool srgb, bool all_modes, const Operand op[4], int gray, const char *blocks, uint64_t row_pitch, uint32_t w,
                             uint32_t h, uint32_t nt_mask, uint32_t groups, unsigned long long *partials, unsigned long long *result, hipStream_t s,
                             uint32_t pt_ref)
{
    if (pt_ref)
        return format == KC_BC1 && !gray ? launch_bc1a_compare(srgb ? 1 : 0, op, pt_ref, blocks, row_pitch, w, h, nt_mask, groups, partials, result, s)
                                         : hipErrorInvalidValue;
    const BcFormat *f = bc_format(format);
    if (all_modes && f && f->counts_undecoded)
        return launch_bc_modes_compare(format, srgb ? 1 : 0, op, gray, blocks, row_pitch, w, h, nt_mask, groups, partials, result, s);
    if (format == KC_BC6H) return launch_bc6h_compare(op, gray, blocks, row_pitch, w, h, nt_mask, groups, partials, result, s);
    return launch_bc_compare(format, srgb ? 1 : 0, op, gray, blocks, row_pitch, w, h, nt_mask, groups, partials, result, s);
}

// One launch of the encoder for `img` (forced already) into `dst`, block rows `row_pitch` bytes apart.  The channels the format
// reads come from the image as to_u8 sees it (Gray: (v, v, v, 1)); constants cost no loads.  KC_BC6H reads R, G and B.
// pt_ref != 0: KC_BC_PUNCH_THROUGH with that reference byte (BC1 of an RGBA image: the callers have refused the rest), which
// reads alpha too.
int bc_encode(kc_image *img, int format, bool srgb, char *dst, size_t row_pitch, hipStream_t s, uint32_t pt_ref)
{
    Context &c = ctx();
    const BcFormat &f = *bc_format(format);  // the entry points have refused an unknown format
    Operand o[4];
    const uint32_t n_res = image_source_operands(img, pt_ref ? 0xfu : f.channels, o);
    const uint32_t w = img->w(), h = img->h();
    const uint64_t in_bytes = (uint64_t)w * h * 4 * n_res, out_bytes = bc_level_bytes(w, h, f);
    const uint32_t nt_mask = cache_policy_mask(in_bytes, out_bytes, n_res ? n_res : 1);
    hipError_t e = bc_launch_encode(format, srgb, o, img->is_rgba() ? 0 : 1, dst, row_pitch, w, h, nt_mask, s, pt_ref);
    if (e != hipSuccess) return hip_fail(e, "launch_bc_encode");
    c.launches++;
    c.alg_bytes += in_bytes + out_bytes;
    return KC_OK;
}

int image_to_bc(kc_image *img, int format, uint32_t flags, uint8_t *host, size_t host_bytes)
{
    KC_TRY(bc_check_flags(format, flags, KC_BC_SRGB | kBcPunchThroughBits, "kc_image_to_bc"));
    const BcFormat *f = bc_format(format);
    if (!f) return bc_refuse("unknown format");
    if (!img || !host) return bc_refuse("NULL image or host buffer");
    KC_TRY(need_init());
    if ((flags & KC_BC_PUNCH_THROUGH) && !img->is_rgba()) return bc_refuse("KC_BC_PUNCH_THROUGH is for RGBA images");
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    uint64_t bx = 0, by = 0;
    KC_TRY(bc_block_count(img->w(), img->h(), "kc_bc_image", &bx, &by));
    const size_t nbytes = bc_level_bytes(img->w(), img->h(), *f);
    if (host_bytes < nbytes) return bc_refuse("host_bytes < blocks * block bytes");
    KC_TRY(image_force(img));  // a pending fused chain runs first
    PoolStaging staging;
    KC_TRY(staging.alloc(nbytes));
    KC_TRY(bc_encode(img, format, (flags & KC_BC_SRGB) != 0, (char *)staging.ptr, (size_t)bx * f->block_bytes, c.stream, bc_punch_through_ref(flags)));
    hipError_t e = hipMemcpyAsync(host, staging.ptr, nbytes, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) return hip_fail(e, "image_to_bc");
    return KC_OK;
}

int image_to_bc_device(kc_image *img, const kc_bc_image *dst, uint32_t flags, void *hip_stream)
{
    KC_TRY(bc_check_flags(dst ? dst->format : 0, flags, KC_BC_SRGB | kBcPunchThroughBits, "kc_image_to_bc_device"));
    KC_TRY(bc_image_validate(dst, nullptr));
    if (!img) return bc_refuse("image is NULL");
    if ((flags & KC_BC_PUNCH_THROUGH) && !img->is_rgba()) return bc_refuse("KC_BC_PUNCH_THROUGH is for RGBA images");
    if (img->w() != dst->width || img->h() != dst->height) return bc_refuse("descriptor size differs from the image's");
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    KC_TRY(image_force(img));  // a pending fused chain runs first
    return with_stream_edges(hip_stream, [&] {
        return bc_encode(img, dst->format, (flags & KC_BC_SRGB) != 0, (char *)dst->ptr, dst->row_pitch_bytes, c.stream, bc_punch_through_ref(flags));
    });
}

}  // namespace kc
