// Block decode, the error of an encoding and .dds input: kc_image_from_bc, kc_image_from_bc_device, kc_image_bc_compare,
// kc_image_bc_error, kc_dds_parse, kc_image_read_dds (include/kanter_core_amd.h).  The host side checks the arguments in the
// header's order, allocates the planes a format holds (constant planes for the channels it does not), and launches
// bc_decode.hip's kernels on the library's stream: ordered against the caller's stream by the two event edges of
// kc_image_to_bc_device, or after an upload into pool staging.  The counts and the error record come back through the
// context's StatsBuffers (stats.cpp): pinned host memory and an event of the call's own.  The .dds parser is arithmetic on
// bytes, with no device call.
#include <cstdio>

#include "kc_runtime.hpp"

namespace kc {

static int bcd_refuse(const char *who, const char *what)
{
    set_error(std::string(who) + ": " + what);
    return KC_ERR_INVALID_ARG;
}

// Flag bits other than KC_BC_GRAY and KC_BC_ALL_MODES, or KC_BC_GRAY with a format other than BC4, are KC_ERR_UNSUPPORTED
static int bcd_check_flags(int format, uint32_t flags, const char *who)
{
    if (flags & ~(uint32_t)(KC_BC_GRAY | KC_BC_ALL_MODES)) {
        set_error(std::string(who) + ": flags other than KC_BC_GRAY and KC_BC_ALL_MODES (no transfer function is applied on decode)");
        return KC_ERR_UNSUPPORTED;
    }
    const BcFormat *f = bc_format(format);
    if ((flags & KC_BC_GRAY) && !(f && f->planes == 1)) {  // a Gray image is one plane: BC4
        set_error(std::string(who) + ": KC_BC_GRAY is for BC4 only");
        return KC_ERR_UNSUPPORTED;
    }
    return KC_OK;
}

// One launch of the decoder (two with a count) on the library's stream: the blocks at `src`, block rows `row_pitch` bytes apart,
// into a new image.  *counted: the count is in flight and stats_fetch brings it.  KC_BC_ALL_MODES in `flags`: every block is
// decoded, so nothing is counted and the caller's count is 0 without a wait.
static int bc_decode(const char *src, size_t row_pitch, uint32_t w, uint32_t h, int format, uint32_t flags, bool want_count, kc_image **out,
                     bool *counted)
{
    const bool gray = (flags & KC_BC_GRAY) != 0, all_modes = (flags & KC_BC_ALL_MODES) != 0;
    Context &c = ctx();
    const BcFormat &f = *bc_format(format);  // the entry points have refused an unknown format
    const int n_res = f.planes, n = gray ? 1 : 4;
    kc_plane *p[4];
    float *dp[4];
    int s = image_planes_for_import(w, h, n_res, n, p, dp);  // the sampling convention: missing G, B = 0, A = 1
    const bool count = want_count && f.counts_undecoded && !all_modes;
    BcDecodeArgs a{};
    uint32_t groups = 0;
    if (s == KC_OK) {
        a.src = src;
        a.row_pitch = row_pitch;
        a.w = w;
        a.h = h;
        a.bx = (w + 3) / 4;
        a.by = (h + 3) / 4;
        a.dst_pitch = (uint32_t)(p[0]->pitch / sizeof(float));
        for (int i = 0; i < n_res; ++i) a.dst[i] = dp[i];
        groups = bc_decode_groups(w, h, count);
        if (count) {
            s = stats_buffers((size_t)groups * sizeof(unsigned long long));
            a.partials = (unsigned long long *)c.stats.partials;
            a.result = c.stats.result;
        }
    }
    if (s == KC_OK) {
        const uint64_t in_bytes = bc_level_bytes(w, h, f), out_bytes = (uint64_t)w * h * 4 * n_res;
        hipError_t e = bc_launch_decode(format, all_modes, a, count, cache_policy_mask(in_bytes, out_bytes, 1), groups, c.stream);
        if (e != hipSuccess) s = hip_fail(e, "launch_bc_decode");
        else {
            c.launches += count ? 2 : 1;
            c.alg_bytes += in_bytes + out_bytes;
        }
    }
    *counted = s == KC_OK && count;
    return image_of_import_planes(s, n, p, out);
}

int image_from_bc(const uint8_t *host, size_t host_bytes, uint32_t w, uint32_t h, int format, uint32_t flags, kc_image **out,
                  uint64_t *undecoded_blocks)
{
    KC_TRY(bcd_check_flags(format, flags, "kc_image_from_bc"));
    const BcFormat *f = bc_format(format);
    if (!f) return bcd_refuse("kc_image_from_bc", "unknown format");
    if (!host || !out) return bcd_refuse("kc_image_from_bc", "NULL host buffer or output");
    if (w == 0 || h == 0) return bcd_refuse("kc_image_from_bc", "zero extent");
    uint64_t bx = 0, by = 0;
    KC_TRY(bc_block_count(w, h, "kc_image_from_bc", &bx, &by));
    const size_t nbytes = bc_level_bytes(w, h, *f);
    if (host_bytes < nbytes) return bcd_refuse("kc_image_from_bc", "host_bytes < blocks * block bytes");
    KC_TRY(need_init());
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    PoolStaging staging;
    KC_TRY(staging.alloc(nbytes));
    kc_image *img = nullptr;
    bool counted = false;
    hipError_t e = hipMemcpyAsync(staging.ptr, host, nbytes, hipMemcpyHostToDevice, c.stream);
    int s = e == hipSuccess ? bc_decode((const char *)staging.ptr, (size_t)bx * f->block_bytes, w, h, format, flags,
                                        undecoded_blocks != nullptr, &img, &counted)
                            : KC_OK;
    if (s == KC_OK && e == hipSuccess && counted) s = stats_fetch(1);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);  // the caller's bytes have been read
    if (s == KC_OK && e != hipSuccess) s = hip_fail(e, "image_from_bc");
    if (s != KC_OK) {
        image_release(img);
        return s;
    }
    if (undecoded_blocks) *undecoded_blocks = counted ? c.stats.host[0] : 0;
    *out = img;
    return KC_OK;
}

int image_from_bc_device(const kc_bc_image *src, uint32_t flags, void *hip_stream, kc_image **out, uint64_t *undecoded_blocks)
{
    KC_TRY(bcd_check_flags(src ? src->format : 0, flags, "kc_image_from_bc_device"));
    if (!out) return bcd_refuse("kc_image_from_bc_device", "NULL output");
    KC_TRY(bc_image_validate(src, nullptr));
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    kc_image *img = nullptr;
    bool counted = false;
    int s = with_stream_edges(hip_stream, [&] {
        return bc_decode((const char *)src->ptr, src->row_pitch_bytes, src->width, src->height, src->format, flags,
                         undecoded_blocks != nullptr, &img, &counted);
    });
    if (s == KC_OK && counted) s = stats_fetch(1);
    if (s != KC_OK) {
        image_release(img);
        return s;
    }
    if (undecoded_blocks) *undecoded_blocks = counted ? c.stats.host[0] : 0;
    *out = img;
    return KC_OK;
}

// ---------------------------------------------------------------- the error of an encoding
// The comparison of `img` (forced already) with the blocks at `blocks`, block rows `row_pitch` bytes apart, on the library's
// stream; waits for the record.
static int bc_compare(kc_image *img, int format, uint32_t flags, const char *blocks, size_t row_pitch, kc_bc_error *out)
{
    Context &c = ctx();
    const BcFormat &f = *bc_format(format);  // the entry points have refused an unknown format
    const uint32_t pt_ref = bc_punch_through_ref(flags);  // KC_BC_PUNCH_THROUGH: alpha is read and compared too
    const uint32_t channels = pt_ref ? 0xfu : f.channels;
    Operand o[4];
    const uint32_t n_res = image_source_operands(img, channels, o);
    const uint32_t w = img->w(), h = img->h();
    const uint32_t groups = bc_compare_groups(w, h);
    KC_TRY(stats_buffers((size_t)groups * KC_BC_REC_WORDS * sizeof(unsigned long long)));
    const uint64_t in_bytes = (uint64_t)w * h * 4 * n_res;
    const uint64_t blk_bytes = bc_level_bytes(w, h, f);
    const uint32_t nt_mask = cache_policy_mask(in_bytes + blk_bytes, 0, n_res ? n_res : 1);
    unsigned long long *partials = (unsigned long long *)c.stats.partials;
    hipError_t e = bc_launch_compare(format, (flags & KC_BC_SRGB) != 0, (flags & KC_BC_ALL_MODES) != 0, o, img->is_rgba() ? 0 : 1, blocks, row_pitch, w, h, nt_mask, groups, partials,
                                     c.stats.result, c.stream, pt_ref);
    if (e != hipSuccess) return hip_fail(e, "launch_bc_compare");
    c.launches += 2;
    c.alg_bytes += in_bytes + blk_bytes;
    KC_TRY(stats_fetch(KC_BC_REC_WORDS));
    const unsigned long long *res = c.stats.host;
    kc_bc_error r;
    std::memset(&r, 0, sizeof r);
    r.format = format;
    r.flags = flags;
    r.channel_mask = channels;
    r.pixels = (uint64_t)w * h;
    for (int ch = 0; ch < 4; ++ch) {
        r.sse[ch] = res[ch];
        r.max_abs[ch] = (uint32_t)res[4 + ch];
    }
    r.undecoded_blocks = res[8];
    for (int k = 0; k < 8; ++k) r.bc7_mode_blocks[k] = res[9 + k];
    *out = r;
    return KC_OK;
}

int image_bc_compare(kc_image *img, const kc_bc_image *blocks, uint32_t flags, kc_bc_error *out)
{
    KC_TRY(bc_check_flags(blocks ? blocks->format : 0, flags, KC_BC_SRGB | KC_BC_ALL_MODES | kBcPunchThroughBits, "kc_image_bc_compare"));
    if (!img || !out) return bcd_refuse("kc_image_bc_compare", "NULL image or output");
    KC_TRY(bc_image_validate(blocks, nullptr));
    if ((flags & KC_BC_PUNCH_THROUGH) && !img->is_rgba()) return bcd_refuse("kc_image_bc_compare", "KC_BC_PUNCH_THROUGH is for RGBA images");
    if (img->w() != blocks->width || img->h() != blocks->height) return bcd_refuse("kc_image_bc_compare", "descriptor size differs from the image's");
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    KC_TRY(image_force(img));  // a pending fused chain runs first
    return bc_compare(img, blocks->format, flags, (const char *)blocks->ptr, blocks->row_pitch_bytes, out);
}

int image_bc_error(kc_image *img, int format, uint32_t flags, kc_bc_error *out)
{
    KC_TRY(bc_check_flags(format, flags, KC_BC_SRGB | kBcPunchThroughBits, "kc_image_bc_error"));
    const BcFormat *f = bc_format(format);
    if (!f) return bcd_refuse("kc_image_bc_error", "unknown format");
    if (!img || !out) return bcd_refuse("kc_image_bc_error", "NULL image or output");
    KC_TRY(need_init());
    if ((flags & KC_BC_PUNCH_THROUGH) && !img->is_rgba()) return bcd_refuse("kc_image_bc_error", "KC_BC_PUNCH_THROUGH is for RGBA images");
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    uint64_t bx = 0, by = 0;
    KC_TRY(bc_block_count(img->w(), img->h(), "kc_image_bc_error", &bx, &by));
    KC_TRY(image_force(img));  // a pending fused chain runs first
    PoolStaging staging;
    KC_TRY(staging.alloc(bc_level_bytes(img->w(), img->h(), *f)));
    const size_t row_pitch = (size_t)bx * f->block_bytes;
    KC_TRY(bc_encode(img, format, (flags & KC_BC_SRGB) != 0, (char *)staging.ptr, row_pitch, c.stream, bc_punch_through_ref(flags)));
    return bc_compare(img, format, flags, (const char *)staging.ptr, row_pitch, out);  // waits: the staging is free after it
}

// ---------------------------------------------------------------- DDS input
static uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

int dds_parse(const uint8_t *data, size_t bytes, kc_dds_info *info)
{
    auto unsupported = [](const char *what) {
        set_error(std::string("kc_dds_parse: ") + what);
        return KC_ERR_UNSUPPORTED;
    };
    if (!data || !info) return bcd_refuse("kc_dds_parse", "NULL buffer or output");
    if (bytes < 128) return bcd_refuse("kc_dds_parse", "fewer than the 128 bytes of a header");
    uint32_t d[37] = { 0 };
    const size_t words = bytes >= 148 ? 37 : 32;
    for (size_t i = 0; i < words; ++i) d[i] = le32(data + 4 * i);
    if (d[0] != fourcc('D', 'D', 'S', ' ')) return bcd_refuse("kc_dds_parse", "no DDS magic");
    if (d[1] != 124 || d[19] != 32) return bcd_refuse("kc_dds_parse", "dwSize is not 124 or the pixel format's is not 32");
    const uint32_t h = d[3], w = d[4];
    if (w == 0 || h == 0) return bcd_refuse("kc_dds_parse", "zero extent");
    const bool dx10 = (d[20] & 0x4u) && d[21] == fourcc('D', 'X', '1', '0');
    if (dx10 && bytes < 148) return bcd_refuse("kc_dds_parse", "fewer than the 148 bytes of a DX10 header");
    // well-formed from here on: what is not a BC texture this library decodes is unsupported
    if (!(d[20] & 0x4u)) return unsupported("not a FourCC format (uncompressed)");
    if ((d[28] & 0x200u) || (d[28] & 0x200000u) || ((d[2] & 0x800000u) && d[6] > 1)) return unsupported("cube maps and volumes");
    uint32_t flags = 0;
    const BcFormat *f = dx10 ? bc_format_of_dds(d[32], 0, &flags) : bc_format_of_dds(0, d[21], &flags);  // what kc_dds_header writes, and the legacy files
    if (dx10) {
        if (!f) return unsupported("a dxgiFormat other than BC1, BC3, BC4, BC5 and BC7 UNORM");
        if (d[33] != 3) return unsupported("a resource dimension other than TEXTURE2D");
        if (d[34] & 0x4u) return unsupported("cube maps");
        if (d[35] != 1) return unsupported("texture arrays");
    } else if (!f) {
        return unsupported("a FourCC other than DXT1, DXT5, ATI1 / BC4U, ATI2 / BC5U and DX10");
    }
    const int format = f->format;
    const uint32_t levels = ((d[2] & 0x20000u) && d[7]) ? d[7] : 1u;
    uint32_t L = 0;
    KC_TRY(mip_level_count(w, h, &L));
    if (levels > L) return bcd_refuse("kc_dds_parse", "more levels than the chain of this size has");
    std::vector<size_t> offs(L);
    size_t total = 0;
    KC_TRY(bc_mip_layout(w, h, format, nullptr, offs.data(), L, &total));
    const size_t data_offset = dx10 ? 148 : 128, data_bytes = levels == L ? total : offs[levels];
    if (bytes - data_offset < data_bytes) return bcd_refuse("kc_dds_parse", "shorter than the header's levels need");
    info->width = w;
    info->height = h;
    info->format = format;
    info->flags = flags;
    info->levels = levels;
    info->data_offset = data_offset;
    info->data_bytes = data_bytes;
    return KC_OK;
}

int image_read_dds(const char *path, uint32_t level, uint32_t flags, kc_image **out, kc_dds_info *info)
{
    if (flags & ~(uint32_t)(KC_BC_GRAY | KC_BC_ALL_MODES)) {
        set_error("kc_image_read_dds: flags other than KC_BC_GRAY and KC_BC_ALL_MODES");
        return KC_ERR_UNSUPPORTED;
    }
    if (!path || !out) return bcd_refuse("kc_image_read_dds", "NULL path or output");
    std::vector<uint8_t> file;
    {
        FILE *f = std::fopen(path, "rb");
        if (!f) {
            set_error(std::string("kc_image_read_dds: cannot open ") + path);
            return KC_ERR_IO;
        }
        uint8_t buf[1 << 16];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + n);
        const bool bad = std::ferror(f) != 0;
        std::fclose(f);
        if (bad) {
            set_error(std::string("kc_image_read_dds: cannot read ") + path);
            return KC_ERR_IO;
        }
    }
    kc_dds_info di;
    KC_TRY(dds_parse(file.data(), file.size(), &di));
    if (info) *info = di;
    if (level >= di.levels) return bcd_refuse("kc_image_read_dds", "level is not below the file's level count");
    uint32_t L = 0;
    KC_TRY(mip_level_count(di.width, di.height, &L));
    std::vector<size_t> offs(L);
    KC_TRY(bc_mip_layout(di.width, di.height, di.format, nullptr, offs.data(), L, nullptr));
    const uint32_t W = (di.width >> level) ? di.width >> level : 1u, H = (di.height >> level) ? di.height >> level : 1u;
    const size_t end = level + 1 < di.levels ? offs[level + 1] : di.data_bytes;
    return image_from_bc(file.data() + di.data_offset + offs[level], end - offs[level], W, H, di.format, flags, out, nullptr);
}

}  // namespace kc
