// The export of mip chains (include/kanter_core_amd.h): kc_bc_mip_layout, kc_image_to_bc_mips, kc_image_to_bc_mips_device,
// kc_image_levels_to_bc_mips, kc_dds_header, kc_image_write_dds, kc_image_levels_write_dds.  The BC chain is mip.cpp's chain
// (image_build_mips) and bc.cpp's encoder launch once per level; the DDS writer is host code.
#include <cstdio>

#include "kc_runtime.hpp"

namespace kc {

// ---------------------------------------------------------------- the BC chain
// flags of the chain exporters: KC_BC_SRGB under kc_image_to_bc's rule (bc_check_flags), plus KC_MIP_PER_LEVEL, KC_MIP_NORMALS,
// which does not go with KC_BC_SRGB: a vector is not a colour, KC_MIP_COVERAGE_REF, and KC_BC_PUNCH_THROUGH, which shares its byte
static int bc_mips_check_flags(int format, uint32_t flags, const char *who)
{
    KC_TRY(bc_check_flags(format, flags,
                          KC_BC_SRGB | KC_MIP_PER_LEVEL | KC_MIP_NORMALS | KC_MIP_ALPHA_WEIGHT | kCoverageFlagBits | kBcPunchThroughBits, who));
    if ((flags & KC_MIP_NORMALS) && (flags & KC_BC_SRGB)) {
        set_error(std::string(who) + ": KC_MIP_NORMALS with KC_BC_SRGB");
        return KC_ERR_UNSUPPORTED;
    }
    KC_TRY(mip_check_alpha_flags(flags, who));
    return mip_check_coverage_flags(flags, who);
}

int bc_mip_layout(uint32_t w, uint32_t h, int format, uint32_t *levels, size_t *offsets, uint32_t cap, size_t *total_bytes)
{
    const BcFormat *f = bc_format(format);
    if (!f) return mip_refuse("kc_bc_mip_layout", "unknown format");
    if (w == 0 || h == 0) return mip_refuse("kc_bc_mip_layout", "zero extent");
    const uint32_t L = 1u + floor_log2(w > h ? w : h);
    if (levels) *levels = L;
    if (offsets && cap < L) return mip_refuse("kc_bc_mip_layout", "cap is below the level count");
    uint64_t bx = 0, by = 0;
    KC_TRY(bc_block_count(w, h, "kc_bc_mip_layout", &bx, &by));
    size_t at = 0;
    for (uint32_t k = 0; k < L; ++k) {
        if (offsets) offsets[k] = at;
        at += bc_level_bytes(level_extent(w, k), level_extent(h, k), *f);
    }
    if (total_bytes) *total_bytes = at;
    return KC_OK;
}

// The first `count` levels of a chain (forced) as blocks at dst, level k at its kc_bc_mip_layout offset; on the library's stream
static int bc_levels_encode(kc_image *const *lv, uint32_t count, int format, uint32_t flags, char *dst)
{
    Context &c = ctx();
    const BcFormat &f = *bc_format(format);  // the entry points have refused an unknown format
    size_t at = 0;
    int s = KC_OK;
    for (uint32_t k = 0; k < count && s == KC_OK; ++k) {
        const uint32_t W = lv[k]->w(), H = lv[k]->h();
        s = bc_encode(lv[k], format, (flags & KC_BC_SRGB) != 0, dst + at, (((size_t)W + 3) / 4) * f.block_bytes, c.stream,
                      bc_punch_through_ref(flags));
        at += bc_level_bytes(W, H, f);
    }
    return s;
}

// The chain of `img` (forced by image_build_mips) as blocks at dst
static int bc_mips_encode(kc_image *img, int format, uint32_t flags, char *dst)
{
    uint32_t L = 0;
    KC_TRY(mip_level_count(img->w(), img->h(), &L));
    std::vector<kc_image *> lv(L, nullptr);
    uint32_t count = 0;
    // the byte goes to the chain only with KC_MIP_COVERAGE: under KC_BC_PUNCH_THROUGH alone it is the encoder's
    const uint32_t chain_bits = KC_MIP_PER_LEVEL | KC_MIP_NORMALS | KC_MIP_ALPHA_WEIGHT | ((flags & KC_MIP_COVERAGE) ? kCoverageFlagBits : 0u);
    KC_TRY(image_build_mips(img, flags & chain_bits, lv.data(), L, &count));
    const int s = bc_levels_encode(lv.data(), L, format, flags, dst);
    // the level planes go back to the pool here; the pool hands a block out again only to work enqueued on the same stream
    for (kc_image *i : lv) image_release(i);
    return s;
}

// kc_image_levels_to_bc_mips / kc_image_levels_write_dds: the checks of a chain the caller holds; *total = the bytes of its
// `count` levels.  The flags, the arguments, need_init(), then the levels themselves, which are forced.
static int bc_levels_check(kc_image *const *levels, uint32_t count, int format, uint32_t flags, const void *out, const char *who, size_t *total)
{
    KC_TRY(bc_check_flags(format, flags, KC_BC_SRGB | kBcPunchThroughBits, who));
    const BcFormat *f = bc_format(format);
    if (!f) return mip_refuse(who, "unknown format");
    if (!levels || !out || count == 0) return mip_refuse(who, "NULL level array or output, or no level");
    KC_TRY(need_init());
    if (!levels[0]) return mip_refuse(who, "a NULL level");
    if ((flags & KC_BC_PUNCH_THROUGH) && !levels[0]->is_rgba()) return mip_refuse(who, "KC_BC_PUNCH_THROUGH is for RGBA images");
    const uint32_t w = levels[0]->w(), h = levels[0]->h();
    if (count > 1u + floor_log2(w > h ? w : h)) return mip_refuse(who, "more levels than the chain of level 0's size has");
    uint64_t bx = 0, by = 0;
    KC_TRY(bc_block_count(w, h, who, &bx, &by));
    *total = 0;
    for (uint32_t k = 0; k < count; ++k) {
        if (!levels[k] || levels[k]->n != levels[0]->n || levels[k]->w() != level_extent(w, k) || levels[k]->h() != level_extent(h, k))
            return mip_refuse(who, "every level must be an image of level 0's kind, max(1, w >> k) by max(1, h >> k)");
        *total += bc_level_bytes(level_extent(w, k), level_extent(h, k), *f);
    }
    for (uint32_t k = 0; k < count; ++k) KC_TRY(image_force(levels[k]));
    return KC_OK;
}

int image_levels_to_bc_mips(kc_image *const *levels, uint32_t count, int format, uint32_t flags, uint8_t *host, size_t host_bytes, const char *who)
{
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    size_t total = 0;
    KC_TRY(bc_levels_check(levels, count, format, flags, host, who, &total));
    if (host_bytes < total) return mip_refuse(who, "host_bytes is below the levels' bytes");
    PoolStaging staging;
    KC_TRY(staging.alloc(total));
    KC_TRY(bc_levels_encode(levels, count, format, flags, (char *)staging.ptr));
    hipError_t e = hipMemcpyAsync(host, staging.ptr, total, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) return hip_fail(e, who);
    return KC_OK;
}

int image_to_bc_mips(kc_image *img, int format, uint32_t flags, uint8_t *host, size_t host_bytes)
{
    KC_TRY(bc_mips_check_flags(format, flags, "kc_image_to_bc_mips"));
    if (!bc_format(format)) return mip_refuse("kc_image_to_bc_mips", "unknown format");
    if (!img || !host) return mip_refuse("kc_image_to_bc_mips", "NULL image or host buffer");
    KC_TRY(need_init());
    if ((flags & (KC_MIP_NORMALS | KC_MIP_COVERAGE | KC_MIP_ALPHA_WEIGHT | KC_BC_PUNCH_THROUGH)) && !img->is_rgba())
        return mip_refuse("kc_image_to_bc_mips", "KC_MIP_NORMALS, KC_MIP_COVERAGE, KC_MIP_ALPHA_WEIGHT and KC_BC_PUNCH_THROUGH are for RGBA images");
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    size_t total = 0;
    KC_TRY(bc_mip_layout(img->w(), img->h(), format, nullptr, nullptr, 0, &total));
    if (host_bytes < total) return mip_refuse("kc_image_to_bc_mips", "host_bytes is below the chain's bytes");
    PoolStaging staging;
    KC_TRY(staging.alloc(total));
    KC_TRY(bc_mips_encode(img, format, flags, (char *)staging.ptr));
    hipError_t e = hipMemcpyAsync(host, staging.ptr, total, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) return hip_fail(e, "image_to_bc_mips");
    return KC_OK;
}

int image_to_bc_mips_device(kc_image *img, int format, uint32_t flags, void *device_ptr, size_t bytes, void *hip_stream)
{
    KC_TRY(bc_mips_check_flags(format, flags, "kc_image_to_bc_mips_device"));
    const size_t bb = bc_block_bytes(format);
    if (bb == 0) return mip_refuse("kc_image_to_bc_mips_device", "unknown format");
    if (!img || !device_ptr) return mip_refuse("kc_image_to_bc_mips_device", "NULL image or device pointer");
    if ((uintptr_t)device_ptr % bb) return mip_refuse("kc_image_to_bc_mips_device", "the pointer must be a multiple of the block bytes");
    KC_TRY(need_init());  // an image exists only after kc_init: it is not looked at before
    if ((flags & (KC_MIP_NORMALS | KC_MIP_COVERAGE | KC_MIP_ALPHA_WEIGHT | KC_BC_PUNCH_THROUGH)) && !img->is_rgba())
        return mip_refuse("kc_image_to_bc_mips_device", "KC_MIP_NORMALS, KC_MIP_COVERAGE, KC_MIP_ALPHA_WEIGHT and KC_BC_PUNCH_THROUGH are for RGBA images");
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    size_t total = 0;
    KC_TRY(bc_mip_layout(img->w(), img->h(), format, nullptr, nullptr, 0, &total));
    if (bytes < total) return mip_refuse("kc_image_to_bc_mips_device", "bytes is below the chain's bytes");
    KC_TRY(device_extent_check(device_ptr, total, "kc_image_to_bc_mips_device"));
    return with_stream_edges(hip_stream, [&] { return bc_mips_encode(img, format, flags, (char *)device_ptr); });
}

// ---------------------------------------------------------------- DDS
int dds_header(uint32_t w, uint32_t h, int format, uint32_t flags, uint32_t levels, uint8_t *out, size_t *bytes)
{
    KC_TRY(bc_check_flags(format, flags, KC_BC_SRGB, "kc_dds_header"));
    const BcFormat *f = bc_format(format);
    if (!f) return mip_refuse("kc_dds_header", "unknown format");
    if (!out || w == 0 || h == 0) return mip_refuse("kc_dds_header", "NULL output or zero extent");
    if (levels == 0 || levels > 1u + floor_log2(w > h ? w : h)) return mip_refuse("kc_dds_header", "levels is 0 or above the chain's level count");
    const uint64_t linear = (((uint64_t)w + 3) / 4) * (((uint64_t)h + 3) / 4) * f->block_bytes;
    if (linear > 0xffffffffull) return mip_refuse("kc_dds_header", "level 0 is larger than the header can say");
    const bool mips = levels > 1;
    uint32_t d[37] = { 0 };
    d[0] = fourcc('D', 'D', 'S', ' ');
    d[1] = 124;          // DDS_HEADER: dwSize
    d[2] = 0x1u | 0x2u | 0x4u | 0x1000u | 0x80000u | (mips ? 0x20000u : 0u);  // CAPS, HEIGHT, WIDTH, PIXELFORMAT, LINEARSIZE, MIPMAPCOUNT
    d[3] = h;
    d[4] = w;
    d[5] = (uint32_t)linear;  // dwPitchOrLinearSize
    d[6] = 0;                 // dwDepth
    d[7] = levels;            // dwMipMapCount; d[8..18]: reserved
    d[19] = 32;               // DDS_PIXELFORMAT: dwSize
    d[20] = 0x4;              // DDPF_FOURCC
    d[21] = fourcc('D', 'X', '1', '0');  // d[22..26]: bit count and masks, 0
    d[27] = 0x1000u | (mips ? 0x8u | 0x400000u : 0u);  // dwCaps: TEXTURE (, COMPLEX, MIPMAP); d[28..31]: 0
    d[32] = (flags & KC_BC_SRGB) ? f->dxgi_srgb : f->dxgi;  // DDS_HEADER_DXT10: the number kc_dds_parse looks up in the same table
    d[33] = 3;                // D3D10_RESOURCE_DIMENSION_TEXTURE2D
    d[34] = 0;                // miscFlag
    d[35] = 1;                // arraySize
    d[36] = 0;                // miscFlags2
    for (int i = 0; i < 37; ++i)  // little-endian, whatever the host's order
        for (int b = 0; b < 4; ++b) out[4 * i + b] = (uint8_t)(d[i] >> (8 * b));
    if (bytes) *bytes = 148;
    return KC_OK;
}

static int dds_write_file(const char *path, const std::vector<uint8_t> &file, const char *who)
{
    FILE *f = std::fopen(path, "wb");
    if (!f) {
        set_error(std::string(who) + ": cannot open " + path);
        return KC_ERR_IO;
    }
    const bool ok = std::fwrite(file.data(), 1, file.size(), f) == file.size();
    if (std::fclose(f) != 0 || !ok) {
        set_error(std::string(who) + ": cannot write " + path);
        return KC_ERR_IO;
    }
    return KC_OK;
}

int image_write_dds(kc_image *img, const char *path, int format, uint32_t flags, int with_mips)
{
    KC_TRY(bc_mips_check_flags(format, flags, "kc_image_write_dds"));
    if (!bc_format(format)) return mip_refuse("kc_image_write_dds", "unknown format");
    if (!img || !path) return mip_refuse("kc_image_write_dds", "NULL image or path");
    KC_TRY(need_init());
    const uint32_t w = img->w(), h = img->h();
    uint32_t L = 1;
    size_t total = 0;
    KC_TRY(bc_mip_layout(w, h, format, &L, nullptr, 0, &total));
    if (!with_mips) {
        L = 1;
        total = bc_level_bytes(w, h, *bc_format(format));
    }
    std::vector<uint8_t> file(148 + total);
    KC_TRY(dds_header(w, h, format, flags & KC_BC_SRGB, L, file.data(), nullptr));
    if (with_mips) KC_TRY(image_to_bc_mips(img, format, flags, file.data() + 148, total));
    else KC_TRY(image_to_bc(img, format, flags & (KC_BC_SRGB | ((flags & KC_BC_PUNCH_THROUGH) ? kBcPunchThroughBits : 0u)), file.data() + 148, total));
    return dds_write_file(path, file, "kc_image_write_dds");
}

int image_levels_write_dds(kc_image *const *levels, uint32_t count, const char *path, int format, uint32_t flags)
{
    const char *who = "kc_image_levels_write_dds";
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    size_t total = 0;
    KC_TRY(bc_levels_check(levels, count, format, flags, path, who, &total));
    std::vector<uint8_t> file(148 + total);
    KC_TRY(dds_header(levels[0]->w(), levels[0]->h(), format, flags & KC_BC_SRGB, count, file.data(), nullptr));
    KC_TRY(image_levels_to_bc_mips(levels, count, format, flags, file.data() + 148, total, who));
    return dds_write_file(path, file, who);
}

}  // namespace kc
