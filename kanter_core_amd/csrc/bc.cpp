// Block compression: kc_bc_image_validate, kc_image_to_bc, kc_image_to_bc_device (include/kanter_core_amd.h).  The host side
// checks the arguments and the caller's descriptor -- arithmetic first, then that its bytes lie in one allocation of the
// library's device -- and launches bc.hip's encoder (KC_BC7: bc7.hip's, KC_BC6H: bc6h.hip's) once per call: on the library's stream, ordered
// against the caller's stream by the two event edges of kc_image_to_device, or into pool staging that is copied to the
// caller's host memory.
#include "kc_runtime.hpp"

namespace kc {

size_t bc_block_bytes(int format)
{
    return format == KC_BC1 || format == KC_BC4 ? 8 : format == KC_BC3 || format == KC_BC5 || format == KC_BC7 || format == KC_BC6H ? 16 : 0;
}

static int bc_refuse(const char *what)
{
    set_error(std::string("kc_bc_image: ") + what);
    return KC_ERR_INVALID_ARG;
}

// Flag bits other than KC_BC_SRGB, or KC_BC_SRGB with a format without colour, are KC_ERR_UNSUPPORTED
int bc_check_flags(int format, uint32_t flags, const char *who)
{
    if (flags & ~(uint32_t)KC_BC_SRGB) {
        set_error(std::string(who) + ": flags other than KC_BC_SRGB");
        return KC_ERR_UNSUPPORTED;
    }
    if ((flags & KC_BC_SRGB) && (format == KC_BC4 || format == KC_BC5 || format == KC_BC6H)) {
        set_error(std::string(who) + ": KC_BC_SRGB is for BC1, BC3 and BC7 only");
        return KC_ERR_UNSUPPORTED;
    }
    return KC_OK;
}

// The arithmetic half of the validation: needs no device.
static int bc_check_arith(const kc_bc_image *d, size_t *extent)
{
    if (!d) return bc_refuse("descriptor is NULL");
    const size_t bb = bc_block_bytes(d->format);
    if (bb == 0) return bc_refuse("unknown format");
    if (!d->ptr || d->width == 0 || d->height == 0) return bc_refuse("NULL pointer or zero extent");
    const uint64_t bx = ((uint64_t)d->width + 3) / 4, by = ((uint64_t)d->height + 3) / 4;
    // the kernel's block index is 32-bit, with room for the grid-stride step
    if (bx * by > (1ull << 31)) return bc_refuse("image too large: more than 2^31 blocks");
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

// One launch of the encoder for `img` (forced already) into `dst`, block rows `row_pitch` bytes apart.  The channels the format
// reads come from the image as to_u8 sees it (Gray: (v, v, v, 1)); constants cost no loads.  KC_BC6H reads R, G and B.
int bc_encode(kc_image *img, int format, bool srgb, char *dst, size_t row_pitch, hipStream_t s)
{
    Context &c = ctx();
    const bool rgba = img->is_rgba();
    Operand o[4];
    for (int i = 0; i < 4; ++i) o[i] = rgba ? plane_operand(img->planes[i]) : i < 3 ? plane_operand(img->planes[0]) : Operand{ nullptr, 0, 1.0f };
    const int n_ch = format == KC_BC1 || format == KC_BC6H ? 3 : format == KC_BC3 || format == KC_BC7 ? 4 : format == KC_BC4 ? 1 : 2;
    const float *seen[4] = { nullptr, nullptr, nullptr, nullptr };
    uint32_t n_res = 0;  // distinct resident planes the launch reads
    for (int i = 0; i < n_ch; ++i) {
        if (!o[i].ptr) continue;
        bool dup = false;
        for (uint32_t k = 0; k < n_res; ++k) dup |= seen[k] == o[i].ptr;
        if (!dup) seen[n_res++] = o[i].ptr;
    }
    const uint32_t w = img->w(), h = img->h();
    const uint64_t in_bytes = (uint64_t)w * h * 4 * n_res;
    const uint64_t out_bytes = (uint64_t)((w + 3) / 4) * ((h + 3) / 4) * bc_block_bytes(format);
    const uint32_t nt_mask = cache_policy_mask(in_bytes, out_bytes, n_res ? n_res : 1);
    hipError_t e = format == KC_BC6H  ? launch_bc6h_encode(o, rgba ? 0 : 1, dst, row_pitch, w, h, nt_mask, s)
                   : format == KC_BC7 ? launch_bc7_encode(srgb ? 1 : 0, o, rgba ? 0 : 1, dst, row_pitch, w, h, nt_mask, s)
                                      : launch_bc_encode(format, srgb ? 1 : 0, o, rgba ? 0 : 1, dst, row_pitch, w, h, nt_mask, s);
    if (e != hipSuccess) return hip_fail(e, "launch_bc_encode");
    c.launches++;
    c.alg_bytes += in_bytes + out_bytes;
    return KC_OK;
}

int image_to_bc(kc_image *img, int format, uint32_t flags, uint8_t *host, size_t host_bytes)
{
    KC_TRY(bc_check_flags(format, flags, "kc_image_to_bc"));
    const size_t bb = bc_block_bytes(format);
    if (bb == 0) return bc_refuse("unknown format");
    if (!img || !host) return bc_refuse("NULL image or host buffer");
    KC_TRY(need_init());
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    const uint32_t w = img->w(), h = img->h();
    const uint64_t bx = ((uint64_t)w + 3) / 4, by = ((uint64_t)h + 3) / 4;
    if (bx * by > (1ull << 31)) return bc_refuse("image too large: more than 2^31 blocks");
    const size_t nbytes = (size_t)(bx * by) * bb;
    if (host_bytes < nbytes) return bc_refuse("host_bytes < blocks * block bytes");
    KC_TRY(image_force(img));  // a pending fused chain runs first
    const size_t block = (nbytes + 255) / 256 * 256;
    void *staging = nullptr;
    KC_TRY(pool_alloc(block, &staging));
    int s = bc_encode(img, format, (flags & KC_BC_SRGB) != 0, (char *)staging, (size_t)bx * bb, c.stream);
    hipError_t e = hipSuccess;
    if (s == KC_OK) e = hipMemcpyAsync(host, staging, nbytes, hipMemcpyDeviceToHost, c.stream);
    if (s == KC_OK && e == hipSuccess) e = hipStreamSynchronize(c.stream);
    pool_free(staging, block);
    if (s != KC_OK) return s;
    if (e != hipSuccess) return hip_fail(e, "image_to_bc");
    return KC_OK;
}

int image_to_bc_device(kc_image *img, const kc_bc_image *dst, uint32_t flags, void *hip_stream)
{
    KC_TRY(bc_check_flags(dst ? dst->format : 0, flags, "kc_image_to_bc_device"));
    KC_TRY(bc_image_validate(dst, nullptr));
    if (!img) return bc_refuse("image is NULL");
    if (img->w() != dst->width || img->h() != dst->height) return bc_refuse("descriptor size differs from the image's");
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    KC_TRY(image_force(img));  // a pending fused chain runs first
    hipStream_t hs = (hipStream_t)hip_stream;
    const bool edges = hs && hs != c.stream;
    if (edges) KC_TRY(stream_edge(hs, c.stream));
    KC_TRY(bc_encode(img, dst->format, (flags & KC_BC_SRGB) != 0, (char *)dst->ptr, dst->row_pitch_bytes, c.stream));
    if (edges) KC_TRY(stream_edge(c.stream, hs));
    return KC_OK;
}

}  // namespace kc
