// Device-memory images: kc_device_image_validate, kc_image_from_device, kc_image_to_device (include/kanter_core_amd.h).  The host
// side checks the caller's descriptor -- arithmetic first, then that its bytes lie in one allocation of the library's device --
// and orders the conversion kernels of devimage.hip against the caller's stream with two event edges; nothing here waits.
#include "kc_runtime.hpp"

namespace kc {

static size_t elem_bytes(int dtype) { return dtype == KC_DTYPE_U8 ? 1 : dtype == KC_DTYPE_F32 ? 4 : 2; }

static int devimage_refuse(const char *what)
{
    set_error(std::string("kc_device_image: ") + what);
    return KC_ERR_INVALID_ARG;
}

// The arithmetic half of the validation: needs no device.
static int devimage_check_arith(const kc_device_image *d, size_t *extent)
{
    if (!d) return devimage_refuse("descriptor is NULL");
    if (d->channels < 1 || d->channels > 4) return devimage_refuse("channels must be 1..4");
    if (d->dtype < KC_DTYPE_U8 || d->dtype > KC_DTYPE_F32) return devimage_refuse("unknown dtype");
    if (d->layout != KC_LAYOUT_INTERLEAVED && d->layout != KC_LAYOUT_PLANAR) return devimage_refuse("unknown layout");
    if (!d->ptr || d->width == 0 || d->height == 0) return devimage_refuse("NULL pointer or zero extent");
    const size_t e = elem_bytes(d->dtype);
    const bool planar = d->layout == KC_LAYOUT_PLANAR && d->channels > 1;
    if ((uintptr_t)d->ptr % e || d->row_pitch_bytes % e || (planar && d->channel_pitch_bytes % e))
        return devimage_refuse("pointer and pitches must be multiples of the element size");
    // a quad index of the kernels is 32-bit, with room for the grid-stride step
    if ((uint64_t)((d->width + 3) / 4) * d->height > (1ull << 31)) return devimage_refuse("image too large");
    size_t row_bytes = 0, last = 0, ext = 0;
    const size_t px = d->layout == KC_LAYOUT_INTERLEAVED ? (size_t)d->channels : 1;
    if (__builtin_mul_overflow((size_t)d->width, px * e, &row_bytes)) return devimage_refuse("extent overflows");
    if (d->row_pitch_bytes < row_bytes)
        return devimage_refuse(d->layout == KC_LAYOUT_INTERLEAVED ? "row pitch < width * channels * element size"
                                                                   : "row pitch < width * element size");
    if (__builtin_mul_overflow((size_t)(d->height - 1), d->row_pitch_bytes, &last) || __builtin_add_overflow(last, row_bytes, &ext))
        return devimage_refuse("extent overflows");
    if (planar) {
        size_t plane = 0, planes = 0;
        if (__builtin_mul_overflow((size_t)d->height, d->row_pitch_bytes, &plane) || d->channel_pitch_bytes < plane)
            return devimage_refuse("channel planes overlap: channel pitch < height * row pitch");
        if (__builtin_mul_overflow((size_t)(d->channels - 1), d->channel_pitch_bytes, &planes) || __builtin_add_overflow(ext, planes, &ext))
            return devimage_refuse("extent overflows");
    }
    if ((uintptr_t)d->ptr + ext < (uintptr_t)d->ptr) return devimage_refuse("extent overflows");
    *extent = ext;
    return KC_OK;
}

// [ptr, ptr + extent) lies in one device allocation of the library's device (needs kc_init); `who` prefixes the error text
int device_extent_check(const void *ptr, size_t ext, const char *who)
{
    KC_TRY(need_init());
    Context &c = ctx();
    auto refuse = [&](const char *what) {
        set_error(std::string(who) + ": " + what);
        return KC_ERR_INVALID_ARG;
    };
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, ptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return refuse("ptr is not memory the HIP runtime knows (a host pointer?)");
    }
    if (attr.type != hipMemoryTypeDevice || attr.device != c.device) return refuse("ptr is not device memory of the library's device");
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return refuse("no device allocation contains ptr");
    }
    const uintptr_t lo = (uintptr_t)base, p = (uintptr_t)ptr;
    if (p < lo || p - lo > size || ext > size - (p - lo)) return refuse("the described extent runs past the end of its allocation");
    return KC_OK;
}

int device_image_validate(const kc_device_image *d, size_t *extent_bytes)
{
    size_t ext = 0;
    KC_TRY(devimage_check_arith(d, &ext));
    if (extent_bytes) *extent_bytes = ext;
    return device_extent_check(d->ptr, ext, "kc_device_image");
}

// vec: the pointer and the pitches allow the widest access of a whole pixel quad (devimage.hip: 16, 8 or 4 bytes for a
// quad of interleaved pixels, the quad's 4 elements per channel plane)
static DevImageArgs devimage_args(const kc_device_image *d)
{
    DevImageArgs a;
    a.ptr = (const char *)d->ptr;
    a.row_pitch = d->row_pitch_bytes;
    a.channel_pitch = d->channel_pitch_bytes;
    a.w = d->width;
    a.h = d->height;
    a.channels = d->channels;
    a.layout = d->layout;
    const size_t e = elem_bytes(d->dtype);
    size_t unit;
    uint64_t bits = (uintptr_t)d->ptr | d->row_pitch_bytes;
    if (d->layout == KC_LAYOUT_INTERLEAVED) {
        const size_t quad = 4 * (size_t)d->channels * e;
        unit = quad % 16 == 0 ? 16 : quad % 8 == 0 ? 8 : 4;
    } else {
        unit = 4 * e;
        if (d->channels > 1) bits |= d->channel_pitch_bytes;
    }
    a.vec = bits % unit == 0;
    return a;
}

// The library's stream waits for what `hip_stream` holds now (before the conversion) / `hip_stream` waits for the conversion
// (after it).  The events are released at once; the runtime keeps them until they have fired.
int stream_edge(hipStream_t from, hipStream_t to)
{
    hipEvent_t ev = nullptr;
    KC_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, from);
    if (e == hipSuccess) e = hipStreamWaitEvent(to, ev, 0);
    (void)hipEventDestroy(ev);
    if (e != hipSuccess) return hip_fail(e, "device image stream ordering");
    return KC_OK;
}

int image_from_device(const kc_device_image *src, uint32_t flags, void *hip_stream, kc_image **out)
{
    if (flags & ~(uint32_t)KC_DEVICE_GRAY) {
        set_error("kc_image_from_device: flags other than KC_DEVICE_GRAY");
        return KC_ERR_UNSUPPORTED;
    }
    KC_TRY(device_image_validate(src, nullptr));
    const bool gray = (flags & KC_DEVICE_GRAY) != 0;
    if (gray && src->channels != 1) return devimage_refuse("KC_DEVICE_GRAY needs channels == 1");
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    const uint32_t w = src->width, h = src->height;
    const int n = src->channels;
    kc_plane *p[4];
    float *dp[4];
    int s = image_planes_for_import(w, h, n, gray ? 1 : 4, p, dp);
    if (s == KC_OK)
        s = with_stream_edges(hip_stream, [&] {
            const DevImageArgs a = devimage_args(src);
            const uint64_t in_bytes = (uint64_t)w * h * n * elem_bytes(src->dtype), out_bytes = (uint64_t)w * h * 4 * n;
            bool nt = false;
            hipError_t e = launch_image_import(src->dtype, a, dp, (uint32_t)(p[0]->pitch / 4), cache_policy_mask(in_bytes, out_bytes, 1), c.stream, &nt);
            if (e != hipSuccess) return hip_fail(e, "launch_image_import");
            c.launches++;
            c.counters[a.vec ? "image_import_vec" : "image_import_scalar"]++;
            if (nt) c.counters["image_import_nt"]++;
            c.alg_bytes += in_bytes + out_bytes;
            return (int)KC_OK;
        });
    return image_of_import_planes(s, gray ? 1 : 4, p, out);
}

int image_to_device(kc_image *img, const kc_device_image *dst, uint32_t flags, void *hip_stream)
{
    if (flags & ~(uint32_t)KC_DEVICE_SRGB) {
        set_error("kc_image_to_device: flags other than KC_DEVICE_SRGB");
        return KC_ERR_UNSUPPORTED;
    }
    const bool srgb = (flags & KC_DEVICE_SRGB) != 0;
    if (srgb && dst && dst->dtype != KC_DTYPE_U8) {
        set_error("kc_image_to_device: KC_DEVICE_SRGB is for U8 only");
        return KC_ERR_UNSUPPORTED;
    }
    KC_TRY(device_image_validate(dst, nullptr));
    if (!img) return devimage_refuse("image is NULL");
    if (img->w() != dst->width || img->h() != dst->height) return devimage_refuse("descriptor size differs from the image's");
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    KC_TRY(image_force(img));  // a pending fused chain runs first
    const bool rgba = img->is_rgba();
    const int n = dst->channels;
    Operand o[4];
    const uint32_t n_res = image_source_operands(img, (1u << n) - 1, o);  // the distinct resident planes among the channels written
    const uint32_t w = img->w(), h = img->h();
    return with_stream_edges(hip_stream, [&] {
        const uint64_t in_bytes = (uint64_t)w * h * 4 * n_res, out_bytes = (uint64_t)w * h * n * elem_bytes(dst->dtype);
        const DevImageArgs a = devimage_args(dst);
        bool nt = false;
        hipError_t e = launch_image_export(dst->dtype, srgb ? 1 : 0, o, rgba ? 0 : 1, a, cache_policy_mask(in_bytes, out_bytes, n_res ? n_res : 1),
                                           c.stream, &nt);
        if (e != hipSuccess) return hip_fail(e, "launch_image_export");
        c.launches++;
        c.counters[a.vec ? "image_export_vec" : "image_export_scalar"]++;
        if (nt) c.counters["image_export_nt"]++;
        c.alg_bytes += in_bytes + out_bytes;
        return (int)KC_OK;
    });
}

}  // namespace kc
