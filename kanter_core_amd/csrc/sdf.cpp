// kc_image_distance_field, kc_sdf_texel, kc_sdf_cap (include/kanter_core_amd.h): the signed distance field of one channel's
// alpha-test mask.  A constant plane is answered here; a resident one goes through sdf.hip's two launches, with the 16-bit
// intermediate in a staging block of the pool that goes back when the call returns (both launches are enqueued by then).
#include <cmath>

#include "kc_runtime.hpp"

namespace kc {

static int sdf_refuse(const char *who, const char *what)
{
    set_error(std::string(who) + ": " + what);
    return KC_ERR_INVALID_ARG;
}

uint32_t sdf_cap(uint32_t spread) { return spread * spread + spread + 1u; }

// The value rule as the device computes it (sdf.hip, sdf_value): every f64 operation is IEEE, the one rounding to f32 is last
float sdf_texel(uint32_t d2, bool inside, uint32_t spread)
{
    if (d2 >= sdf_cap(spread)) return inside ? 1.0f : 0.0f;
    volatile double d = std::sqrt((double)d2);
    volatile double sd = inside ? d - 0.5 : 0.5 - d;
    volatile double q = sd / (2.0 * (double)spread);
    volatile double v = 0.5 + q;
    return (float)v;
}

int image_distance_field(kc_image *img, uint32_t channel, uint32_t ref_u8, uint32_t spread, uint32_t flags, kc_image **out)
{
    const char *who = "kc_image_distance_field";
    KC_TRY(need_init());
    if (flags & ~(uint32_t)KC_SDF_WRAP) {
        set_error(std::string(who) + ": flags other than KC_SDF_WRAP");
        return KC_ERR_UNSUPPORTED;
    }
    if (!img || !out) return sdf_refuse(who, "NULL argument");
    if (ref_u8 < 1 || ref_u8 > 255) return sdf_refuse(who, "the reference byte is outside 1..255");
    if (spread < 1 || spread > KC_SDF_MAX_SPREAD) return sdf_refuse(who, "the spread is outside 1..KC_SDF_MAX_SPREAD");
    if (channel >= (uint32_t)img->n) return sdf_refuse(who, "the image has no such channel");
    const uint32_t w = img->w(), h = img->h();
    if ((uint64_t)w * h > (1ull << 31)) return sdf_refuse(who, "image too large");
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    KC_TRY(image_force(img));  // a pending fused chain or resample runs first
    const kc_plane *p = img->planes[channel];
    const bool wrap = (flags & KC_SDF_WRAP) != 0;
    kc_plane *res = nullptr;
    if (p->kind == kc_plane::CONST) {  // one class only: every texel saturates
        res = plane_new_const(w, h, quant_u8_host(p->cval) >= ref_u8 ? 1.0f : 0.0f);
    } else {
        PoolStaging mid;
        KC_TRY(mid.alloc((size_t)w * h * sizeof(uint16_t)));
        KC_TRY(plane_new_mem(w, h, &res));
        SdfArgs a{};
        a.src = p->dptr;
        a.src_pitch = (uint32_t)(p->pitch / sizeof(float));
        a.mid = (uint16_t *)mid.ptr;
        a.dst = res->dptr;
        a.dst_pitch = (uint32_t)(res->pitch / sizeof(float));
        a.w = w;
        a.h = h;
        a.ref = ref_u8;
        a.spread = spread;
        const uint64_t texels = (uint64_t)w * h;
        const uint32_t policy = cache_policy_mask(texels * 4, texels * 4, 1);
        const bool nt_in = (policy & 1u) != 0, nt_out = (policy & 0x100u) != 0;
        hipError_t e = launch_sdf_columns(a, wrap, nt_in, c.stream);
        if (e == hipSuccess) {
            c.launches++;
            c.counters["sdf_columns"]++;
            e = launch_sdf_rows(a, wrap, nt_out, c.stream);
        }
        if (e != hipSuccess) {
            plane_release(res);
            return hip_fail(e, "launch_sdf");
        }
        c.launches++;
        c.counters["sdf_rows"]++;
        if (nt_in) c.counters["sdf_columns_nt"]++;
        if (nt_out) c.counters["sdf_rows_nt"]++;
        c.alg_bytes += texels * (4 + 2 + 2 + 4);  // the plane read, the intermediate written and read back, the field written
    }
    *out = image_new(1, &res);
    plane_release(res);
    return KC_OK;
}

}  // namespace kc
