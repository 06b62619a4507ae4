// kc_image_blur, kc_blur_weights, kc_blur_texel (include/kanter_core_amd.h): a separable Gaussian blur of the planes of an image.
// Constant planes are answered here with the same two functions the entry points expose; resident ones go through blur.hip's
// launches, one per blurred axis for all of them together, with the f32 intermediate in a staging block of the pool that goes
// back when the call returns (both launches are enqueued by then).
#include <cmath>

#include "kc_runtime.hpp"

namespace kc {

static int blur_refuse(const char *who, const char *what)
{
    set_error(std::string(who) + ": " + what);
    return KC_ERR_INVALID_ARG;
}

// The radius of a sigma the rule accepts; 0 for sigma == 0 (the axis is not blurred); -1 for one it refuses
static int blur_radius(float sigma)
{
    if (!(sigma >= 0.0f) || std::isinf(sigma)) return -1;  // NaN, negative, infinite
    if (sigma == 0.0f) return 0;
    const double r = std::ceil(3.0 * (double)sigma);
    if (r > (double)KC_BLUR_MAX_RADIUS) return -1;
    return r < 1.0 ? 1 : (int)r;
}

int blur_weights(float sigma, float *weights, uint32_t capacity, uint32_t *radius)
{
    const int R = blur_radius(sigma);
    if (R < 1 || capacity < (uint32_t)R + 1u) return KC_ERR_INVALID_ARG;
    const double s = (double)sigma;
    double g[KC_BLUR_MAX_RADIUS + 1];
    for (int k = 0; k <= R; ++k) g[k] = std::exp(-(double)(k * k) / (2.0 * s * s));
    volatile double side = 0.0;  // volatile: every sum below is one IEEE f64 operation, in this order
    for (int k = 1; k <= R; ++k) side = side + g[k];
    volatile double twice = 2.0 * side;
    volatile double total = g[0] + twice;
    for (int k = 0; k <= R; ++k) weights[k] = (float)(g[k] / total);
    *radius = (uint32_t)R;
    return KC_OK;
}

// The texel rule as the device computes it (blur.hip): every f32 operation is rounded on its own, the outermost pair first
float blur_texel(const float *taps, const float *weights, uint32_t R)
{
    volatile float pair = taps[0] + taps[2u * R];
    volatile float acc = weights[R] * pair;
    for (uint32_t k = R - 1u; k >= 1u; --k) {
        pair = taps[R - k] + taps[R + k];
        volatile float term = weights[k] * pair;
        acc = acc + term;
    }
    volatile float centre = weights[0] * taps[R];
    acc = acc + centre;
    return acc;
}

// a constant through one axis: the rule on all-equal taps
static float blur_const(float v, const float *weights, uint32_t R)
{
    float taps[2 * KC_BLUR_MAX_RADIUS + 1];
    for (uint32_t i = 0; i <= 2u * R; ++i) taps[i] = v;
    return blur_texel(taps, weights, R);
}

int image_blur(kc_image *img, float sigma_x, float sigma_y, uint32_t channel_mask, uint32_t flags, kc_image **out)
{
    const char *who = "kc_image_blur";
    KC_TRY(need_init());
    if (flags & ~(uint32_t)KC_BLUR_WRAP) {
        set_error(std::string(who) + ": flags other than KC_BLUR_WRAP");
        return KC_ERR_UNSUPPORTED;
    }
    if (!img || !out) return blur_refuse(who, "NULL argument");
    const int rx = blur_radius(sigma_x), ry = blur_radius(sigma_y);
    if (rx < 0 || ry < 0) return blur_refuse(who, "a sigma is NaN, negative, infinite or needs a radius above KC_BLUR_MAX_RADIUS");
    if (channel_mask == 0 || (channel_mask >> img->n) != 0) return blur_refuse(who, "the channel mask is empty or names a channel the image does not have");
    const uint32_t w = img->w(), h = img->h();
    if ((uint64_t)w * h > (1ull << 31)) return blur_refuse(who, "image too large");
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    KC_TRY(image_force(img));  // a pending fused chain or resample runs first
    const int n = img->n;
    if (rx == 0 && ry == 0) {  // neither axis is blurred: the source's planes themselves
        *out = image_new(n, img->planes);
        return KC_OK;
    }
    BlurArgs ax{}, ay{};  // the x pass and the y pass
    uint32_t Rx = 0, Ry = 0;
    if (rx > 0 && blur_weights(sigma_x, ax.weights, KC_BLUR_MAX_RADIUS + 1, &Rx) != KC_OK) return blur_refuse(who, "sigma_x");
    if (ry > 0 && blur_weights(sigma_y, ay.weights, KC_BLUR_MAX_RADIUS + 1, &Ry) != KC_OK) return blur_refuse(who, "sigma_y");

    // Every channel's result: the source's plane where the mask leaves it out, the result of an earlier channel that is the same
    // plane, a constant, or a new plane that the launches fill
    kc_plane *res[4] = { nullptr, nullptr, nullptr, nullptr };
    uint32_t n_res = 0;  // the distinct resident planes the launches read
    int status = KC_OK;
    for (int ch = 0; ch < n && status == KC_OK; ++ch) {
        kc_plane *p = img->planes[ch];
        if (!(channel_mask >> ch & 1u)) {
            plane_retain(p);
            res[ch] = p;
            continue;
        }
        int same = -1;
        for (int e = 0; e < ch; ++e)
            if ((channel_mask >> e & 1u) && img->planes[e] == p) same = e;
        if (same >= 0) {
            plane_retain(res[same]);
            res[ch] = res[same];
        } else if (p->kind == kc_plane::CONST) {
            float v = p->cval;
            if (Rx) v = blur_const(v, ax.weights, Rx);
            if (Ry) v = blur_const(v, ay.weights, Ry);
            res[ch] = plane_new_const(w, h, v);
        } else {
            status = plane_new_mem(w, h, &res[ch]);
            if (status == KC_OK) {
                ax.src[n_res] = p->dptr;
                ax.src_pitch[n_res] = (uint32_t)(p->pitch / sizeof(float));
                ay.dst[n_res] = res[ch]->dptr;
                ay.dst_pitch[n_res] = (uint32_t)(res[ch]->pitch / sizeof(float));
                ++n_res;
            }
        }
    }
    PoolStaging mid;
    const uint32_t mid_pitch = (w + 3u) / 4u * 4u;
    const size_t mid_plane = (size_t)mid_pitch * h;
    if (status == KC_OK && n_res && Rx && Ry) status = mid.alloc(mid_plane * n_res * sizeof(float));
    if (status == KC_OK && n_res) {
        for (uint32_t i = 0; i < n_res; ++i) {
            if (Rx && Ry) {  // x into the intermediate, y out of it
                ax.dst[i] = (float *)mid.ptr + mid_plane * i;
                ax.dst_pitch[i] = mid_pitch;
                ay.src[i] = ax.dst[i];
                ay.src_pitch[i] = mid_pitch;
            } else if (Rx) {
                ax.dst[i] = ay.dst[i];
                ax.dst_pitch[i] = ay.dst_pitch[i];
            } else {
                ay.src[i] = ax.src[i];
                ay.src_pitch[i] = ax.src_pitch[i];
            }
        }
        ax.w = ay.w = w;
        ax.h = ay.h = h;
        ax.planes = ay.planes = n_res;
        ax.radius = Rx;
        ay.radius = Ry;
        const bool wrap = (flags & KC_BLUR_WRAP) != 0;
        const uint64_t bytes = (uint64_t)w * h * 4 * n_res;
        const uint32_t policy = cache_policy_mask(bytes, bytes, n_res);
        const bool nt_in = (policy & 1u) != 0, nt_out = (policy & 0x100u) != 0;  // the source of the first pass, the result of the last
        hipError_t e = hipSuccess;
        if (Rx) {
            e = launch_blur_rows(ax, wrap, nt_in, c.stream);
            if (e == hipSuccess) {
                c.launches++;
                c.counters["blur_rows"]++;
                if (nt_in) c.counters["blur_rows_nt"]++;
                c.alg_bytes += bytes * 2;  // every texel read and written
            }
        }
        if (Ry && e == hipSuccess) {
            e = launch_blur_columns(ay, wrap, nt_out, c.stream);
            if (e == hipSuccess) {
                c.launches++;
                c.counters["blur_columns"]++;
                if (nt_out) c.counters["blur_columns_nt"]++;
                c.alg_bytes += bytes * 2;
            }
        }
        if (e != hipSuccess) status = hip_fail(e, "launch_blur");
    }
    if (status == KC_OK) *out = image_new(n, res);
    for (int ch = 0; ch < n; ++ch)
        if (res[ch]) plane_release(res[ch]);
    return status;
}

}  // namespace kc
