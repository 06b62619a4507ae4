// kc_image_channel_stats (include/kanter_core_amd.h): per-channel min, max, NaN count and u8 histograms.  Constant channels
// are answered here; the distinct resident planes go to one launch of stats.hip's kernels, whose result is copied to pinned
// host memory and waited for with an event of the call's own.
#include <cmath>

#include "kc_runtime.hpp"

namespace kc {

// The sRGB threshold table of the device quantiser, as host data: quant_u8_srgb below counts thresholds exactly as the
// device form settles its estimate, so a constant channel lands in the bin its pixels would.
namespace host_srgb {
#pragma push_macro("__constant__")
#undef __constant__
#define __constant__ static const
#include "srgb_thresholds.inc"
#pragma pop_macro("__constant__")
}  // namespace host_srgb

// streaming.h's quant_u8, on the host: ((v.clamp(0,1) * 255.).min(255.)) as u8, NaN -> 255
uint32_t quant_u8_host(float v)
{
    float x = v;
    if (x < 0.0f) x = 0.0f;
    if (x > 1.0f) x = 1.0f;
    x = x * 255.0f;
    if (!(x <= 255.0f)) x = 255.0f;
    return (uint32_t)x;
}

// streaming.h's quant_u8_srgb, on the host: the number of thresholds T[1..255] the clamped value reaches
static uint32_t quant_u8_srgb_host(float v)
{
    float x = v;
    if (x < 0.0f) x = 0.0f;
    if (x > 1.0f) x = 1.0f;
    if (x != x) return 255u;
    uint32_t xb;
    std::memcpy(&xb, &x, 4);
    if ((int32_t)xb <= 0) return 0u;  // +0.0 and -0.0
    uint32_t q = 0;
    while (q < 255u && xb >= host_srgb::kSrgbThresholdBits[q + 1]) ++q;
    return q;
}

static float key_value(unsigned long long key)
{
    const uint32_t k = (uint32_t)key, bits = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

void channel_stats_release()
{
    Context::StatsBuffers &b = ctx().stats;
    if (b.done) (void)hipEventDestroy(b.done);
    if (b.partials) (void)hipFree(b.partials);
    if (b.result) (void)hipFree(b.result);
    if (b.host) (void)hipHostFree(b.host);
    b = Context::StatsBuffers{};
}

static constexpr uint32_t kStatsMaxWords = 16 + 4 * 256;  // a record / the result with four histograms

// The context's buffers, with room for `partials_bytes` of partial records (bc_decode.cpp's reductions use them too)
int stats_buffers(size_t partials_bytes)
{
    Context::StatsBuffers &b = ctx().stats;
    if (!b.done) {
        int cus = 0;
        KC_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx().device));
        b.cus = cus > 0 ? (uint32_t)cus : 1u;
        KC_HIP(hipMalloc((void **)&b.result, kStatsMaxWords * sizeof(unsigned long long)));
        KC_HIP(hipHostMalloc((void **)&b.host, kStatsMaxWords * sizeof(unsigned long long), hipHostMallocDefault));
        KC_HIP(hipEventCreateWithFlags(&b.done, hipEventDisableTiming));
    }
    if (b.partials_bytes < partials_bytes) {
        if (b.partials) {
            // the previous call's launches have finished (it waited for them): the old block is free
            KC_HIP(hipFree(b.partials));
            b.partials = nullptr;
            b.partials_bytes = 0;
        }
        KC_HIP(hipMalloc(&b.partials, partials_bytes));
        b.partials_bytes = partials_bytes;
    }
    return KC_OK;
}

int stats_fetch(uint32_t words)
{
    Context &c = ctx();
    KC_HIP(hipMemcpyAsync(c.stats.host, c.stats.result, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
    KC_HIP(hipEventRecord(c.stats.done, c.stream));
    KC_HIP(hipEventSynchronize(c.stats.done));
    return KC_OK;
}

int image_channel_stats(kc_image *img, uint32_t flags, kc_channel_stats *out)
{
    if (flags & ~(uint32_t)(KC_STATS_HISTOGRAM | KC_STATS_SRGB)) {
        set_error("kc_image_channel_stats: flags other than KC_STATS_HISTOGRAM and KC_STATS_SRGB");
        return KC_ERR_UNSUPPORTED;
    }
    const bool hist = (flags & KC_STATS_HISTOGRAM) != 0, srgb = (flags & KC_STATS_SRGB) != 0;
    if (srgb && !hist) {
        set_error("kc_image_channel_stats: KC_STATS_SRGB needs KC_STATS_HISTOGRAM");
        return KC_ERR_INVALID_ARG;
    }
    KC_TRY(need_init());
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    KC_TRY(image_force(img));  // a pending fused chain or resample runs first
    const uint32_t w = img->w(), h = img->h();
    if ((uint64_t)((w + 3) / 4) * h > (1ull << 31)) {  // the kernel's quad index is 32-bit, with room for the grid-stride step
        set_error("kc_image_channel_stats: image too large");
        return KC_ERR_UNSUPPORTED;
    }
    const int n = img->n;
    kc_channel_stats r;
    std::memset(&r, 0, sizeof r);
    r.channels = (uint32_t)n;
    r.flags = flags;
    r.pixels = (uint64_t)w * h;
    for (int i = 0; i < 4; ++i) r.min[i] = r.max[i] = NAN;

    // slots: the distinct resident planes, one per quantiser they are binned with (alpha is linear under KC_STATS_SRGB)
    StatsArgs a{};
    a.w = w;
    a.h = h;
    int slot_of[4] = { -1, -1, -1, -1 };
    for (int ch = 0; ch < n; ++ch) {
        const kc_plane *p = img->planes[ch];
        const bool sq = srgb && ch < 3;
        if (p->kind == kc_plane::CONST) {
            const float v = p->cval;
            if (std::isnan(v)) r.nan_count[ch] = r.pixels;
            else r.min[ch] = r.max[ch] = v;
            if (hist) r.histogram[ch][sq ? quant_u8_srgb_host(v) : quant_u8_host(v)] = r.pixels;
            continue;
        }
        const uint32_t pitch = (uint32_t)(p->pitch / sizeof(float));
        uint32_t s = 0;
        while (s < a.n && !(a.ptr[s] == p->dptr && a.pitch[s] == pitch && ((a.srgb >> s) & 1u) == (sq ? 1u : 0u))) ++s;
        if (s == a.n) {
            a.ptr[s] = p->dptr;
            a.pitch[s] = pitch;
            a.srgb |= (sq ? 1u : 0u) << s;
            a.n++;
        }
        slot_of[ch] = (int)s;
    }
    if (a.n > 0) {
        a.rec_words = 16u + (hist ? 256u * a.n : 0u);
        KC_TRY(stats_buffers(0));
        const uint32_t groups = channel_stats_groups(w, h, hist, srgb, c.stats.cus);
        KC_TRY(stats_buffers((size_t)groups * a.rec_words * sizeof(uint32_t)));
        a.partials = (uint32_t *)c.stats.partials;
        a.result = c.stats.result;
        const uint64_t in_bytes = (uint64_t)w * h * 4 * a.n;
        const bool nt = (cache_policy_mask(in_bytes, 0, a.n) & 0xffu) != 0;
        hipError_t e = launch_channel_stats(a, hist, srgb && a.srgb != 0, nt, groups, c.stream);
        if (e != hipSuccess) return hip_fail(e, "launch_channel_stats");
        c.launches += 2;
        if (nt) c.counters["stats_nt"]++;
        c.alg_bytes += in_bytes;
        KC_TRY(stats_fetch(a.rec_words));
        const unsigned long long *res = c.stats.host;
        for (int ch = 0; ch < n; ++ch) {
            const int s = slot_of[ch];
            if (s < 0) continue;
            r.nan_count[ch] = res[8 + s];
            if (r.nan_count[ch] < r.pixels) {  // some non-NaN pixel: the keys hold its range
                r.min[ch] = key_value(res[s]);
                r.max[ch] = key_value(res[4 + s]);
            }
            if (hist)
                for (int b = 0; b < 256; ++b) r.histogram[ch][b] = res[16 + 256 * s + b];
        }
    }
    *out = r;
    return KC_OK;
}

}  // namespace kc
