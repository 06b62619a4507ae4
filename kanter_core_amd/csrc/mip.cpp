// Mip chains and their export (include/kanter_core_amd.h): kc_mip_level_count, kc_preview_level, kc_image_build_mips,
// kc_image_build_roughness_mips, kc_bc_mip_layout, kc_image_to_bc_mips, kc_image_to_bc_mips_device, kc_image_levels_to_bc_mips,
// kc_dds_header, kc_image_write_dds, kc_image_levels_write_dds.  The host side does the level arithmetic,
// folds constant planes with the device's expression, allocates the level planes and enqueues mip.hip's kernels on the library's
// stream: the pyramid kernel while both extents still halve (up to six levels per launch), the one-level kernel for the rest and
// for every level under KC_MIP_PER_LEVEL; under KC_MIP_NORMALS mip_normals.hip's two kernels take R, G, B together and
// renormalise every level; under KC_MIP_COVERAGE mip_coverage.hip's select and scale give alpha planes of their own; under
// KC_MIP_ALPHA_WEIGHT mip_alpha.hip's pull and push give colour planes of their own, level 0 included; a roughness
// chain is mip_roughness.hip's two kernels on the vector of a normal map and the roughness plane together.  The BC chain
// is bc.cpp's encoder launch once per level; the DDS writer is host code.
#include <cmath>
#include <cstdio>
#include <limits>

#include "kc_runtime.hpp"

namespace kc {

static int mip_refuse(const char *who, const char *what)
{
    set_error(std::string(who) + ": " + what);
    return KC_ERR_INVALID_ARG;
}

static uint32_t floor_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }  // v > 0

int mip_level_count(uint32_t w, uint32_t h, uint32_t *levels)
{
    if (!levels || w == 0 || h == 0) return mip_refuse("kc_mip_level_count", "NULL output or zero extent");
    *levels = 1u + floor_log2(w > h ? w : h);
    return KC_OK;
}

static uint32_t level_extent(uint32_t v, uint32_t k) { return k < 32 && (v >> k) ? v >> k : 1u; }

int preview_level(uint32_t w, uint32_t h, uint32_t max_extent, uint32_t *level, uint32_t *pw, uint32_t *ph)
{
    if (!level || !pw || !ph || w == 0 || h == 0 || max_extent == 0)
        return mip_refuse("kc_preview_level", "NULL output, zero size or zero extent");
    uint32_t k = 0;
    while ((w > h ? w : h) >> k > max_extent) ++k;  // max_extent >= 1: ends at the 1 x 1 level at the latest
    *level = k;
    *pw = level_extent(w, k);
    *ph = level_extent(h, k);
    return KC_OK;
}

// The contract's expression on a constant plane, once per level: ((c + c) + (c + c)) * 0.25f in f32.  It is not c for very
// large c (c + c overflows) or denormal c (the product rounds), so nothing is shortcut; the volatile temporaries keep the
// compiler from folding or contracting the four operations differently from the device.
float mip_const_fold(float c)
{
    volatile float a = c;
    volatile float s = a + a;
    volatile float t = s + s;
    volatile float q = 0.25f;
    volatile float r = t * q;
    return r;
}

// KC_MIP_NORMALS on one texel, from the boxes of R, G, B to the stored values: the device's expression (mip_normals.hip) with
// the host's correctly rounded sqrtf and /, every operation through a volatile temporary like mip_const_fold.  This is
// kc_mip_normal_texel and what folds an image whose R, G, B are all constant.
void mip_normal_texel(const float box[3], float out[3])
{
    volatile float v[3], u[3] = { 0.0f, 0.0f, 1.0f };
    volatile float two = 2.0f, one = 1.0f, half = 0.5f;
    for (int c = 0; c < 3; ++c) {
        volatile float m = box[c] * two;
        v[c] = m - one;
    }
    volatile float xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
    volatile float xy = xx + yy;
    volatile float q = xy + zz;
    volatile float l = std::sqrt((float)q);
    if (l > 0.0f && l < std::numeric_limits<float>::infinity())  // false for NaN
        for (int c = 0; c < 3; ++c) u[c] = v[c] / l;
    for (int c = 0; c < 3; ++c) {
        volatile float m = u[c] * half;
        out[c] = m + half;
    }
}

// ---------------------------------------------------------------- roughness chains: the rule's arithmetic
// Level 0 of the normals on one texel, from the stored R, G, B to the unit vector: the device's expression (mip_roughness.hip,
// unit_normal), every operation through a volatile temporary like mip_const_fold.  This is kc_mip_unit_normal.
void mip_unit_normal(const float rgb[3], float u[3])
{
    volatile float v[3];
    volatile float two = 2.0f, one = 1.0f;
    for (int c = 0; c < 3; ++c) {
        volatile float m = rgb[c] * two;
        v[c] = m - one;
    }
    volatile float xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
    volatile float xy = xx + yy;
    volatile float q = xy + zz;
    volatile float l = std::sqrt((float)q);
    const bool ok = l > 0.0f && l < std::numeric_limits<float>::infinity();  // false for NaN
    for (int c = 0; c < 3; ++c) {
        volatile float d = ok ? v[c] / l : (c == 2 ? 1.0f : 0.0f);
        u[c] = d;
    }
}

// rough(m, r, power) of the header, the stored texel of a level >= 1: the device's expression (mip_roughness.hip, rough_texel)
// likewise.  This is kc_mip_roughness_texel.
float mip_roughness_texel(const float m[3], float r, float power)
{
    if (r != r) return r;
    volatile float xx = m[0] * m[0], yy = m[1] * m[1], zz = m[2] * m[2];
    volatile float xy = xx + yy;
    volatile float q = xy + zz;
    volatile float l = std::sqrt((float)q);
    if (l == 0.0f) return 1.0f;
    volatile float one = 1.0f, floor = 0x1p-14f, two = 2.0f;
    volatile float s = one - l;
    volatile float t = s / l;
    if (!(t > floor)) return r;
    volatile float te = t - floor;
    volatile float rc = std::fmin(std::fmax(r, 0.0f), 1.0f);
    volatile float a = rc * rc;
    volatile float a2 = a * a;
    volatile float te2 = two * te;
    volatile float tp = te2 * power;
    volatile float am = a2 - one;
    volatile float B = tp * am;
    volatile float num = B - a2, den = B - one;
    volatile float n = num / den;
    volatile float h = std::sqrt((float)n);
    volatile float d = std::sqrt((float)h);
    return d;
}

// ---------------------------------------------------------------- KC_MIP_ALPHA_WEIGHT: the rule's arithmetic
// w0 of an alpha: the device's expression (mip_alpha.hip, alpha_weight).  This is kc_mip_alpha_weight.
float mip_alpha_weight(float a)
{
    if (!(a > 0.0f)) return 0.0f;  // NaN, -0.0 and negatives
    return a < 1.0f ? a : 1.0f;
}

// q = P / W of a texel of a level >= 1, known where W > 0 (false for NaN), q = 0 elsewhere: the device's expression
// (mip_alpha.hip, alpha_texel), the host's correctly rounded divide through a volatile temporary like mip_const_fold.  This is
// kc_mip_alpha_texel and what folds an image of four constant planes.
bool mip_alpha_texel(const float p[3], float w, float q[3])
{
    const bool known = w > 0.0f;
    for (int c = 0; c < 3; ++c) {
        volatile float n = p[c], d = w;
        volatile float r = known ? n / d : 0.0f;
        q[c] = r;
    }
    return known;
}

// the flag's own refusal: a vector is not a colour
static int mip_check_alpha_flags(uint32_t flags, const char *who)
{
    if ((flags & KC_MIP_ALPHA_WEIGHT) && (flags & KC_MIP_NORMALS)) {
        set_error(std::string(who) + ": KC_MIP_NORMALS with KC_MIP_ALPHA_WEIGHT");
        return KC_ERR_UNSUPPORTED;
    }
    return KC_OK;
}

// ---------------------------------------------------------------- KC_MIP_COVERAGE: the rule's arithmetic
static constexpr uint32_t kCoverageFlagBits = KC_MIP_COVERAGE | 0xff000000u;

int mip_check_coverage_flags(uint32_t flags, const char *who)
{
    const uint32_t ref = flags >> 24;
    // a byte if and only if coverage or punch-through: where KC_BC_PUNCH_THROUGH is not accepted it has been refused as an unknown bit
    if ((flags & KC_MIP_COVERAGE) ? ref == 0 : (ref != 0 && !(flags & KC_BC_PUNCH_THROUGH))) {
        set_error(std::string(who) + ": KC_MIP_COVERAGE goes with a reference byte 1..255 in bits 24-31 (KC_MIP_COVERAGE_REF)");
        return KC_ERR_UNSUPPORTED;
    }
    return KC_OK;
}

// r_B = (float)B / 255.0f, one IEEE divide: the smallest f32 that quant_u8 takes to at least B
float alpha_ref_threshold(uint32_t ref_u8)
{
    volatile float b = (float)ref_u8, d = 255.0f;
    volatile float r = b / d;
    return r;
}

// T_k of n_k texels for c_0 covered of n_0 (n_0 <= 2^31: the product fits 64 bits)
static uint64_t coverage_target(uint64_t n_0, uint64_t n_k, uint64_t c_0)
{
    if (c_0 == 0) return 0;
    const uint64_t t = (c_0 * n_k + n_0 / 2) / n_0;
    return std::min(n_k, std::max<uint64_t>(t, 1));
}

int mip_coverage_target(uint32_t w, uint32_t h, uint64_t covered0, uint32_t level, uint64_t *target)
{
    const char *who = "kc_mip_coverage_target";
    if (!target || w == 0 || h == 0) return mip_refuse(who, "NULL output or zero extent");
    const uint64_t n_0 = (uint64_t)w * h;
    if (n_0 > (1ull << 31)) return mip_refuse(who, "image too large");
    if (covered0 > n_0 || level >= 1u + floor_log2(w > h ? w : h)) return mip_refuse(who, "covered0 above the texels, or level at or above the level count");
    *target = level == 0 ? covered0 : coverage_target(n_0, (uint64_t)level_extent(w, level) * level_extent(h, level), covered0);
    return KC_OK;
}

// s_k from v_k: the device's expression (mip_coverage.hip, coverage_scale), every operation through a volatile temporary like
// mip_const_fold.  ve >= 2^-16 keeps r_B / ve finite; the loop ends because ve * s grows with s.
float mip_coverage_scale(float v, uint32_t ref_u8)
{
    volatile float ve = v > 0x1p-16f ? v : 0x1p-16f;  // NaN takes the floor too
    volatile float s = alpha_ref_threshold(ref_u8) / ve;
    for (;;) {
        volatile float m = ve * s;
        if (quant_u8_host(m) >= ref_u8) return s;
        s = std::nextafter((float)s, std::numeric_limits<float>::infinity());
    }
}

namespace {
// The distinct resident planes of an image: slot s reads src[s]; slot_of[ch] = the slot of channel ch, -1 for a constant
struct MipSlots {
    const kc_plane *src[4];
    int n = 0;
    int slot_of[4] = { -1, -1, -1, -1 };
    void add(int ch, const kc_plane *p)
    {
        if (p->kind == kc_plane::CONST) return;
        int s = 0;
        while (s < n && !(src[s] == p || (src[s]->dptr == p->dptr && src[s]->pitch == p->pitch))) ++s;
        if (s == n) src[n++] = p;
        slot_of[ch] = s;
    }
};

struct MipChain {
    std::vector<kc_plane *> planes;  // [level - 1][channel], one reference each held here until the images exist
    std::vector<kc_plane *> scratch;  // planes no level image keeps (KC_MIP_COVERAGE: a plain alpha nothing else aliases)
    ~MipChain()
    {
        for (kc_plane *p : planes) plane_release(p);
        for (kc_plane *p : scratch) plane_release(p);
    }
};
}  // namespace

// The level walk of a chain of L levels of a w x h image, for both families: launch(k, sw, sh, fused, nt) enqueues the launch
// that reads level k (sw x sh) and writes `fused` levels with the pyramid kernel -- as many as both extents still halve, six at
// the most -- or, with fused == 0, one level with the one-level kernel: after an extent has reached 1, and at every level under
// KC_MIP_PER_LEVEL.  nt is the cache policy of a launch that reads in_planes(k) planes and writes out_planes per level.
template <class Planes, class Launch>
static int mip_walk(Context &c, uint32_t w, uint32_t h, uint32_t L, bool per_level, uint32_t out_planes, Planes in_planes, Launch launch)
{
    for (uint32_t k = 0; k + 1 < L;) {  // k: the level the next launch reads
        const uint32_t sw = level_extent(w, k), sh = level_extent(h, k);
        const uint32_t small = sw < sh ? sw : sh;
        const uint32_t fused = per_level || small < 2 ? 0u : floor_log2(small) < 6u ? floor_log2(small) : 6u;
        const uint32_t n_src = in_planes(k);
        const uint64_t in_bytes = (uint64_t)sw * sh * 4 * n_src;
        const uint64_t out_bytes = (uint64_t)level_extent(w, k + 1) * level_extent(h, k + 1) * 4 * out_planes;
        const bool nt = (cache_policy_mask(in_bytes, out_bytes, n_src) & 0xffu) != 0;
        KC_TRY(launch(k, sw, sh, fused, nt));
        if (nt) c.counters["mip_nt"]++;
        c.launches++;
        k += fused ? fused : 1u;
    }
    return KC_OK;
}

// The plain rule's launches for the resident planes of sl: level k of slot s is slot_planes[(k - 1) * 4 + s]
static int mip_launch_plain(Context &c, const MipSlots &sl, const std::vector<kc_plane *> &slot_planes, uint32_t w, uint32_t h, uint32_t L,
                            bool per_level)
{
    if (sl.n == 0 || L < 2) return KC_OK;
    auto plane_at = [&](uint32_t k, int s) -> const kc_plane * { return k == 0 ? sl.src[s] : slot_planes[(size_t)(k - 1) * 4 + s]; };
    auto pitch_at = [&](uint32_t k) { return (uint32_t)(plane_at(k, 0)->pitch / sizeof(float)); };
    auto fill = [&](auto &a, uint32_t k, uint32_t sw, uint32_t sh) {  // the source side of a launch that reads level k
        a.w = sw;
        a.h = sh;
        for (int s = 0; s < sl.n; ++s) {
            a.src[s] = plane_at(k, s)->dptr;
            a.src_pitch[s] = (uint32_t)(plane_at(k, s)->pitch / sizeof(float));
        }
    };
    KC_TRY(mip_walk(c, w, h, L, per_level, (uint32_t)sl.n, [&](uint32_t) { return (uint32_t)sl.n; },
                    [&](uint32_t k, uint32_t sw, uint32_t sh, uint32_t fused, bool nt) {
        if (fused) {
            MipPyramidArgs a{};
            fill(a, k, sw, sh);
            a.n = fused;
            for (uint32_t j = 0; j < fused; ++j) {
                for (int s = 0; s < sl.n; ++s) a.dst[s][j] = plane_at(k + 1 + j, s)->dptr;
                a.dst_pitch[j] = pitch_at(k + 1 + j);
            }
            hipError_t e = launch_mip_pyramid(a, (uint32_t)sl.n, nt, c.stream);
            if (e != hipSuccess) return hip_fail(e, "launch_mip_pyramid");
            c.counters["mip_pyramid"]++;
        } else {
            MipLevelArgs a{};
            fill(a, k, sw, sh);
            for (int s = 0; s < sl.n; ++s) a.dst[s] = plane_at(k + 1, s)->dptr;
            a.dst_pitch = pitch_at(k + 1);
            hipError_t e = launch_mip_level(a, (uint32_t)sl.n, nt, c.stream);
            if (e != hipSuccess) return hip_fail(e, "launch_mip_level");
            c.counters["mip_level"]++;
        }
        return (int)KC_OK;
    }));
    uint64_t texels = (uint64_t)w * h;  // level 0 read once, every further level written once
    for (uint32_t j = 1; j < L; ++j) texels += (uint64_t)level_extent(w, j) * level_extent(h, j);
    c.alg_bytes += 4 * texels * sl.n;
    return KC_OK;
}

// KC_MIP_NORMALS: the coupled launches for R, G, B (rgb[c]: the channel's plane at level 0, at least one of them resident; sl:
// its distinct resident planes); level k of channel c is rgb_planes[(k - 1) * 3 + c], resident at every level
static int mip_launch_normals(Context &c, const kc_plane *const rgb[3], const MipSlots &sl, const std::vector<kc_plane *> &rgb_planes,
                              uint32_t w, uint32_t h, uint32_t L, bool per_level)
{
    if (L < 2) return KC_OK;
    // level 0: constants, and channels that read an earlier channel's plane; below it every channel has a plane of its own
    uint32_t const_mask = 0, from = 0;
    for (int ch = 0; ch < 3; ++ch) {
        int f = ch;
        if (sl.slot_of[ch] < 0) const_mask |= 1u << ch;
        else
            for (int e = ch - 1; e >= 0; --e)
                if (sl.slot_of[e] == sl.slot_of[ch]) f = e;
        from |= (uint32_t)f << (2 * ch);
    }
    auto fill = [&](auto &a, uint32_t k, uint32_t sw, uint32_t sh) {  // the source side of a launch that reads level k
        a.w = sw;
        a.h = sh;
        for (int ch = 0; ch < 3; ++ch) {
            const kc_plane *p = k == 0 ? rgb[ch] : rgb_planes[(size_t)(k - 1) * 3 + ch];
            const bool is_const = k == 0 && ((const_mask >> ch) & 1u);
            a.src[ch] = is_const ? nullptr : p->dptr;
            a.src_pitch[ch] = is_const ? 0u : (uint32_t)(p->pitch / sizeof(float));
            a.cval[ch] = is_const ? p->cval : 0.0f;
        }
        a.const_mask = k == 0 ? const_mask : 0u;
        a.from = k == 0 ? from : (0u | 1u << 2 | 2u << 4);
    };
    KC_TRY(mip_walk(c, w, h, L, per_level, 3u, [&](uint32_t k) { return k == 0 ? (uint32_t)sl.n : 3u; },
                    [&](uint32_t k, uint32_t sw, uint32_t sh, uint32_t fused, bool nt) {
        if (fused) {
            NormalPyramidArgs a{};
            fill(a, k, sw, sh);
            a.n = fused;
            for (uint32_t j = 0; j < fused; ++j) {
                for (int ch = 0; ch < 3; ++ch) a.dst[ch][j] = rgb_planes[(size_t)(k + j) * 3 + ch]->dptr;
                a.dst_pitch[j] = (uint32_t)(rgb_planes[(size_t)(k + j) * 3]->pitch / sizeof(float));
            }
            hipError_t e = launch_normal_pyramid(a, nt, c.stream);
            if (e != hipSuccess) return hip_fail(e, "launch_normal_pyramid");
            c.counters["mip_normals_pyramid"]++;
        } else {
            NormalLevelArgs a{};
            fill(a, k, sw, sh);
            for (int ch = 0; ch < 3; ++ch) a.dst[ch] = rgb_planes[(size_t)k * 3 + ch]->dptr;
            a.dst_pitch = (uint32_t)(rgb_planes[(size_t)k * 3]->pitch / sizeof(float));
            hipError_t e = launch_normal_level(a, nt, c.stream);
            if (e != hipSuccess) return hip_fail(e, "launch_normal_level");
            c.counters["mip_normals_level"]++;
        }
        return (int)KC_OK;
    }));
    uint64_t written = 0;  // every distinct resident plane of level 0 read once, three planes of every further level written once
    for (uint32_t j = 1; j < L; ++j) written += (uint64_t)level_extent(w, j) * level_extent(h, j);
    c.alg_bytes += 4 * (uint64_t)w * h * sl.n + 12 * written;
    return KC_OK;
}

// kc_image_build_roughness_mips: the coupled launches for the vector of the normals and the roughness (src0: X, Y, Z of the
// normal map and the roughness plane at level 0, constant or resident, at least one of the first three resident); level k's
// stored plane is dst_planes[k - 1].  The four plain boxes of the last level a launch writes are the next launch's sources:
// state planes from the pool, held in mc.scratch until the call returns (everything that reads them is enqueued by then).
static int mip_launch_roughness(Context &c, const kc_plane *const src0[4], const std::vector<kc_plane *> &dst_planes, MipChain &mc, float power,
                                uint32_t w, uint32_t h, uint32_t L, bool per_level)
{
    if (L < 2) return KC_OK;
    MipSlots sl;  // the distinct resident planes of level 0
    uint32_t const_mask = 0;
    for (int ch = 0; ch < 4; ++ch) {
        sl.add(ch, src0[ch]);
        if (sl.slot_of[ch] < 0) const_mask |= 1u << ch;
    }
    const kc_plane *state[4] = { nullptr, nullptr, nullptr, nullptr };  // of the level the next launch reads
    uint64_t state_texels = 0;
    auto fill = [&](auto &a, uint32_t k, uint32_t sw, uint32_t sh, uint32_t last) -> int {  // a launch that reads level k and ends at `last`
        a.w = sw;
        a.h = sh;
        a.power = power;
        for (int ch = 0; ch < 4; ++ch) {
            const kc_plane *p = k == 0 ? src0[ch] : state[ch];
            const bool is_const = k == 0 && ((const_mask >> ch) & 1u);
            a.src[ch] = is_const ? nullptr : p->dptr;
            a.src_pitch[ch] = is_const ? 0u : (uint32_t)(p->pitch / sizeof(float));
            a.cval[ch] = is_const ? p->cval : 0.0f;
        }
        a.const_mask = k == 0 ? const_mask : 0u;
        for (int ch = 0; ch < 4; ++ch) {
            state[ch] = nullptr;
            a.state[ch] = nullptr;
        }
        if (last + 1 < L) {  // more levels follow
            const uint32_t W = level_extent(w, last), H = level_extent(h, last);
            for (int ch = 0; ch < 4; ++ch) {
                kc_plane *p = nullptr;
                KC_TRY(plane_new_mem(W, H, &p));
                mc.scratch.push_back(p);
                if (p->pitch != dst_planes[last - 1]->pitch) return mip_refuse("kc_image_build_roughness_mips", "planes of one size differ in pitch");
                state[ch] = p;
                a.state[ch] = p->dptr;
            }
            state_texels += (uint64_t)W * H;
        }
        return KC_OK;
    };
    KC_TRY(mip_walk(c, w, h, L, per_level, 1u, [&](uint32_t k) { return k == 0 ? (uint32_t)sl.n : 4u; },
                    [&](uint32_t k, uint32_t sw, uint32_t sh, uint32_t fused, bool nt) {
        if (fused) {
            RoughnessPyramidArgs a{};
            KC_TRY(fill(a, k, sw, sh, k + fused));
            a.n = fused;
            for (uint32_t j = 0; j < fused; ++j) {
                a.dst[j] = dst_planes[k + j]->dptr;
                a.dst_pitch[j] = (uint32_t)(dst_planes[k + j]->pitch / sizeof(float));
            }
            hipError_t e = launch_roughness_pyramid(a, k == 0, nt, c.stream);
            if (e != hipSuccess) return hip_fail(e, "launch_roughness_pyramid");
            c.counters["mip_roughness_pyramid"]++;
        } else {
            RoughnessLevelArgs a{};
            KC_TRY(fill(a, k, sw, sh, k + 1));
            a.dst = dst_planes[k]->dptr;
            a.dst_pitch = (uint32_t)(dst_planes[k]->pitch / sizeof(float));
            hipError_t e = launch_roughness_level(a, k == 0, nt, c.stream);
            if (e != hipSuccess) return hip_fail(e, "launch_roughness_level");
            c.counters["mip_roughness_level"]++;
        }
        return (int)KC_OK;
    }));
    // every distinct resident plane of level 0 read once, one plane of every further level written once, the four state planes
    // of a level written once and read once
    uint64_t written = 0;
    for (uint32_t j = 1; j < L; ++j) written += (uint64_t)level_extent(w, j) * level_extent(h, j);
    c.alg_bytes += 4 * (uint64_t)w * h * sl.n + 4 * written + 32 * state_texels;
    return KC_OK;
}

// KC_MIP_ALPHA_WEIGHT: the pull launches for the premultiplied colour and the weight (src0: R, G, B, alpha at level 0, constant
// or resident, the colours or alpha resident) and the push launch over all levels; level k's colour planes are col[3 k + c],
// level 0 included.  The weight of every level >= 1 lives in a scratch plane, and P_c of the last level a launch writes in
// three state planes that the next launch reads: all from the pool, held in mc.scratch until the call returns (everything
// that reads them is enqueued by then).
static int mip_launch_alpha(Context &c, const kc_plane *const src0[4], const std::vector<kc_plane *> &col, MipChain &mc, uint32_t w, uint32_t h,
                            uint32_t L, bool per_level)
{
    const char *who = "kc_image_build_mips";
    if (L > KC_ALPHA_MAX_LEVELS) return mip_refuse("KC_MIP_ALPHA_WEIGHT", "more levels than the job table holds");
    MipSlots sl;  // the distinct resident planes of level 0
    uint32_t const_mask = 0;
    for (int ch = 0; ch < 4; ++ch) {
        sl.add(ch, src0[ch]);
        if (sl.slot_of[ch] < 0) const_mask |= 1u << ch;
    }
    auto pitch_of = [](const kc_plane *p) { return (uint32_t)(p->pitch / sizeof(float)); };
    std::vector<kc_plane *> weight(L, nullptr);  // [level], levels >= 1
    for (uint32_t k = 0; k < L; ++k) {
        if (k) {
            KC_TRY(plane_new_mem(level_extent(w, k), level_extent(h, k), &weight[k]));
            mc.scratch.push_back(weight[k]);
        }
        for (int ch = 0; ch < 3; ++ch)
            if (col[3 * k + ch]->pitch != (k ? weight[k] : col[0])->pitch) return mip_refuse(who, "planes of one size differ in pitch");
    }
    const kc_plane *state[3] = { nullptr, nullptr, nullptr };  // of the level the next launch reads
    uint64_t state_texels = 0;
    auto fill = [&](auto &a, uint32_t k, uint32_t sw, uint32_t sh, uint32_t last) -> int {  // a launch that reads level k and ends at `last`
        a.w = sw;
        a.h = sh;
        for (int ch = 0; ch < 4; ++ch) {
            const kc_plane *p = k == 0 ? src0[ch] : ch < 3 ? state[ch] : weight[k];
            const bool is_const = k == 0 && ((const_mask >> ch) & 1u);
            a.src[ch] = is_const ? nullptr : p->dptr;
            a.src_pitch[ch] = is_const ? 0u : pitch_of(p);
            a.cval[ch] = is_const ? p->cval : 0.0f;
        }
        a.const_mask = k == 0 ? const_mask : 0u;
        for (int ch = 0; ch < 3; ++ch) {
            a.dst0[ch] = k == 0 ? col[ch]->dptr : nullptr;
            state[ch] = nullptr;
            a.state[ch] = nullptr;
        }
        a.dst0_pitch = k == 0 ? pitch_of(col[0]) : 0u;
        if (last + 1 < L && last > k) {  // more levels follow
            const uint32_t W = level_extent(w, last), H = level_extent(h, last);
            for (int ch = 0; ch < 3; ++ch) {
                kc_plane *p = nullptr;
                KC_TRY(plane_new_mem(W, H, &p));
                mc.scratch.push_back(p);
                if (p->pitch != weight[last]->pitch) return mip_refuse(who, "planes of one size differ in pitch");
                state[ch] = p;
                a.state[ch] = p->dptr;
            }
            state_texels += (uint64_t)W * H;
        }
        return KC_OK;
    };
    if (L == 1) {  // a 1 x 1 image: no level to pull, level 0's colour alone
        AlphaPullLevelArgs a{};
        KC_TRY(fill(a, 0, w, h, 0));
        hipError_t e = launch_alpha_pull_level(a, true, false, c.stream);
        if (e != hipSuccess) return hip_fail(e, "launch_alpha_pull_level");
        c.counters["mip_alpha_pull_level"]++;
        c.launches++;
    }
    KC_TRY(mip_walk(c, w, h, L, per_level, 4u, [&](uint32_t k) { return k == 0 ? (uint32_t)sl.n : 4u; },
                    [&](uint32_t k, uint32_t sw, uint32_t sh, uint32_t fused, bool nt) {
        if (fused) {
            AlphaPullPyramidArgs a{};
            KC_TRY(fill(a, k, sw, sh, k + fused));
            a.n = fused;
            for (uint32_t j = 0; j < fused; ++j) {
                for (int ch = 0; ch < 3; ++ch) a.dst[ch][j] = col[3 * (k + 1 + j) + ch]->dptr;
                a.wdst[j] = weight[k + 1 + j]->dptr;
                a.dst_pitch[j] = pitch_of(weight[k + 1 + j]);
            }
            hipError_t e = launch_alpha_pull_pyramid(a, k == 0, nt, c.stream);
            if (e != hipSuccess) return hip_fail(e, "launch_alpha_pull_pyramid");
            c.counters["mip_alpha_pull_pyramid"]++;
        } else {
            AlphaPullLevelArgs a{};
            KC_TRY(fill(a, k, sw, sh, k + 1));
            for (int ch = 0; ch < 3; ++ch) a.dst[ch] = col[3 * (k + 1) + ch]->dptr;
            a.wdst = weight[k + 1]->dptr;
            a.dst_pitch = pitch_of(weight[k + 1]);
            hipError_t e = launch_alpha_pull_level(a, k == 0, nt, c.stream);
            if (e != hipSuccess) return hip_fail(e, "launch_alpha_pull_level");
            c.counters["mip_alpha_pull_level"]++;
        }
        return (int)KC_OK;
    }));
    AlphaPushArgs pa{};
    uint32_t wgs = 0;
    uint64_t below = 0;  // the texels of the levels >= 1
    for (uint32_t k = 0; k < L; ++k) {
        AlphaPushJob &J = pa.jobs[k];
        for (int ch = 0; ch < 3; ++ch) J.dst[ch] = col[3 * k + ch]->dptr;
        J.dst_pitch = pitch_of(col[3 * k]);
        const kc_plane *ws = k ? weight[k] : (const_mask & 8u) ? nullptr : src0[3];
        J.wsrc = ws ? ws->dptr : nullptr;
        J.w_pitch = ws ? pitch_of(ws) : 0u;
        J.w = level_extent(w, k);
        J.h = level_extent(h, k);
        J.first_wg = wgs;
        J.wgs = alpha_push_job_wgs(J.w, J.h);
        wgs += J.wgs;
        if (k) below += (uint64_t)J.w * J.h;
    }
    pa.levels = L;
    hipError_t e = launch_alpha_push(pa, wgs, c.stream);
    if (e != hipSuccess) return hip_fail(e, "launch_alpha_push");
    c.counters["mip_alpha_push"]++;
    c.launches++;
    // the pull: every distinct resident plane of level 0 read once, level 0's three colour planes written, three colours and the
    // weight of every further level written, the three state planes of a level written and read and its weight read; the push:
    // level 0's alpha where it is resident and every weight read (what it writes depends on the data and is not counted)
    const uint64_t n0 = (uint64_t)w * h;
    c.alg_bytes += 4 * n0 * sl.n + 12 * n0 + 16 * below + 28 * state_texels + ((const_mask & 8u) ? 0 : 4 * n0) + 4 * below;
    return KC_OK;
}

// KC_MIP_COVERAGE: the select over alpha's plain chain (plain[k]: p_k, plain[0] the image's alpha; L levels of a w x h image,
// w h <= 2^31) and, with `scaled` (scaled[k - 1]: d_k), the scale launch.  The records and the histograms live in
// `scratch`, which the caller gives back to the pool once everything that reads it is enqueued (or waited for); *rec = the L
// device records.  Launches: a count and a pick per pass, three passes when there is a level >= 1, and the scale.
static int coverage_enqueue(Context &c, const std::vector<const kc_plane *> &plain, const std::vector<kc_plane *> *scaled, uint32_t w, uint32_t h,
                            uint32_t L, uint32_t ref, PoolStaging &scratch, CoverageRecord **rec)
{
    if (L > KC_COVERAGE_MAX_LEVELS) return mip_refuse("KC_MIP_COVERAGE", "more levels than the job table holds");
    const size_t rec_bytes = ((size_t)L * sizeof(CoverageRecord) + 255) / 256 * 256, hist_bytes = (size_t)L * KC_COVERAGE_BINS * sizeof(uint32_t);
    KC_TRY(scratch.alloc(rec_bytes + hist_bytes));
    CoverageArgs a{};
    uint32_t wgs = 0;
    uint64_t below = 0;  // the texels of the levels >= 1
    for (uint32_t k = 0; k < L; ++k) {
        CoverageJob &J = a.jobs[k];
        J.src = plain[k]->dptr;
        J.src_pitch = (uint32_t)(plain[k]->pitch / sizeof(float));
        J.dst = scaled && k ? (*scaled)[k - 1]->dptr : nullptr;
        J.dst_pitch = scaled && k ? (uint32_t)((*scaled)[k - 1]->pitch / sizeof(float)) : 0u;
        J.w = level_extent(w, k);
        J.h = level_extent(h, k);
        J.first_wg = wgs;
        J.wgs = coverage_job_wgs(J.w, J.h);
        wgs += J.wgs;
        if (k) below += (uint64_t)J.w * J.h;
    }
    const uint32_t wgs0 = a.jobs[0].wgs;
    a.rec = (CoverageRecord *)scratch.ptr;
    a.hist = (uint32_t *)((char *)scratch.ptr + rec_bytes);
    a.levels = L;
    a.ref = ref;
    a.r_b = alpha_ref_threshold(ref);
    KC_HIP(hipMemsetAsync(scratch.ptr, 0, rec_bytes + hist_bytes, c.stream));
    uint32_t launches = 0;
    for (uint32_t pass = 0; pass < (L > 1 ? 3u : 1u); ++pass) {
        hipError_t e = pass == 0 ? launch_coverage_count(a, 0, 0, wgs, c.stream) : launch_coverage_count(a, pass, wgs0, wgs - wgs0, c.stream);
        if (e != hipSuccess) return hip_fail(e, "launch_coverage_count");
        e = launch_coverage_pick(a, pass, c.stream);
        if (e != hipSuccess) return hip_fail(e, "launch_coverage_pick");
        launches += 2;
    }
    uint64_t texels = (uint64_t)w * h + 3 * below;  // level 0 once, every further level once per pass
    if (scaled && L > 1) {
        hipError_t e = launch_coverage_scale(a, wgs0, wgs - wgs0, c.stream);
        if (e != hipSuccess) return hip_fail(e, "launch_coverage_scale");
        launches++;
        texels += 2 * below;  // read once more, written once
    }
    c.launches += launches;
    c.counters["mip_coverage"] += launches;
    c.alg_bytes += 4 * texels;
    *rec = a.rec;
    return KC_OK;
}

// the kernels' indices are 32-bit and the pyramid's tile rows a grid dimension
static bool mip_size_ok(uint32_t w, uint32_t h)
{
    return !(w > (1u << 30) || ((uint64_t)h + 63) / 64 > 65535ull || (((uint64_t)w + 3) / 4) * h > (1ull << 31));
}

// KC_MIP_ALPHA_WEIGHT on a forced RGBA image whose alpha is not a constant >= 1: levels[0] is an image of its own -- new colour
// planes beside img's alpha -- and every further level has new colour planes.  A constant alpha of weight 0 gives constant-zero
// colour, four constants are folded here through mip_alpha_texel (pull, then push from the last level up; every texel of a
// level is the same), everything else goes through mip_launch_alpha.  Alpha itself is placed exactly as image_build_mips
// places it: folded, or the plain launches and KC_MIP_COVERAGE's planes.
static int image_build_alpha_mips(Context &c, kc_image *img, uint32_t ref, bool per_level, kc_image **levels, uint32_t w, uint32_t h, uint32_t L)
{
    const kc_plane *A = img->planes[3];
    const bool a_const = A->kind == kc_plane::CONST;
    const float w0 = a_const ? mip_alpha_weight(A->cval) : 0.0f;
    const bool zero = a_const && !(w0 > 0.0f);
    const bool fold = !zero && a_const && img->planes[0]->kind == kc_plane::CONST && img->planes[1]->kind == kc_plane::CONST &&
                      img->planes[2]->kind == kc_plane::CONST;
    MipChain mc;  // planes: one reference per plane of the level images, in no particular order
    mc.planes.reserve((size_t)L * 4);
    // alpha: alpha_out[k] is the plane of level k's image
    MipSlots sl;
    sl.add(3, A);
    std::vector<kc_plane *> slot_planes(L > 1 ? (size_t)(L - 1) * 4 : 0, nullptr), alpha_out(L, img->planes[3]);
    const bool coverage = ref != 0 && !a_const && L > 1;
    std::vector<kc_plane *> scaled(coverage ? L - 1 : 0, nullptr);
    float av = A->cval;
    for (uint32_t k = 1; k < L; ++k) {
        const uint32_t W = level_extent(w, k), H = level_extent(h, k);
        kc_plane *p = nullptr;
        if (a_const) {
            av = mip_const_fold(av);
            p = plane_new_const(W, H, av);
        } else {
            KC_TRY(plane_new_mem(W, H, &p));
            slot_planes[(size_t)(k - 1) * 4] = p;
            if (coverage) {
                mc.scratch.push_back(p);
                p = nullptr;
                KC_TRY(plane_new_mem(W, H, &p));
                scaled[k - 1] = p;
            }
        }
        mc.planes.push_back(p);
        alpha_out[k] = p;
    }
    // colour: col[3 k + ch], level 0 included
    std::vector<kc_plane *> col((size_t)L * 3, nullptr);
    std::vector<float> folded((size_t)L * 3, 0.0f);
    if (fold) {
        float P[3], W = w0;
        std::vector<char> known(L, 1);
        for (int ch = 0; ch < 3; ++ch) {
            volatile float v = img->planes[ch]->cval, m = v * W;  // w0 > 0: the product
            P[ch] = m;
            folded[ch] = img->planes[ch]->cval;  // level 0 is known: c itself
        }
        for (uint32_t k = 1; k < L; ++k) {
            for (int ch = 0; ch < 3; ++ch) P[ch] = mip_const_fold(P[ch]);
            W = mip_const_fold(W);
            known[k] = mip_alpha_texel(P, W, &folded[3 * k]);
        }
        for (uint32_t k = L - 1; k >= 1; --k)  // the push; an unknown last level keeps its 0
            if (!known[k] && k + 1 < L)
                for (int ch = 0; ch < 3; ++ch) folded[3 * k + ch] = folded[3 * (k + 1) + ch];
    }
    for (uint32_t k = 0; k < L; ++k) {
        const uint32_t W = level_extent(w, k), H = level_extent(h, k);
        for (int ch = 0; ch < 3; ++ch) {
            kc_plane *p = nullptr;
            if (zero || fold) p = plane_new_const(W, H, folded[3 * k + ch]);
            else KC_TRY(plane_new_mem(W, H, &p));
            mc.planes.push_back(p);
            col[3 * k + ch] = p;
        }
    }
    if (!zero && !fold) KC_TRY(mip_launch_alpha(c, img->planes, col, mc, w, h, L, per_level));
    KC_TRY(mip_launch_plain(c, sl, slot_planes, w, h, L, per_level));
    PoolStaging coverage_scratch;  // back to the pool when the call returns: everything that reads it is enqueued by then
    if (coverage) {
        std::vector<const kc_plane *> plain(L, img->planes[3]);
        for (uint32_t k = 1; k < L; ++k) plain[k] = slot_planes[(size_t)(k - 1) * 4];
        CoverageRecord *rec = nullptr;
        KC_TRY(coverage_enqueue(c, plain, &scaled, w, h, L, ref, coverage_scratch, &rec));
    }
    for (uint32_t k = 0; k < L; ++k) {
        kc_plane *const planes[4] = { col[3 * k], col[3 * k + 1], col[3 * k + 2], alpha_out[k] };
        levels[k] = image_new(4, planes);  // retains; mc drops its own
    }
    return KC_OK;
}

int image_build_mips(kc_image *img, uint32_t flags, kc_image **levels, uint32_t cap, uint32_t *count)
{
    if (flags & ~(uint32_t)(KC_MIP_PER_LEVEL | KC_MIP_NORMALS | KC_MIP_ALPHA_WEIGHT | kCoverageFlagBits)) {
        set_error("kc_image_build_mips: flags other than KC_MIP_PER_LEVEL, KC_MIP_NORMALS, KC_MIP_ALPHA_WEIGHT and KC_MIP_COVERAGE_REF");
        return KC_ERR_UNSUPPORTED;
    }
    KC_TRY(mip_check_alpha_flags(flags, "kc_image_build_mips"));
    KC_TRY(mip_check_coverage_flags(flags, "kc_image_build_mips"));
    if (!img || !levels || !count) return mip_refuse("kc_image_build_mips", "NULL image, level array or count");
    KC_TRY(need_init());
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    const uint32_t w = img->w(), h = img->h(), L = 1u + floor_log2(w > h ? w : h);
    *count = L;
    const bool normals = (flags & KC_MIP_NORMALS) != 0, per_level = (flags & KC_MIP_PER_LEVEL) != 0;
    const uint32_t ref = flags >> 24;  // != 0: KC_MIP_COVERAGE
    if (normals && !img->is_rgba()) return mip_refuse("kc_image_build_mips", "KC_MIP_NORMALS is for RGBA images (X, Y, Z in R, G, B)");
    if (ref && !img->is_rgba()) return mip_refuse("kc_image_build_mips", "KC_MIP_COVERAGE is for RGBA images");
    if ((flags & KC_MIP_ALPHA_WEIGHT) && !img->is_rgba()) return mip_refuse("kc_image_build_mips", "KC_MIP_ALPHA_WEIGHT is for RGBA images");
    if (cap < L) return mip_refuse("kc_image_build_mips", "cap is below the level count");
    if (!mip_size_ok(w, h)) return mip_refuse("kc_image_build_mips", "image too large");
    if (ref && (uint64_t)w * h > (1ull << 31)) return mip_refuse("kc_image_build_mips", "image too large");  // the targets' 64-bit products
    KC_TRY(image_force(img));  // pending chains and deferred resizes run first
    // KC_MIP_ALPHA_WEIGHT: a constant alpha >= 1 weighs every texel 1, which is the plain chain of the image bit for bit
    if ((flags & KC_MIP_ALPHA_WEIGHT) && !(img->planes[3]->kind == kc_plane::CONST && mip_alpha_weight(img->planes[3]->cval) == 1.0f))
        return image_build_alpha_mips(c, img, ref, per_level, levels, w, h, L);
    const int n = img->n;
    // sl: the planes the plain rule reduces (under KC_MIP_NORMALS: alpha alone); rgb: R, G, B under KC_MIP_NORMALS
    MipSlots sl, rgb;
    for (int ch = normals ? 3 : 0; ch < n; ++ch) sl.add(ch, img->planes[ch]);
    if (normals)
        for (int ch = 0; ch < 3; ++ch) rgb.add(ch, img->planes[ch]);
    // the planes of every level: one new resident plane per slot, shared by the channels that alias it, one constant per
    // constant channel; under KC_MIP_NORMALS three constants for R, G, B when all three are, three new resident planes otherwise
    MipChain mc;
    mc.planes.reserve((size_t)(L - 1) * n);
    std::vector<kc_plane *> slot_planes((size_t)(L - 1) * 4, nullptr);  // [level - 1][slot], owned through mc.planes
    std::vector<kc_plane *> rgb_planes(normals && rgb.n > 0 ? (size_t)(L - 1) * 3 : 0, nullptr);  // [level - 1][channel], likewise
    // KC_MIP_COVERAGE with a resident alpha: the level images get alpha planes of their own (d_k), the slot's planes keep the
    // plain alpha (p_k) that the next level is made from -- shared with R, G, B where they alias alpha, scratch otherwise
    const bool coverage = ref != 0 && sl.slot_of[3] >= 0 && L > 1;
    std::vector<kc_plane *> alpha_planes(coverage ? L - 1 : 0, nullptr);  // [level - 1], owned through mc.planes
    float cv[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    for (int ch = 0; ch < n; ++ch) cv[ch] = img->planes[ch]->cval;
    for (uint32_t k = 1; k < L; ++k) {
        const uint32_t W = level_extent(w, k), H = level_extent(h, k);
        if (normals && rgb.n == 0) {  // the fold: the box of each constant, then the texel's rule
            const float box[3] = { mip_const_fold(cv[0]), mip_const_fold(cv[1]), mip_const_fold(cv[2]) };
            mip_normal_texel(box, cv);
        }
        for (int ch = 0; ch < n; ++ch) {
            const int s = sl.slot_of[ch];
            kc_plane *p = nullptr;
            if (normals && ch < 3) {
                if (rgb.n == 0) {
                    p = plane_new_const(W, H, cv[ch]);
                } else {
                    KC_TRY(plane_new_mem(W, H, &p));
                    rgb_planes[(size_t)(k - 1) * 3 + ch] = p;
                }
            } else if (s < 0) {
                cv[ch] = mip_const_fold(cv[ch]);
                p = plane_new_const(W, H, cv[ch]);
            } else if (coverage && ch == 3) {
                kc_plane *&plain = slot_planes[(size_t)(k - 1) * 4 + s];
                if (!plain) {
                    KC_TRY(plane_new_mem(W, H, &plain));
                    mc.scratch.push_back(plain);
                }
                KC_TRY(plane_new_mem(W, H, &p));
                alpha_planes[k - 1] = p;
            } else if (slot_planes[(size_t)(k - 1) * 4 + s]) {
                p = slot_planes[(size_t)(k - 1) * 4 + s];
                plane_retain(p);
            } else {
                KC_TRY(plane_new_mem(W, H, &p));
                slot_planes[(size_t)(k - 1) * 4 + s] = p;
            }
            mc.planes.push_back(p);
        }
    }
    if (normals && rgb.n > 0) KC_TRY(mip_launch_normals(c, img->planes, rgb, rgb_planes, w, h, L, per_level));
    KC_TRY(mip_launch_plain(c, sl, slot_planes, w, h, L, per_level));
    PoolStaging coverage_scratch;  // back to the pool when the call returns: everything that reads it is enqueued by then
    if (coverage) {
        std::vector<const kc_plane *> plain(L, img->planes[3]);
        for (uint32_t k = 1; k < L; ++k) plain[k] = slot_planes[(size_t)(k - 1) * 4 + sl.slot_of[3]];
        CoverageRecord *rec = nullptr;
        KC_TRY(coverage_enqueue(c, plain, &alpha_planes, w, h, L, ref, coverage_scratch, &rec));
    }
    image_retain(img);
    levels[0] = img;
    for (uint32_t k = 1; k < L; ++k) levels[k] = image_new(n, mc.planes.data() + (size_t)(k - 1) * n);  // retains; mc drops its own
    return KC_OK;
}

// kc_image_build_roughness_mips: the named channel by the roughness rule (mip_launch_roughness), every other channel by the
// plain one, exactly as image_build_mips places them
int image_build_roughness_mips(kc_image *img, uint32_t channel, kc_image *normals, float power, uint32_t flags, kc_image **levels, uint32_t cap,
                               uint32_t *count)
{
    const char *who = "kc_image_build_roughness_mips";
    if (flags & ~(uint32_t)KC_MIP_PER_LEVEL) {
        set_error(std::string(who) + ": flags other than KC_MIP_PER_LEVEL");
        return KC_ERR_UNSUPPORTED;
    }
    if (!img || !normals || !levels || !count) return mip_refuse(who, "NULL image, normal map, level array or count");
    if (!(power > 0.0f && power <= 65536.0f)) return mip_refuse(who, "power must be a finite number above 0 and at most 65536");  // false for NaN
    KC_TRY(need_init());
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    const uint32_t w = img->w(), h = img->h(), L = 1u + floor_log2(w > h ? w : h);
    *count = L;
    if (!normals->is_rgba()) return mip_refuse(who, "the normal map must be an RGBA image (X, Y, Z in R, G, B)");
    if (normals->w() != w || normals->h() != h) return mip_refuse(who, "the normal map and the image differ in size");
    if (channel >= (uint32_t)img->n) return mip_refuse(who, "channel out of range for the image's kind");
    if (cap < L) return mip_refuse(who, "cap is below the level count");
    if (!mip_size_ok(w, h)) return mip_refuse(who, "image too large");
    KC_TRY(image_force(img));  // pending chains and deferred resizes of both run first
    KC_TRY(image_force(normals));
    const bool per_level = (flags & KC_MIP_PER_LEVEL) != 0;
    const kc_plane *src0[4] = { normals->planes[0], normals->planes[1], normals->planes[2], img->planes[channel] };
    // flat normals leave d = r everywhere: the plain chain of img, nothing new launched
    if (src0[0]->kind == kc_plane::CONST && src0[1]->kind == kc_plane::CONST && src0[2]->kind == kc_plane::CONST)
        return image_build_mips(img, flags, levels, cap, count);
    const int n = img->n;
    MipSlots sl;  // the planes the plain rule reduces: every channel but the named one
    for (int ch = 0; ch < n; ++ch)
        if ((uint32_t)ch != channel) sl.add(ch, img->planes[ch]);
    MipChain mc;
    mc.planes.reserve((size_t)(L - 1) * n);
    std::vector<kc_plane *> slot_planes((size_t)(L - 1) * 4, nullptr);  // [level - 1][slot], owned through mc.planes
    std::vector<kc_plane *> rough_planes(L - 1, nullptr);                // [level - 1], likewise: the named channel's own planes
    float cv[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    for (int ch = 0; ch < n; ++ch) cv[ch] = img->planes[ch]->cval;
    for (uint32_t k = 1; k < L; ++k) {
        const uint32_t W = level_extent(w, k), H = level_extent(h, k);
        for (int ch = 0; ch < n; ++ch) {
            const int s = sl.slot_of[ch];
            kc_plane *p = nullptr;
            if ((uint32_t)ch == channel) {
                KC_TRY(plane_new_mem(W, H, &p));
                rough_planes[k - 1] = p;
            } else if (s < 0) {
                cv[ch] = mip_const_fold(cv[ch]);
                p = plane_new_const(W, H, cv[ch]);
            } else if (slot_planes[(size_t)(k - 1) * 4 + s]) {
                p = slot_planes[(size_t)(k - 1) * 4 + s];
                plane_retain(p);
            } else {
                KC_TRY(plane_new_mem(W, H, &p));
                slot_planes[(size_t)(k - 1) * 4 + s] = p;
            }
            mc.planes.push_back(p);
        }
    }
    KC_TRY(mip_launch_roughness(c, src0, rough_planes, mc, power, w, h, L, per_level));
    KC_TRY(mip_launch_plain(c, sl, slot_planes, w, h, L, per_level));
    image_retain(img);
    levels[0] = img;
    for (uint32_t k = 1; k < L; ++k) levels[k] = image_new(n, mc.planes.data() + (size_t)(k - 1) * n);  // retains; mc drops its own
    return KC_OK;
}

// kc_image_mip_coverage_info: alpha's plain chain in scratch planes, the select, the records back
int image_mip_coverage_info(kc_image *img, uint32_t flags, kc_mip_coverage_level *out, uint32_t cap, uint32_t *count)
{
    const char *who = "kc_image_mip_coverage_info";
    if ((flags & ~(uint32_t)(KC_MIP_PER_LEVEL | KC_MIP_NORMALS | kCoverageFlagBits)) || !(flags & KC_MIP_COVERAGE)) {
        set_error(std::string(who) + ": flags must hold KC_MIP_COVERAGE_REF, with KC_MIP_PER_LEVEL and KC_MIP_NORMALS at the most");
        return KC_ERR_UNSUPPORTED;
    }
    KC_TRY(mip_check_coverage_flags(flags, who));
    if (!img || !out || !count) return mip_refuse(who, "NULL image, record array or count");
    KC_TRY(need_init());
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    const uint32_t w = img->w(), h = img->h(), L = 1u + floor_log2(w > h ? w : h), ref = flags >> 24;
    *count = L;
    if (!img->is_rgba()) return mip_refuse(who, "KC_MIP_COVERAGE is for RGBA images");
    if (cap < L) return mip_refuse(who, "cap is below the level count");
    if (w > (1u << 30) || ((uint64_t)h + 63) / 64 > 65535ull || (uint64_t)w * h > (1ull << 31)) return mip_refuse(who, "image too large");
    KC_TRY(image_force(img));
    const uint64_t n_0 = (uint64_t)w * h;
    const kc_plane *alpha = img->planes[3];
    if (alpha->kind == kc_plane::CONST) {  // answered here: every texel of a level is covered or none is
        float cv = alpha->cval;
        const uint64_t c_0 = quant_u8_host(cv) >= ref ? n_0 : 0;
        for (uint32_t k = 0; k < L; ++k) {
            const uint64_t n_k = (uint64_t)level_extent(w, k) * level_extent(h, k);
            if (k) cv = mip_const_fold(cv);
            out[k] = kc_mip_coverage_level{ n_k, k ? coverage_target(n_0, n_k, c_0) : c_0, quant_u8_host(cv) >= ref ? n_k : 0, 0.0f, 1.0f };
        }
        return KC_OK;
    }
    MipSlots sl;
    sl.add(3, alpha);
    MipChain mc;
    std::vector<kc_plane *> slot_planes((size_t)(L - 1) * 4, nullptr);
    std::vector<const kc_plane *> plain(L, alpha);
    for (uint32_t k = 1; k < L; ++k) {
        kc_plane *p = nullptr;
        KC_TRY(plane_new_mem(level_extent(w, k), level_extent(h, k), &p));
        mc.scratch.push_back(p);
        slot_planes[(size_t)(k - 1) * 4] = p;
        plain[k] = p;
    }
    KC_TRY(mip_launch_plain(c, sl, slot_planes, w, h, L, (flags & KC_MIP_PER_LEVEL) != 0));
    PoolStaging scratch;
    CoverageRecord *rec = nullptr;
    KC_TRY(coverage_enqueue(c, plain, nullptr, w, h, L, ref, scratch, &rec));
    std::vector<CoverageRecord> got(L);
    hipError_t e = hipMemcpyAsync(got.data(), rec, (size_t)L * sizeof(CoverageRecord), hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) return hip_fail(e, who);
    for (uint32_t k = 0; k < L; ++k) out[k] = kc_mip_coverage_level{ got[k].texels, got[k].target, got[k].plain_covered, got[k].v, got[k].scale };
    return KC_OK;
}

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
