// Mip chains (include/kanter_core_amd.h): kc_mip_level_count, kc_preview_level, kc_image_build_mips,
// kc_image_build_roughness_mips, kc_image_mip_coverage_info.  The host side does the level arithmetic,
// folds constant planes with the device's expression, allocates the level planes and enqueues mip.hip's kernels on the library's
// stream: the pyramid kernel while both extents still halve (up to six levels per launch), the one-level kernel for the rest and
// for every level under KC_MIP_PER_LEVEL; under KC_MIP_NORMALS mip_normals.hip's two kernels take R, G, B together and
// renormalise every level; under KC_MIP_COVERAGE mip_coverage.hip's select and scale give alpha planes of their own; under
// KC_MIP_ALPHA_WEIGHT mip_alpha.hip's pull and push give colour planes of their own, level 0 included; a roughness
// chain is mip_roughness.hip's two kernels on the vector of a normal map and the roughness plane together.  The file holds the
// rules' host arithmetic, then the chains: mip_plan decides the launches of a chain, mip_enqueue enqueues them for every
// family, mip_place places the planes of the levels.  The export of a chain is mip_export.cpp.
#include <array>
#include <cmath>
#include <limits>

#include "kc_runtime.hpp"

namespace kc {

int mip_refuse(const char *who, const char *what)
{
    set_error(std::string(who) + ": " + what);
    return KC_ERR_INVALID_ARG;
}

int mip_level_count(uint32_t w, uint32_t h, uint32_t *levels)
{
    if (!levels || w == 0 || h == 0) return mip_refuse("kc_mip_level_count", "NULL output or zero extent");
    *levels = 1u + floor_log2(w > h ? w : h);
    return KC_OK;
}

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
int mip_check_alpha_flags(uint32_t flags, const char *who)
{
    if ((flags & KC_MIP_ALPHA_WEIGHT) && (flags & KC_MIP_NORMALS)) {
        set_error(std::string(who) + ": KC_MIP_NORMALS with KC_MIP_ALPHA_WEIGHT");
        return KC_ERR_UNSUPPORTED;
    }
    return KC_OK;
}

// ---------------------------------------------------------------- KC_MIP_COVERAGE: the rule's arithmetic
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

// ---------------------------------------------------------------- the chains: the plan of the launches
std::vector<MipStep> mip_plan(uint32_t w, uint32_t h, uint32_t L, bool per_level, uint32_t in0, uint32_t in_below, uint32_t out_planes,
                              const Options &o)
{
    std::vector<MipStep> plan;
    plan.reserve(L);
    for (uint32_t k = 0; k + 1 < L; k = plan.back().last()) {  // k: the level the next launch reads
        const uint32_t sw = level_extent(w, k), sh = level_extent(h, k);
        const uint32_t small = sw < sh ? sw : sh;
        const uint32_t fused = per_level || small < 2 ? 0u : floor_log2(small) < 6u ? floor_log2(small) : 6u;
        const uint32_t n_src = k == 0 ? in0 : in_below;
        const uint64_t in_bytes = (uint64_t)sw * sh * 4 * n_src;
        const uint64_t out_bytes = (uint64_t)level_extent(w, k + 1) * level_extent(h, k + 1) * 4 * out_planes;
        plan.push_back(MipStep{ k, sw, sh, fused, (cache_policy_mask(in_bytes, out_bytes, n_src, o) & 0xffu) != 0 });
    }
    return plan;
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

uint32_t pitch_of(const kc_plane *p) { return (uint32_t)(p->pitch / sizeof(float)); }

// the texels of the levels >= 1
uint64_t texels_below(uint32_t w, uint32_t h, uint32_t L)
{
    uint64_t texels = 0;
    for (uint32_t k = 1; k < L; ++k) texels += (uint64_t)level_extent(w, k) * level_extent(h, k);
    return texels;
}

// Level 0 of a family that couples n channels (3 or 4) in one thread: plane[ch], constant or resident; sl: its distinct
// resident planes; bit ch of const_mask: a constant; bits 2 ch, 2 ch + 1 of `from` (KC_MIP_NORMALS): the earliest channel that
// reads the same plane, ch itself otherwise.  Below level 0 every channel has a resident plane of its own.
struct MipSource {
    const kc_plane *const *plane;
    int n;
    MipSlots sl;
    uint32_t const_mask = 0, from = 0;
    MipSource(const kc_plane *const *planes, int channels) : plane(planes), n(channels)
    {
        for (int ch = 0; ch < n; ++ch) {
            sl.add(ch, plane[ch]);
            int f = ch;
            if (sl.slot_of[ch] < 0) const_mask |= 1u << ch;
            else
                for (int e = ch - 1; e >= 0; --e)
                    if (sl.slot_of[e] == sl.slot_of[ch]) f = e;
            from |= (uint32_t)f << (2 * ch);
        }
    }
    // the source side of the launch s in any of the coupled argument blocks: level 0, or the planes `below` of level s.k
    template <class Args> void fill(Args &a, const MipStep &s, const kc_plane *const *below) const
    {
        a.w = s.sw;
        a.h = s.sh;
        for (int ch = 0; ch < n; ++ch) {
            const kc_plane *p = s.k == 0 ? plane[ch] : below[ch];
            const bool is_const = s.k == 0 && ((const_mask >> ch) & 1u);
            a.src[ch] = is_const ? nullptr : p->dptr;
            a.src_pitch[ch] = is_const ? 0u : pitch_of(p);
            a.cval[ch] = is_const ? p->cval : 0.0f;
        }
        a.const_mask = s.k == 0 ? const_mask : 0u;
    }
};

// ---------------------------------------------------------------- the chains: one enqueue loop, and the families
// The state planes of a launch: the boxes of the last level it writes, which the next launch reads instead of stored planes
// (four under the roughness rule, three under KC_MIP_ALPHA_WEIGHT); all NULL where a family has none or no level follows.
using MipState = std::array<kc_plane *, 4>;

// The n state planes of a W x H level, from the pool, held in mc.scratch until the call returns (everything that reads them is
// enqueued by then); pitch: of the level's stored planes, which the kernels take for the state planes' too
int mip_state_planes(MipChain &mc, int n, uint32_t W, uint32_t H, size_t pitch, const char *who, MipState &out)
{
    for (int ch = 0; ch < n; ++ch) {
        KC_TRY(plane_new_mem(W, H, &out[ch]));
        mc.scratch.push_back(out[ch]);
        if (out[ch]->pitch != pitch) return mip_refuse(who, "planes of one size differ in pitch");
    }
    return KC_OK;
}

// a field of an argument block that a pyramid kernel has once per fused level and a one-level kernel once
template <class T, size_t N> T &at_level(T (&field)[N], uint32_t j) { return field[j]; }
template <class T> T &at_level(T &field, uint32_t) { return field; }

// Enqueues the launches of `plan` (a chain of L levels of a w x h image) for the family f on the library's stream and counts
// them.  A family names its two argument blocks, their launchers and counters and the state planes it passes from launch to
// launch (kState, with level_pitch and kWho for mip_state_planes); its fill(a, s, in, out) writes either block for the step s,
// where `in` are the state planes of level s.k and `out` those of level s.last().  *state_texels grows by the texels of every
// level that got state planes.
template <class Family>
int mip_enqueue(Context &c, const Family &f, MipChain &mc, const std::vector<MipStep> &plan, uint32_t w, uint32_t h, uint32_t L,
                uint64_t *state_texels = nullptr)
{
    MipState in{}, out{};
    for (const MipStep &s : plan) {
        out = MipState{};
        if constexpr (Family::kState > 0)
            if (s.last() + 1 < L) {  // more levels follow
                const uint32_t W = level_extent(w, s.last()), H = level_extent(h, s.last());
                KC_TRY(mip_state_planes(mc, Family::kState, W, H, f.level_pitch(s.last()), Family::kWho, out));
                *state_texels += (uint64_t)W * H;
            }
        hipError_t e;
        if (s.fused) {
            typename Family::Pyramid a{};
            a.n = s.fused;
            f.fill(a, s, in, out);
            e = f.launch(a, s, c.stream);
        } else {
            typename Family::Level a{};
            f.fill(a, s, in, out);
            e = f.launch(a, s, c.stream);
        }
        if (e != hipSuccess) return hip_fail(e, s.fused ? Family::kPyramid : Family::kLevel);
        c.counters[s.fused ? Family::kPyramidCounter : Family::kLevelCounter]++;
        if (s.nt) c.counters["mip_nt"]++;
        c.launches++;
        in = out;
    }
    return KC_OK;
}

// The plain rule on the resident planes of sl: level k of slot s is slot_planes[(k - 1) * 4 + s]
struct PlainFamily {
    using Pyramid = MipPyramidArgs;
    using Level = MipLevelArgs;
    static constexpr int kState = 0;
    static constexpr const char *kPyramid = "launch_mip_pyramid", *kLevel = "launch_mip_level", *kPyramidCounter = "mip_pyramid",
                                *kLevelCounter = "mip_level";
    const MipSlots &sl;
    const std::vector<kc_plane *> &slot_planes;
    const kc_plane *at(uint32_t k, int s) const { return k == 0 ? sl.src[s] : slot_planes[(size_t)(k - 1) * 4 + s]; }
    template <class Args> void fill(Args &a, const MipStep &s, const MipState &, const MipState &) const
    {
        a.w = s.sw;
        a.h = s.sh;
        for (int p = 0; p < sl.n; ++p) {
            a.src[p] = at(s.k, p)->dptr;
            a.src_pitch[p] = pitch_of(at(s.k, p));
        }
        for (uint32_t j = 0, k = s.k + 1; k <= s.last(); ++j, ++k) {
            for (int p = 0; p < sl.n; ++p) at_level(a.dst[p], j) = at(k, p)->dptr;
            at_level(a.dst_pitch, j) = pitch_of(at(k, 0));
        }
    }
    hipError_t launch(const Pyramid &a, const MipStep &s, hipStream_t stream) const { return launch_mip_pyramid(a, (uint32_t)sl.n, s.nt, stream); }
    hipError_t launch(const Level &a, const MipStep &s, hipStream_t stream) const { return launch_mip_level(a, (uint32_t)sl.n, s.nt, stream); }
};

// KC_MIP_NORMALS: R, G, B coupled (src: level 0, at least one of the three resident); level k of channel c is
// own[(k - 1) * 4 + c], resident at every level
struct NormalFamily {
    using Pyramid = NormalPyramidArgs;
    using Level = NormalLevelArgs;
    static constexpr int kState = 0;
    static constexpr const char *kPyramid = "launch_normal_pyramid", *kLevel = "launch_normal_level",
                                *kPyramidCounter = "mip_normals_pyramid", *kLevelCounter = "mip_normals_level";
    const MipSource &src;
    const std::vector<kc_plane *> &own;
    kc_plane *const *at(uint32_t k) const { return &own[(size_t)(k - 1) * 4]; }  // k >= 1
    template <class Args> void fill(Args &a, const MipStep &s, const MipState &, const MipState &) const
    {
        src.fill(a, s, s.k ? at(s.k) : nullptr);
        a.from = s.k == 0 ? src.from : (0u | 1u << 2 | 2u << 4);
        for (uint32_t j = 0, k = s.k + 1; k <= s.last(); ++j, ++k) {
            for (int ch = 0; ch < 3; ++ch) at_level(a.dst[ch], j) = at(k)[ch]->dptr;
            at_level(a.dst_pitch, j) = pitch_of(at(k)[0]);
        }
    }
    hipError_t launch(const Pyramid &a, const MipStep &s, hipStream_t stream) const { return launch_normal_pyramid(a, s.nt, stream); }
    hipError_t launch(const Level &a, const MipStep &s, hipStream_t stream) const { return launch_normal_level(a, s.nt, stream); }
};

// kc_image_build_roughness_mips: the vector of the normals and the roughness coupled (src: X, Y, Z of the normal map and the
// roughness plane at level 0, at least one of the first three resident); level k's stored plane is own[(k - 1) * 4 + channel].
// The four plain boxes of the last level a launch writes are the next launch's sources: its state planes.
struct RoughnessFamily {
    using Pyramid = RoughnessPyramidArgs;
    using Level = RoughnessLevelArgs;
    static constexpr int kState = 4;
    static constexpr const char *kPyramid = "launch_roughness_pyramid", *kLevel = "launch_roughness_level",
                                *kPyramidCounter = "mip_roughness_pyramid", *kLevelCounter = "mip_roughness_level",
                                *kWho = "kc_image_build_roughness_mips";
    const MipSource &src;
    const std::vector<kc_plane *> &own;
    uint32_t channel;
    float power;
    const kc_plane *at(uint32_t k) const { return own[(size_t)(k - 1) * 4 + channel]; }  // k >= 1
    size_t level_pitch(uint32_t k) const { return at(k)->pitch; }
    template <class Args> void fill(Args &a, const MipStep &s, const MipState &in, const MipState &out) const
    {
        src.fill(a, s, in.data());
        a.power = power;
        for (int ch = 0; ch < 4; ++ch) a.state[ch] = out[ch] ? out[ch]->dptr : nullptr;
        for (uint32_t j = 0, k = s.k + 1; k <= s.last(); ++j, ++k) {
            at_level(a.dst, j) = at(k)->dptr;
            at_level(a.dst_pitch, j) = pitch_of(at(k));
        }
    }
    hipError_t launch(const Pyramid &a, const MipStep &s, hipStream_t stream) const { return launch_roughness_pyramid(a, s.k == 0, s.nt, stream); }
    hipError_t launch(const Level &a, const MipStep &s, hipStream_t stream) const { return launch_roughness_level(a, s.k == 0, s.nt, stream); }
};

// KC_MIP_ALPHA_WEIGHT, the pull: the premultiplied colour and the weight coupled (src: R, G, B, alpha at level 0, the colours
// or alpha resident); level k's colour planes are col[3 k + c], level 0 included, and weight[k] the weight plane of a level
// k >= 1.  P_c of the last level a launch writes are the next launch's sources beside that level's weight: its state planes.
struct AlphaPullFamily {
    using Pyramid = AlphaPullPyramidArgs;
    using Level = AlphaPullLevelArgs;
    static constexpr int kState = 3;
    static constexpr const char *kPyramid = "launch_alpha_pull_pyramid", *kLevel = "launch_alpha_pull_level",
                                *kPyramidCounter = "mip_alpha_pull_pyramid", *kLevelCounter = "mip_alpha_pull_level",
                                *kWho = "kc_image_build_mips";
    const MipSource &src;
    const std::vector<kc_plane *> &col, &weight;
    uint32_t L;
    size_t level_pitch(uint32_t k) const { return weight[k]->pitch; }
    template <class Args> void fill(Args &a, const MipStep &s, const MipState &in, const MipState &out) const
    {
        const kc_plane *const below[4] = { in[0], in[1], in[2], weight[s.k] };
        src.fill(a, s, below);
        for (int ch = 0; ch < 3; ++ch) {
            a.dst0[ch] = s.k == 0 ? col[ch]->dptr : nullptr;
            a.state[ch] = out[ch] ? out[ch]->dptr : nullptr;
        }
        a.dst0_pitch = s.k == 0 ? pitch_of(col[0]) : 0u;
        for (uint32_t j = 0, k = s.k + 1; k <= s.last() && k < L; ++j, ++k) {  // k == L on a 1 x 1 image: level 0's colour alone
            for (int ch = 0; ch < 3; ++ch) at_level(a.dst[ch], j) = col[3 * k + ch]->dptr;
            at_level(a.wdst, j) = weight[k]->dptr;
            at_level(a.dst_pitch, j) = pitch_of(weight[k]);
        }
    }
    hipError_t launch(const Pyramid &a, const MipStep &s, hipStream_t stream) const { return launch_alpha_pull_pyramid(a, s.k == 0, s.nt, stream); }
    hipError_t launch(const Level &a, const MipStep &s, hipStream_t stream) const { return launch_alpha_pull_level(a, s.k == 0, s.nt, stream); }
};
}  // namespace

// The plain rule's launches for the resident planes of sl
static int mip_launch_plain(Context &c, const MipSlots &sl, const std::vector<kc_plane *> &slot_planes, MipChain &mc, uint32_t w, uint32_t h,
                            uint32_t L, bool per_level)
{
    if (sl.n == 0 || L < 2) return KC_OK;
    KC_TRY(mip_enqueue(c, PlainFamily{ sl, slot_planes }, mc, mip_plan(w, h, L, per_level, (uint32_t)sl.n, (uint32_t)sl.n, (uint32_t)sl.n), w, h, L));
    c.alg_bytes += 4 * ((uint64_t)w * h + texels_below(w, h, L)) * sl.n;  // level 0 read once, every further level written once
    return KC_OK;
}

// KC_MIP_NORMALS: the coupled launches for R, G, B
static int mip_launch_normals(Context &c, const MipSource &rgb, const std::vector<kc_plane *> &own, MipChain &mc, uint32_t w, uint32_t h, uint32_t L,
                              bool per_level)
{
    if (L < 2) return KC_OK;
    KC_TRY(mip_enqueue(c, NormalFamily{ rgb, own }, mc, mip_plan(w, h, L, per_level, (uint32_t)rgb.sl.n, 3u, 3u), w, h, L));
    // every distinct resident plane of level 0 read once, three planes of every further level written once
    c.alg_bytes += 4 * (uint64_t)w * h * rgb.sl.n + 12 * texels_below(w, h, L);
    return KC_OK;
}

// kc_image_build_roughness_mips: the coupled launches for the vector of the normals and the roughness
static int mip_launch_roughness(Context &c, const MipSource &src, const std::vector<kc_plane *> &own, uint32_t channel, MipChain &mc, float power,
                                uint32_t w, uint32_t h, uint32_t L, bool per_level)
{
    if (L < 2) return KC_OK;
    uint64_t state_texels = 0;
    KC_TRY(mip_enqueue(c, RoughnessFamily{ src, own, channel, power }, mc, mip_plan(w, h, L, per_level, (uint32_t)src.sl.n, 4u, 1u), w, h, L,
                       &state_texels));
    // every distinct resident plane of level 0 read once, one plane of every further level written once, the four state planes
    // of a level written once and read once
    c.alg_bytes += 4 * (uint64_t)w * h * src.sl.n + 4 * texels_below(w, h, L) + 32 * state_texels;
    return KC_OK;
}

// KC_MIP_ALPHA_WEIGHT: the pull launches and the push launch over all levels.  The weight of every level >= 1 lives in a
// scratch plane from the pool, held in mc.scratch like the state planes.
static int mip_launch_alpha(Context &c, const MipSource &src, const std::vector<kc_plane *> &col, MipChain &mc, uint32_t w, uint32_t h, uint32_t L,
                            bool per_level)
{
    if (L > KC_ALPHA_MAX_LEVELS) return mip_refuse("KC_MIP_ALPHA_WEIGHT", "more levels than the job table holds");
    std::vector<kc_plane *> weight(L, nullptr);  // [level], levels >= 1
    for (uint32_t k = 0; k < L; ++k) {
        if (k) {
            KC_TRY(plane_new_mem(level_extent(w, k), level_extent(h, k), &weight[k]));
            mc.scratch.push_back(weight[k]);
        }
        for (int ch = 0; ch < 3; ++ch)
            if (col[3 * k + ch]->pitch != (k ? weight[k] : col[0])->pitch) return mip_refuse(AlphaPullFamily::kWho, "planes of one size differ in pitch");
    }
    uint64_t state_texels = 0;
    // a 1 x 1 image has no level to pull: one one-level launch for level 0's colour, which no level follows
    const std::vector<MipStep> plan = L == 1 ? std::vector<MipStep>{ MipStep{ 0, w, h, 0, false } }
                                             : mip_plan(w, h, L, per_level, (uint32_t)src.sl.n, 4u, 4u);
    KC_TRY(mip_enqueue(c, AlphaPullFamily{ src, col, weight, L }, mc, plan, w, h, L, &state_texels));
    AlphaPushArgs pa{};
    uint32_t wgs = 0;
    const bool a_const = (src.const_mask & 8u) != 0;
    for (uint32_t k = 0; k < L; ++k) {
        AlphaPushJob &J = pa.jobs[k];
        for (int ch = 0; ch < 3; ++ch) J.dst[ch] = col[3 * k + ch]->dptr;
        J.dst_pitch = pitch_of(col[3 * k]);
        const kc_plane *ws = k ? weight[k] : a_const ? nullptr : src.plane[3];
        J.wsrc = ws ? ws->dptr : nullptr;
        J.w_pitch = ws ? pitch_of(ws) : 0u;
        J.w = level_extent(w, k);
        J.h = level_extent(h, k);
        J.first_wg = wgs;
        J.wgs = alpha_push_job_wgs(J.w, J.h);
        wgs += J.wgs;
    }
    pa.levels = L;
    hipError_t e = launch_alpha_push(pa, wgs, c.stream);
    if (e != hipSuccess) return hip_fail(e, "launch_alpha_push");
    c.counters["mip_alpha_push"]++;
    c.launches++;
    // the pull: every distinct resident plane of level 0 read once, level 0's three colour planes written, three colours and the
    // weight of every further level written, the three state planes of a level written and read and its weight read; the push:
    // level 0's alpha where it is resident and every weight read (what it writes depends on the data and is not counted)
    const uint64_t n0 = (uint64_t)w * h, below = texels_below(w, h, L);
    c.alg_bytes += 4 * n0 * src.sl.n + 12 * n0 + 16 * below + 28 * state_texels + (a_const ? 0 : 4 * n0) + 4 * below;
    return KC_OK;
}

// KC_MIP_COVERAGE: the select over alpha's plain chain (p_0 = alpha0, the image's alpha; p_k = slot_planes[(k - 1) * 4 + slot];
// L levels of a w x h image, w h <= 2^31) and, with `own` (d_k = (*own)[(k - 1) * 4 + 3]), the scale launch.  The records and
// the histograms live in `scratch`, which the caller gives back to the pool once everything that reads it is enqueued (or
// waited for); *rec = the L device records.  Launches: a count and a pick per pass, three passes when there is a level >= 1,
// and the scale.
static int coverage_enqueue(Context &c, const kc_plane *alpha0, const std::vector<kc_plane *> &slot_planes, int slot, const std::vector<kc_plane *> *own,
                            uint32_t w, uint32_t h, uint32_t L, uint32_t ref, PoolStaging &scratch, CoverageRecord **rec)
{
    if (L > KC_COVERAGE_MAX_LEVELS) return mip_refuse("KC_MIP_COVERAGE", "more levels than the job table holds");
    const size_t rec_bytes = ((size_t)L * sizeof(CoverageRecord) + 255) / 256 * 256, hist_bytes = (size_t)L * KC_COVERAGE_BINS * sizeof(uint32_t);
    KC_TRY(scratch.alloc(rec_bytes + hist_bytes));
    CoverageArgs a{};
    uint32_t wgs = 0;
    for (uint32_t k = 0; k < L; ++k) {
        CoverageJob &J = a.jobs[k];
        const kc_plane *plain = k ? slot_planes[(size_t)(k - 1) * 4 + slot] : alpha0, *scaled = own && k ? (*own)[(size_t)(k - 1) * 4 + 3] : nullptr;
        J.src = plain->dptr;
        J.src_pitch = pitch_of(plain);
        J.dst = scaled ? scaled->dptr : nullptr;
        J.dst_pitch = scaled ? pitch_of(scaled) : 0u;
        J.w = level_extent(w, k);
        J.h = level_extent(h, k);
        J.first_wg = wgs;
        J.wgs = coverage_job_wgs(J.w, J.h);
        wgs += J.wgs;
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
    const uint64_t below = texels_below(w, h, L);
    uint64_t texels = (uint64_t)w * h + 3 * below;  // level 0 once, every further level once per pass
    if (own && L > 1) {
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

// ---------------------------------------------------------------- the chains: the planes of the levels
// The planes of levels 1 .. L - 1 of the channels first .. n - 1 of an image (`planes`: level 0), pushed to mc.planes as
// [level - 1][channel - first].  A channel follows the plain rule: a constant is folded, channels that alias one resident
// plane (sl: the distinct ones) share one new resident plane per level, slot_planes[(k - 1) * 4 + slot], which
// mip_launch_plain writes.  A channel in own_mask follows a rule of its own: own(k, ch, W, H, p) gives its plane of level k,
// recorded as own_planes[(k - 1) * 4 + ch] for the launches of that rule.
template <class Own>
static int mip_place(MipChain &mc, const MipSlots &sl, std::vector<kc_plane *> &slot_planes, std::vector<kc_plane *> &own_planes,
                     kc_plane *const *planes, int first, int n, uint32_t own_mask, uint32_t w, uint32_t h, uint32_t L, Own own)
{
    float cv[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    for (int ch = first; ch < n; ++ch) cv[ch] = planes[ch]->cval;
    for (uint32_t k = 1; k < L; ++k) {
        const uint32_t W = level_extent(w, k), H = level_extent(h, k);
        for (int ch = first; ch < n; ++ch) {
            const int s = sl.slot_of[ch];
            kc_plane *p = nullptr;
            if ((own_mask >> ch) & 1u) {
                KC_TRY(own(k, ch, W, H, p));
                own_planes[(size_t)(k - 1) * 4 + ch] = p;
            } else if (s < 0) {
                cv[ch] = mip_const_fold(cv[ch]);
                p = plane_new_const(W, H, cv[ch]);
            } else if (kc_plane *&shared = slot_planes[(size_t)(k - 1) * 4 + s]; shared) {
                p = shared;
                plane_retain(p);
            } else {
                KC_TRY(plane_new_mem(W, H, &p));
                shared = p;
            }
            mc.planes.push_back(p);
        }
    }
    return KC_OK;
}

// the rule of its own of a channel that gets a new resident plane at every level, whatever it is at level 0
static int mip_own_plane(uint32_t, int, uint32_t W, uint32_t H, kc_plane *&p) { return plane_new_mem(W, H, &p); }

// KC_MIP_COVERAGE with a resident alpha, one level: the level image gets an alpha plane of its own (d_k, *scaled); the slot's
// plane keeps the plain alpha (p_k) that the next level is made from -- shared with R, G, B where they alias alpha and have
// placed it, scratch otherwise
static int mip_place_coverage(MipChain &mc, kc_plane *&plain, uint32_t W, uint32_t H, kc_plane *&scaled)
{
    if (!plain) {
        KC_TRY(plane_new_mem(W, H, &plain));
        mc.scratch.push_back(plain);
    }
    return plane_new_mem(W, H, &scaled);
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
    MipChain mc;  // planes: one reference per plane of the level images: alpha of the levels >= 1 first, then the colours
    mc.planes.reserve((size_t)L * 4);
    MipSlots sl;
    sl.add(3, A);
    const bool coverage = ref != 0 && !a_const && L > 1;
    std::vector<kc_plane *> slot_planes((size_t)(L - 1) * 4, nullptr), own_planes(coverage ? (size_t)(L - 1) * 4 : 0, nullptr);
    KC_TRY(mip_place(mc, sl, slot_planes, own_planes, img->planes, 3, 4, coverage ? 8u : 0u, w, h, L,
                     [&](uint32_t k, int, uint32_t W, uint32_t H, kc_plane *&p) { return mip_place_coverage(mc, slot_planes[(size_t)(k - 1) * 4], W, H, p); }));
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
    if (!zero && !fold) KC_TRY(mip_launch_alpha(c, MipSource(img->planes, 4), col, mc, w, h, L, per_level));
    KC_TRY(mip_launch_plain(c, sl, slot_planes, mc, w, h, L, per_level));
    PoolStaging coverage_scratch;  // back to the pool when the call returns: everything that reads it is enqueued by then
    CoverageRecord *rec = nullptr;
    if (coverage) KC_TRY(coverage_enqueue(c, A, slot_planes, 0, &own_planes, w, h, L, ref, coverage_scratch, &rec));
    for (uint32_t k = 0; k < L; ++k) {
        kc_plane *const planes[4] = { col[3 * k], col[3 * k + 1], col[3 * k + 2], k ? mc.planes[k - 1] : img->planes[3] };
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
    MipSlots sl;
    for (int ch = normals ? 3 : 0; ch < n; ++ch) sl.add(ch, img->planes[ch]);
    const MipSource rgb(img->planes, normals ? 3 : 0);
    // KC_MIP_NORMALS on constant R, G, B, [level - 1][channel]: the box of each constant, then the texel's rule
    std::vector<float> flat;
    if (normals && rgb.sl.n == 0) {
        float cv[3] = { img->planes[0]->cval, img->planes[1]->cval, img->planes[2]->cval };
        for (uint32_t k = 1; k < L; ++k) {
            const float box[3] = { mip_const_fold(cv[0]), mip_const_fold(cv[1]), mip_const_fold(cv[2]) };
            mip_normal_texel(box, cv);
            flat.insert(flat.end(), cv, cv + 3);
        }
    }
    // KC_MIP_COVERAGE with a resident alpha: the level images get alpha planes of their own (mip_place_coverage)
    const bool coverage = ref != 0 && sl.slot_of[3] >= 0 && L > 1;
    MipChain mc;
    mc.planes.reserve((size_t)(L - 1) * n);
    // rules of their own: alpha under coverage; under KC_MIP_NORMALS R, G, B -- three constants when all three are, three new
    // resident planes otherwise
    const uint32_t own_mask = (normals ? 7u : 0u) | (coverage ? 8u : 0u);
    std::vector<kc_plane *> slot_planes((size_t)(L - 1) * 4, nullptr), own_planes(own_mask ? (size_t)(L - 1) * 4 : 0, nullptr);  // owned through mc
    KC_TRY(mip_place(mc, sl, slot_planes, own_planes, img->planes, 0, n, own_mask, w, h, L,
                     [&](uint32_t k, int ch, uint32_t W, uint32_t H, kc_plane *&p) {
                         if (ch == 3) return mip_place_coverage(mc, slot_planes[(size_t)(k - 1) * 4 + sl.slot_of[3]], W, H, p);
                         if (rgb.sl.n > 0) return plane_new_mem(W, H, &p);
                         p = plane_new_const(W, H, flat[(size_t)(k - 1) * 3 + ch]);
                         return (int)KC_OK;
                     }));
    if (normals && rgb.sl.n > 0) KC_TRY(mip_launch_normals(c, rgb, own_planes, mc, w, h, L, per_level));
    KC_TRY(mip_launch_plain(c, sl, slot_planes, mc, w, h, L, per_level));
    PoolStaging coverage_scratch;  // back to the pool when the call returns: everything that reads it is enqueued by then
    CoverageRecord *rec = nullptr;
    if (coverage) KC_TRY(coverage_enqueue(c, img->planes[3], slot_planes, sl.slot_of[3], &own_planes, w, h, L, ref, coverage_scratch, &rec));
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
    std::vector<kc_plane *> slot_planes((size_t)(L - 1) * 4, nullptr), own_planes((size_t)(L - 1) * 4, nullptr);  // owned through mc
    KC_TRY(mip_place(mc, sl, slot_planes, own_planes, img->planes, 0, n, 1u << channel, w, h, L, mip_own_plane));
    KC_TRY(mip_launch_roughness(c, MipSource(src0, 4), own_planes, channel, mc, power, w, h, L, per_level));
    KC_TRY(mip_launch_plain(c, sl, slot_planes, mc, w, h, L, per_level));
    image_retain(img);
    levels[0] = img;
    for (uint32_t k = 1; k < L; ++k) levels[k] = image_new(n, mc.planes.data() + (size_t)(k - 1) * n);  // retains; mc drops its own
    return KC_OK;
}

// kc_image_mip_coverage_info: alpha's plain chain in planes that live until the call returns, the select, the records back
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
    if (!mip_size_ok(w, h) || (uint64_t)w * h > (1ull << 31)) return mip_refuse(who, "image too large");  // the targets' 64-bit products
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
    MipChain mc;  // alpha alone, by the plain rule: the planes of its levels go back to the pool when the call returns
    std::vector<kc_plane *> slot_planes((size_t)(L - 1) * 4, nullptr), own_planes;
    KC_TRY(mip_place(mc, sl, slot_planes, own_planes, img->planes, 3, 4, 0u, w, h, L, mip_own_plane));  // own_mask 0: the hook is not called
    KC_TRY(mip_launch_plain(c, sl, slot_planes, mc, w, h, L, (flags & KC_MIP_PER_LEVEL) != 0));
    PoolStaging scratch;
    CoverageRecord *rec = nullptr;
    KC_TRY(coverage_enqueue(c, alpha, slot_planes, 0, nullptr, w, h, L, ref, scratch, &rec));
    std::vector<CoverageRecord> got(L);
    hipError_t e = hipMemcpyAsync(got.data(), rec, (size_t)L * sizeof(CoverageRecord), hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) return hip_fail(e, who);
    for (uint32_t k = 0; k < L; ++k) out[k] = kc_mip_coverage_level{ got[k].texels, got[k].target, got[k].plain_covered, got[k].v, got[k].scale };
    return KC_OK;
}

}  // namespace kc

