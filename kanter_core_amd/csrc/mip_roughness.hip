// Roughness mip chains that absorb the normal map's variance (kc_image_build_roughness_mips, mip.cpp): the two walks of mip.hip --
// mip_steps.h's steps, the one copy every mip unit runs -- with four channels coupled in one thread: the vector of the normals,
// m_x, m_y, m_z, and the roughness r, all four down the plain rule, each level rounded to f32 before the next is made.  What a
// level stores is none of the four but rough(m, r, power) of the header: with l = |m| and t = (1 - l) / l, the plain box r where
// the footprint is flat (t <= 2^-14) or r is NaN, 1 where the normals cancel (l == 0), else
//     te = t - 2^-14,  a2 = clamp01(r)^4,  B = ((2 te) power) (a2 - 1),  d = sqrtf(sqrtf((B - a2) / (B - 1)))
// (tests/mip_roughness_ref.py is the same rule in numpy).  Level 0 of the normals is decoded and normalised texel by texel
// (unit_normal: v = e * 2 - 1, u = v / |v| where 0 < |v| < inf, (0, 0, 1) elsewhere), so u is always finite; below it m lives
// in vector space, never re-encoded and never renormalised: its length is the record of the variance.
//   roughness_pyramid_kernel  mip_pyramid_kernel's tile walk: one workgroup per 64 x 64 source tile, up to six levels; every
//                             level k <= n stores rough() of its four boxes to the one destination plane, and level n also
//                             stores the four boxes themselves to the state planes when further levels follow.
//   roughness_level_kernel    mip_level_kernel's: one level of any size, with the clamps; the same two stores.
// FIRST: the sources are level 0 -- the normal map's R, G, B as stored and the roughness plane, each a resident plane or a
// constant (a value and a bit in the argument block: its loads are that value, its pointer is never formed; channels that alias
// carry one pointer and are loaded once each, from the cache the second time).  Without FIRST they are four state planes.
// sqrtf and / are the build's correctly rounded ones (-fhip-fp32-correctly-rounded-divide-sqrt), nothing is contracted
// (-ffp-contract=off), denormals are kept.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // ld_policy / st_policy
#include "mip_steps.h"  // the box, the tile steps, the one-level walk, the launch checks

// level 0 of the normals: the stored texel (x, y, z) in, the unit vector out
static __device__ __forceinline__ void unit_normal(float &x, float &y, float &z)
{
    const float vx = x * 2.0f - 1.0f, vy = y * 2.0f - 1.0f, vz = z * 2.0f - 1.0f;
    const float l = sqrtf((vx * vx + vy * vy) + vz * vz);
    const bool ok = l > 0.0f && l < __builtin_inff();  // false for NaN
    x = ok ? vx / l : 0.0f;
    y = ok ? vy / l : 0.0f;
    z = ok ? vz / l : 1.0f;
}
// four texels, lane by lane
static __device__ __forceinline__ void unit_normal(mip_f4 &x, mip_f4 &y, mip_f4 &z)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float a = x[j], b = y[j], c = z[j];
        unit_normal(a, b, c);
        x[j] = a;
        y[j] = b;
        z[j] = c;
    }
}

// the stored texel of a level >= 1 from its four boxes
static __device__ __forceinline__ float rough_texel(float mx, float my, float mz, float r, float power)
{
    if (r != r) return r;
    const float l = sqrtf((mx * mx + my * my) + mz * mz);
    if (l == 0.0f) return 1.0f;
    const float t = (1.0f - l) / l;
    if (!(t > 0x1p-14f)) return r;
    const float te = t - 0x1p-14f;
    const float rc = fminf(fmaxf(r, 0.0f), 1.0f), a = rc * rc, a2 = a * a;
    const float B = ((2.0f * te) * power) * (a2 - 1.0f);
    const float n = (B - a2) / (B - 1.0f);
    return sqrtf(sqrtf(n));
}

// Channel c of a first launch: the constant a.cval[c] or the plane a.src[c]; uniform over the launch.
template <class Args, class T, class Const, class Load>
static __device__ __forceinline__ void roughness_channels(const Args &a, T (&v)[4], Const of_const, Load load)
{
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if ((a.const_mask >> c) & 1u) of_const(a.cval[c], v[c]);
        else load(c, v[c]);
    }
}

// mip_steps.h's tile walk on m_x, m_y, m_z and r together, the plain rule on all four: sixteen 16-byte loads issued up front.
template <bool NT, bool FIRST>  // NT: the source does not fit the cache budget: its loads and the level-1 stores are nontemporal
__global__ __launch_bounds__(256) void roughness_pyramid_kernel(const RoughnessPyramidArgs a)
{
    __shared__ float l4[4][16];
    const uint32_t t = threadIdx.x, tx = t & 15u, ty = t >> 4;
    const uint32_t w = a.w, h = a.h, n = a.n;
    const float power = a.power;
    MipRows p[4];
    auto of_const = [](float cv, MipRows &o) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o.r[i] = mip_splat(cv);
    };
    auto load = [&](int c, MipRows &o) __attribute__((always_inline)) { mip_tile_load<NT>(a.src[c], a.src_pitch[c], w, h, tx, ty, o); };
    // four planes, the usual case: sixteen loads and nothing between them
    if (!FIRST || a.const_mask == 0u) MipOwnPlanes()(p, of_const, load);
    else roughness_channels(a, p, of_const, load);
    if constexpr (FIRST) {
#pragma unroll
        for (int i = 0; i < 4; ++i) unit_normal(p[0].r[i], p[1].r[i], p[2].r[i]);
    }
    const bool keep = a.state[0] != nullptr;  // more levels follow: level n's boxes are the next launch's sources
    auto done = [&](uint32_t k, const float (&v)[4][4]) __attribute__((always_inline)) {
        float d[1][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) d[0][i] = (k == 1u || i == 0) ? rough_texel(v[0][i], v[1][i], v[2][i], v[3][i], power) : 0.0f;
        mip_tile_store<NT>(k, d, n, w, h, tx, ty, [&](int, uint32_t j) __attribute__((always_inline)) { return a.dst[j - 1u]; }, a.dst_pitch);
        if (keep && k == n)
            mip_tile_store<NT>(k, v, n, w, h, tx, ty, [&](int c, uint32_t) __attribute__((always_inline)) { return a.state[c]; }, a.dst_pitch);
        return k == 4u && n < 5u;  // levels 2 to 4 are made whatever n is: no branch between the exchanges
    };
    mip_tile_reduce(p, tx, ty, l4, MipPlainRule(), done);
    if (n < 5u) return;  // uniform over the launch: no workgroup meets the barrier
    __syncthreads();
    mip_tile_tail<4>(l4, true, n >= 6u, t, MipPlainRule(), done);
}

// The decode of a first launch in the one-level walk: every source texel of the three normal channels.
struct RoughnessDecode {
    static constexpr bool kNone = false;
    template <class T>
    __device__ __forceinline__ void operator()(MipSrc<T> (&s)[4]) const
    {
        unit_normal(s[0].t0, s[1].t0, s[2].t0);
        unit_normal(s[0].t1, s[1].t1, s[2].t1);
        unit_normal(s[0].b0, s[1].b0, s[2].b0);
        unit_normal(s[0].b1, s[1].b1, s[2].b1);
    }
};

static __device__ __forceinline__ float rough_of(const float (&v)[4], float power) { return rough_texel(v[0], v[1], v[2], v[3], power); }
static __device__ __forceinline__ mip_f4 rough_of(const mip_f4 (&v)[4], float power)
{
    mip_f4 d;
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = rough_texel(v[0][j], v[1][j], v[2][j], v[3][j], power);
    return d;
}

// mip_steps.h's one-level walk on the same four channels; the sink stores rough() and, where a level follows, the boxes.
template <bool NT, bool FIRST>
__global__ __launch_bounds__(256) void roughness_level_kernel(const RoughnessLevelArgs a)
{
    const float power = a.power;
    const bool keep = a.state[0] != nullptr;
    auto channels = [&](auto &v, auto of_const, auto load) __attribute__((always_inline)) {
        if constexpr (FIRST) roughness_channels(a, v, of_const, load);
        else MipOwnPlanes()(v, of_const, load);
    };
    auto sink = [&](size_t o, const auto (&v)[4]) __attribute__((always_inline)) {
        mip_level_store<NT>(a.dst + o, rough_of(v, power));
        if (keep) {
#pragma unroll
            for (int c = 0; c < 4; ++c) mip_level_store<NT>(a.state[c] + o, v[c]);
        }
    };
    if constexpr (FIRST) mip_level_walk<NT, 4>(a.src, a.src_pitch, a.w, a.h, a.dst_pitch, channels, RoughnessDecode(), MipPlainRule(), sink);
    else mip_level_walk<NT, 4>(a.src, a.src_pitch, a.w, a.h, a.dst_pitch, channels, MipNoDecode(), MipPlainRule(), sink);
}

// a first launch: a constant channel reads nothing, a resident one has a plane; at least one of the normals is resident (three
// constants are the plain chain, mip.cpp); below it: four state planes.  The state planes go together.
static bool roughness_args_ok(const float *const src[4], uint32_t const_mask, bool first, float *const state[4])
{
    if (first ? (const_mask & 7u) == 7u || const_mask > 15u : const_mask != 0u) return false;
    for (uint32_t c = 0; c < 4; ++c) {
        if (!((const_mask >> c) & 1u) && !src[c]) return false;
        if ((state[c] != nullptr) != (state[0] != nullptr)) return false;
    }
    return true;
}

hipError_t launch_roughness_pyramid(const RoughnessPyramidArgs &a, bool first, bool nt, hipStream_t s)
{
    dim3 grid;
    if (!roughness_args_ok(a.src, a.const_mask, first, a.state) || !mip_pyramid_grid(a.w, a.h, a.n, 1, &grid)) return hipErrorInvalidValue;
    for (uint32_t j = 0; j < a.n; ++j)
        if (!a.dst[j]) return hipErrorInvalidValue;
    if (first) {
        if (nt) roughness_pyramid_kernel<true, true><<<grid, 256, 0, s>>>(a);
        else roughness_pyramid_kernel<false, true><<<grid, 256, 0, s>>>(a);
    } else {
        if (nt) roughness_pyramid_kernel<true, false><<<grid, 256, 0, s>>>(a);
        else roughness_pyramid_kernel<false, false><<<grid, 256, 0, s>>>(a);
    }
    return hipGetLastError();
}

hipError_t launch_roughness_level(const RoughnessLevelArgs &a, bool first, bool nt, hipStream_t s)
{
    dim3 grid;
    if (!roughness_args_ok(a.src, a.const_mask, first, a.state) || !a.dst || !mip_level_grid(a.w, a.h, 1, &grid)) return hipErrorInvalidValue;
    if (first) {
        if (nt) roughness_level_kernel<true, true><<<grid, 256, 0, s>>>(a);
        else roughness_level_kernel<false, true><<<grid, 256, 0, s>>>(a);
    } else {
        if (nt) roughness_level_kernel<true, false><<<grid, 256, 0, s>>>(a);
        else roughness_level_kernel<false, false><<<grid, 256, 0, s>>>(a);
    }
    return hipGetLastError();
}

}  // namespace kc
