// Mip chains of normal maps (KC_MIP_NORMALS; kc_image_build_mips, mip.cpp): the two walks of mip.hip -- mip_steps.h's steps, the
// one copy both units run -- with R, G, B coupled in one thread and normal_texel as the rule.  A texel of level k is the 2 x 2
// box of each channel (mip.hip's expression and clamps), then, on the three boxes b,
//     v = b * 2.0f - 1.0f,   l = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z),   u = l > 0 && l < inf ? v / l : (0, 0, 1),   d = u * 0.5f + 0.5f
// -- every level normalised and rounded to f32 before the next is made, so the fused kernel and the level-by-level one give the
// same bits (tests/mip_normals_ref.py is the same rule in numpy).  The comparison is false for NaN: a zero vector, an
// underflowed or overflowed sum and a NaN or infinity in any channel all store (0.5, 0.5, 1.0), and no level >= 1 holds a NaN.
//   normal_pyramid_kernel  mip_pyramid_kernel's tile walk: one workgroup per 64 x 64 source tile, up to six levels.  In the
//                          cross-lane steps every lane of an exchange group holds bit-equal sums (f32 addition commutes) and
//                          normalises its own copy, so the groups stay bit-equal all the way down.
//   normal_level_kernel    mip_level_kernel's: one level of any size, with the clamps.
// A channel is a resident plane, a constant (a value and a bit in the argument block: its loads are that value, its pointer is
// never formed) or the loads of an earlier channel that aliases it (mip_steps.h's normal_channels, for the pyramid's loads and
// both paths of the one-level step); all three are uniform over the launch, and three planes of their own -- every level >= 1,
// every HeightToNormal result -- take a path without those branches.  sqrtf and / are
// the build's correctly rounded ones (-fhip-fp32-correctly-rounded-divide-sqrt), nothing is contracted (-ffp-contract=off).
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // ld_policy / st_policy
#include "mip_steps.h"  // the box, the tile steps, the one-level step, normal_channels, the launch checks

// b: the boxes of R, G, B in, the stored texel out
static __device__ __forceinline__ void normal_texel(float (&b)[3])
{
    const float vx = b[0] * 2.0f - 1.0f, vy = b[1] * 2.0f - 1.0f, vz = b[2] * 2.0f - 1.0f;
    const float l = sqrtf((vx * vx + vy * vy) + vz * vz);
    float ux = 0.0f, uy = 0.0f, uz = 1.0f;
    if (l > 0.0f && l < __builtin_inff()) {  // false for NaN
        ux = vx / l;
        uy = vy / l;
        uz = vz / l;
    }
    b[0] = ux * 0.5f + 0.5f;
    b[1] = uy * 0.5f + 0.5f;
    b[2] = uz * 0.5f + 0.5f;
}

// mip_steps.h's tile walk on R, G, B together, normal_texel at every level: twelve 16-byte loads issued up front, every level up
// to n (1..6) stored.
template <bool NT>  // NT: the source does not fit the cache budget: its loads and the level-1 stores are nontemporal
__global__ __launch_bounds__(256) void normal_pyramid_kernel(const NormalPyramidArgs a)
{
    __shared__ float l4[3][16];
    const uint32_t t = threadIdx.x, tx = t & 15u, ty = t >> 4;
    const uint32_t w = a.w, h = a.h, n = a.n;
    MipRows p[3];
    auto of_const = [](float cv, MipRows &o) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o.r[i] = mip_splat(cv);
    };
    auto load = [&](int c, MipRows &o) __attribute__((always_inline)) { mip_tile_load<NT>(a.src[c], a.src_pitch[c], w, h, tx, ty, o); };
    // three planes, the usual case: twelve loads and nothing between them
    if (a.const_mask == 0u && a.from == kNormalOwnPlanes) MipOwnPlanes()(p, of_const, load);
    else normal_channels(a, p, of_const, load);
    auto rule = [](float (&b)[3]) __attribute__((always_inline)) { normal_texel(b); };
    auto done = [&](uint32_t k, const float (&v)[3][4]) __attribute__((always_inline)) {
        mip_tile_store<NT>(k, v, n, w, h, tx, ty, [&](int c, uint32_t j) __attribute__((always_inline)) { return a.dst[c][j - 1u]; }, a.dst_pitch);
        return k == 4u && n < 5u;  // levels 2 to 4 are made whatever n is: no branch between the exchanges
    };
    mip_tile_reduce(p, tx, ty, l4, rule, done);
    if (n < 5u) return;  // uniform over the launch: no workgroup meets the barrier
    __syncthreads();
    mip_tile_tail<3>(l4, true, n >= 6u, t, rule, done);
}

// mip_steps.h's one-level step on R, G, B together, normal_texel on every texel.
template <bool NT>
__global__ __launch_bounds__(256) void normal_level_kernel(const NormalLevelArgs a)
{
    mip_level_step<NT, 3>(a.src, a.src_pitch, a.w, a.h, a.dst, a.dst_pitch, [](float (&b)[3]) __attribute__((always_inline)) { normal_texel(b); },
                          [&](auto &v, auto of_const, auto load) __attribute__((always_inline)) { normal_channels(a, v, of_const, load); });
}

// const_mask and `from` are consistent: a constant channel reads nothing, an aliasing channel names an earlier resident one
static bool normal_channels_ok(const float *const src[3], uint32_t const_mask, uint32_t from)
{
    if (const_mask >= 7u) return false;  // three constants are folded on the host
    for (uint32_t c = 0; c < 3; ++c) {
        const uint32_t f = (from >> (2 * c)) & 3u;
        if ((const_mask >> c) & 1u) continue;
        if (f > c || ((const_mask >> f) & 1u) || ((from >> (2 * f)) & 3u) != f) return false;
        if (f == c && !src[c]) return false;
    }
    return true;
}

hipError_t launch_normal_pyramid(const NormalPyramidArgs &a, bool nt, hipStream_t s)
{
    dim3 grid;
    if (!normal_channels_ok(a.src, a.const_mask, a.from) || !mip_pyramid_grid(a.w, a.h, a.n, 1, &grid)) return hipErrorInvalidValue;
    if (nt) normal_pyramid_kernel<true><<<grid, 256, 0, s>>>(a);
    else normal_pyramid_kernel<false><<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_normal_level(const NormalLevelArgs &a, bool nt, hipStream_t s)
{
    dim3 grid;
    if (!normal_channels_ok(a.src, a.const_mask, a.from) || !mip_level_grid(a.w, a.h, 1, &grid)) return hipErrorInvalidValue;
    if (nt) normal_level_kernel<true><<<grid, 256, 0, s>>>(a);
    else normal_level_kernel<false><<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace kc
