// Alpha-weighted mip chains (KC_MIP_ALPHA_WEIGHT, mip.cpp): the colour of a level is the alpha-weighted average of the texels
// under it, and the texels that have no weight are filled from the coarser levels (pull-push).  The pull is the two walks of
// mip.hip -- mip_steps.h's steps, the one copy every mip unit runs -- with four channels coupled in one thread: the premultiplied
// colour p_r, p_g, p_b and the weight w, all four down the plain rule, each level rounded to f32 before the next is made.  What
// a level stores is q_c = W > 0 ? P_c / W : 0 in its three colour planes and W in a scratch plane (tests/mip_alpha_ref.py is the
// same rule in numpy).
//   alpha_pull_pyramid_kernel  mip_pyramid_kernel's tile walk: one workgroup per 64 x 64 source tile, up to six levels; level n
//                              also stores P_c to the state planes when further levels follow (its W is already in the scratch).
//   alpha_pull_level_kernel    mip_level_kernel's: one level of any size, with the clamps; the same stores.
//   alpha_push_kernel          one thread per quad of every level: an unknown texel (level 0: a <= 0 or NaN; below: W <= 0) takes
//                              the three colours of its nearest ancestor with a positive weight, or keeps the pull's 0; the
//                              weights of the first three ancestor levels are loaded together, the walk is the rare rest.
// FIRST: the sources are level 0 -- R, G, B and alpha as stored, each a resident plane or a constant (a value and a bit in the
// argument block: its loads are that value, its pointer is never formed; channels that alias carry one pointer and are loaded
// once each, from the cache the second time).  Right after the loads w0 = a > 0 ? min(a, 1) : 0 and p_c = w0 > 0 ? c * w0 : 0
// (a select: nothing under a transparent texel enters), and the thread stores level 0's colour, c where w0 > 0 and 0 elsewhere,
// to planes of its own.  Without FIRST the sources are the three state planes and the weight plane of the level read.
// / is the build's correctly rounded one (-fhip-fp32-correctly-rounded-divide-sqrt), nothing is contracted (-ffp-contract=off),
// denormals are kept.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // ld_policy / st_policy
#include "mip_steps.h"  // the box, the tile steps, the one-level walk, the launch checks

static __device__ __forceinline__ float alpha_weight(float a)
{
    if (!(a > 0.0f)) return 0.0f;  // NaN, -0.0 and negatives
    return a < 1.0f ? a : 1.0f;
}

// level 0 of one texel: (r, g, b, a) as stored in, (p_r, p_g, p_b, w0) out; l0: what level 0 stores for the colour
static __device__ __forceinline__ void alpha_premultiply(float &r, float &g, float &b, float &a, float (&l0)[3])
{
    const float w0 = alpha_weight(a);
    const bool known = w0 > 0.0f;
    l0[0] = known ? r : 0.0f;
    l0[1] = known ? g : 0.0f;
    l0[2] = known ? b : 0.0f;
    r = known ? r * w0 : 0.0f;
    g = known ? g * w0 : 0.0f;
    b = known ? b * w0 : 0.0f;
    a = w0;
}
static __device__ __forceinline__ void alpha_premultiply(float &r, float &g, float &b, float &a)
{
    float l0[3];
    alpha_premultiply(r, g, b, a, l0);
}
// four texels, lane by lane
static __device__ __forceinline__ void alpha_premultiply(mip_f4 &r, mip_f4 &g, mip_f4 &b, mip_f4 &a)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float x = r[j], y = g[j], z = b[j], w = a[j];
        alpha_premultiply(x, y, z, w);
        r[j] = x;
        g[j] = y;
        b[j] = z;
        a[j] = w;
    }
}

// the stored colour of a level >= 1 from its boxes
static __device__ __forceinline__ float alpha_texel(float p, float w) { return w > 0.0f ? p / w : 0.0f; }
static __device__ __forceinline__ mip_f4 alpha_texel(mip_f4 p, mip_f4 w)
{
    return mip_f4{ alpha_texel(p[0], w[0]), alpha_texel(p[1], w[1]), alpha_texel(p[2], w[2]), alpha_texel(p[3], w[3]) };
}

// Channel c of a first launch: the constant a.cval[c] or the plane a.src[c]; uniform over the launch.
template <class Args, class T, class Const, class Load>
static __device__ __forceinline__ void alpha_channels(const Args &a, T (&v)[4], Const of_const, Load load)
{
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if ((a.const_mask >> c) & 1u) of_const(a.cval[c], v[c]);
        else load(c, v[c]);
    }
}

// mip_steps.h's tile walk on p_r, p_g, p_b and w together, the plain rule on all four: sixteen 16-byte loads issued up front.
template <bool NT, bool FIRST>  // NT: the source does not fit the cache budget: its loads and the level-0 and level-1 stores are nontemporal
__global__ __launch_bounds__(256) void alpha_pull_pyramid_kernel(const AlphaPullPyramidArgs a)
{
    __shared__ float l4[4][16];
    const uint32_t t = threadIdx.x, tx = t & 15u, ty = t >> 4;
    const uint32_t w = a.w, h = a.h, n = a.n;
    MipRows p[4];
    auto of_const = [](float cv, MipRows &o) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o.r[i] = mip_splat(cv);
    };
    auto load = [&](int c, MipRows &o) __attribute__((always_inline)) { mip_tile_load<NT>(a.src[c], a.src_pitch[c], w, h, tx, ty, o); };
    // four planes, the usual case: sixteen loads and nothing between them
    if (!FIRST || a.const_mask == 0u) MipOwnPlanes()(p, of_const, load);
    else alpha_channels(a, p, of_const, load);
    if constexpr (FIRST) {
        // the thread's own texels of level 0: columns 4 qx .. 4 qx + 3 of rows y0 .. y0 + 3.  A thread whose loads were clamped
        // lies outside the image and stores nothing.
        const uint32_t qx = blockIdx.x * 16u + tx, y0 = blockIdx.y * 64u + 4u * ty;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            mip_f4 l0[3];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float r = p[0].r[i][j], g = p[1].r[i][j], b = p[2].r[i][j], al = p[3].r[i][j], c0[3];
                alpha_premultiply(r, g, b, al, c0);
                p[0].r[i][j] = r;
                p[1].r[i][j] = g;
                p[2].r[i][j] = b;
                p[3].r[i][j] = al;
#pragma unroll
                for (int c = 0; c < 3; ++c) l0[c][j] = c0[c];
            }
            const uint32_t y = y0 + (uint32_t)i;
            if (y < h && 4u * qx < w) {
                const size_t o = (size_t)y * a.dst0_pitch + 4u * qx;
                if (4u * qx + 3u < w) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) st_policy<NT>(reinterpret_cast<mip_f4 *>(a.dst0[c] + o), l0[c]);
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
#pragma unroll
                        for (int j = 0; j < 3; ++j)
                            if (4u * qx + (uint32_t)j < w) a.dst0[c][o + j] = l0[c][j];
                }
            }
        }
    }
    const bool keep = a.state[0] != nullptr;  // more levels follow: level n's P are the next launch's sources, beside its W
    auto done = [&](uint32_t k, const float (&v)[4][4]) __attribute__((always_inline)) {
        float d[4][4], s[3][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool live = k == 1u || i == 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                d[c][i] = live ? alpha_texel(v[c][i], v[3][i]) : 0.0f;
                s[c][i] = v[c][i];
            }
            d[3][i] = v[3][i];
        }
        mip_tile_store<NT>(k, d, n, w, h, tx, ty,
                           [&](int c, uint32_t j) __attribute__((always_inline)) { return c < 3 ? a.dst[c][j - 1u] : a.wdst[j - 1u]; }, a.dst_pitch);
        if (keep && k == n)
            mip_tile_store<NT>(k, s, n, w, h, tx, ty, [&](int c, uint32_t) __attribute__((always_inline)) { return a.state[c]; }, a.dst_pitch);
        return k == 4u && n < 5u;  // levels 2 to 4 are made whatever n is: no branch between the exchanges
    };
    mip_tile_reduce(p, tx, ty, l4, MipPlainRule(), done);
    if (n < 5u) return;  // uniform over the launch: no workgroup meets the barrier
    __syncthreads();
    mip_tile_tail<4>(l4, true, n >= 6u, t, MipPlainRule(), done);
}

// The decode of a first launch in the one-level walk: the weight and the premultiplication of every source texel.
struct AlphaDecode {
    static constexpr bool kNone = false;
    template <class T>
    __device__ __forceinline__ void operator()(MipSrc<T> (&s)[4]) const
    {
        alpha_premultiply(s[0].t0, s[1].t0, s[2].t0, s[3].t0);
        alpha_premultiply(s[0].t1, s[1].t1, s[2].t1, s[3].t1);
        alpha_premultiply(s[0].b0, s[1].b0, s[2].b0, s[3].b0);
        alpha_premultiply(s[0].b1, s[1].b1, s[2].b1, s[3].b1);
    }
};

// Level 0's colour in a first one-level launch.  The thread of the output quad (y, q) owns source rows 2 y, 2 y + 1 and columns
// 8 q .. 8 q + 7; the threads of the last output row and of a row's last quad also own what the box drops or clamps, through
// row h - 1 and column w - 1, so that every texel of level 0 has exactly one owner (w == 1 or h == 1: the one row or column).
// This form runs under KC_MIP_PER_LEVEL and on images one texel wide or high; it reads the texels again, from the cache.
static __device__ __forceinline__ void alpha_level0_copy(const AlphaPullLevelArgs &a)
{
    const uint32_t w = a.w, h = a.h;
    const uint32_t W = max(w >> 1, 1u), H = max(h >> 1, 1u), quads = (W + 3u) / 4u;
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= quads * H) return;
    const uint32_t y = idx / quads, q = idx - y * quads;
    const uint32_t r0 = 2u * y, r1 = y == H - 1u ? h : 2u * y + 2u;
    const uint32_t x0 = 8u * q, x1 = q == quads - 1u ? w : 8u * q + 8u;
    const uint32_t m = a.const_mask, pr = a.src_pitch[0], pg = a.src_pitch[1], pb = a.src_pitch[2], pa = a.src_pitch[3];
    const float vr = a.cval[0], vg = a.cval[1], vb = a.cval[2], va = a.cval[3];
    const float *sr = a.src[0], *sg = a.src[1], *sb = a.src[2], *sa = a.src[3];
    float *dr = a.dst0[0], *dg = a.dst0[1], *db = a.dst0[2];
    for (uint32_t r = r0; r < r1; ++r)
        for (uint32_t x = x0; x < x1; ++x) {
            const float cr = (m & 1u) ? vr : sr[(size_t)r * pr + x];
            const float cg = (m & 2u) ? vg : sg[(size_t)r * pg + x];
            const float cb = (m & 4u) ? vb : sb[(size_t)r * pb + x];
            const float ca = (m & 8u) ? va : sa[(size_t)r * pa + x];
            const bool known = alpha_weight(ca) > 0.0f;
            const size_t o = (size_t)r * a.dst0_pitch + x;
            dr[o] = known ? cr : 0.0f;
            dg[o] = known ? cg : 0.0f;
            db[o] = known ? cb : 0.0f;
        }
}

// mip_steps.h's one-level walk on the same four channels; the sink stores q and W and, where a level follows, P.
template <bool NT, bool FIRST>
__global__ __launch_bounds__(256) void alpha_pull_level_kernel(const AlphaPullLevelArgs a)
{
    if constexpr (FIRST) {
        alpha_level0_copy(a);
        if (!a.wdst) return;  // a 1 x 1 image: no level below it
    }
    const bool keep = a.state[0] != nullptr;
    auto channels = [&](auto &v, auto of_const, auto load) __attribute__((always_inline)) {
        if constexpr (FIRST) alpha_channels(a, v, of_const, load);
        else MipOwnPlanes()(v, of_const, load);
    };
    auto sink = [&](size_t o, const auto (&v)[4]) __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < 3; ++c) mip_level_store<NT>(a.dst[c] + o, alpha_texel(v[c], v[3]));
        mip_level_store<NT>(a.wdst + o, v[3]);
        if (keep) {
#pragma unroll
            for (int c = 0; c < 3; ++c) mip_level_store<NT>(a.state[c] + o, v[c]);
        }
    };
    if constexpr (FIRST) mip_level_walk<NT, 4>(a.src, a.src_pitch, a.w, a.h, a.dst_pitch, channels, AlphaDecode(), MipPlainRule(), sink);
    else mip_level_walk<NT, 4>(a.src, a.src_pitch, a.w, a.h, a.dst_pitch, channels, MipNoDecode(), MipPlainRule(), sink);
}

// The push.  Workgroup -> level through first_wg, which rises with the level; a thread takes a quad of that level.  Rows are
// readable in whole quads, so the weights of a row's last partial quad are one load too; the texels past the row count as known.
// Texels 0, 1 and texels 2, 3 of a quad each share their ancestor of the next level, and all four share every ancestor above
// it; where an ancestor lies depends on the coordinates alone, so the weights of the first three ancestor levels are loaded
// together, before any of them is looked at, and only the colours wait for the choice.  Levels further up (rare: a hole wider
// than eight texels) are walked one by one.  Only unknown texels are written, and only known texels' colours and the weights
// are read: nothing read here is written here.
__global__ __launch_bounds__(256) void alpha_push_kernel(const AlphaPushArgs a)
{
    const uint32_t wg = blockIdx.x, L = a.levels;
    uint32_t j = 0;
    while (j + 1u < L && wg >= a.jobs[j + 1u].first_wg) ++j;
    const AlphaPushJob J = a.jobs[j];
    if (!J.wsrc) return;  // uniform: a constant alpha of positive weight, every texel of level 0 is known
    const uint32_t row_units = (J.w + 3u) / 4u;
    const uint32_t idx = (wg - J.first_wg) * 256u + threadIdx.x;
    if (idx >= row_units * J.h) return;
    const uint32_t y = idx / row_units, q = idx - y * row_units, px = 4u * q;
    const mip_f4 wv = *reinterpret_cast<const mip_f4 *>(J.wsrc + (size_t)y * J.w_pitch + px);
    const uint32_t valid = min(J.w - px, 4u);
    bool unknown[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) unknown[x] = (uint32_t)x < valid && !(wv[x] > 0.0f);  // NaN: unknown
    const bool need_a = unknown[0] || unknown[1], need_b = unknown[2] || unknown[3];
    if (!need_a && !need_b) return;
    // the ancestor of column x at level jj > j: floats into a plane of that level whose rows are `pitch` floats apart
    auto at = [&](uint32_t jj, uint32_t x, uint32_t pitch) __attribute__((always_inline)) {
        const uint32_t s = jj - j;
        return (size_t)min(y >> s, a.jobs[jj].h - 1u) * pitch + min(x >> s, a.jobs[jj].w - 1u);
    };
    auto weight = [&](uint32_t jj, uint32_t x) __attribute__((always_inline)) { return a.jobs[jj].wsrc[at(jj, x, a.jobs[jj].w_pitch)]; };
    float w1a = 0.0f, w1b = 0.0f, w2 = 0.0f, w3 = 0.0f;  // uniform conditions: j is the workgroup's
    if (j + 1u < L) {
        w1a = weight(j + 1u, px);
        w1b = weight(j + 1u, px + 2u);  // past a partial quad's row: clamped, and not looked at
    }
    if (j + 2u < L) w2 = weight(j + 2u, px);
    if (j + 3u < L) w3 = weight(j + 3u, px);
    // the first level above j whose ancestor has a positive weight; 0: none, the texel keeps the pull's 0
    auto first_known = [&](float w1) __attribute__((always_inline)) -> uint32_t {
        if (w1 > 0.0f) return j + 1u;
        if (w2 > 0.0f) return j + 2u;
        if (w3 > 0.0f) return j + 3u;
        for (uint32_t jj = j + 4u; jj < L; ++jj)
            if (weight(jj, px) > 0.0f) return jj;
        return 0u;
    };
    const uint32_t la = need_a ? first_known(w1a) : 0u, lb = need_b ? first_known(w1b) : 0u;
    // the three colours of column x's ancestor at level jj; the first three levels through the workgroup's own table entries
    auto colours = [&](uint32_t jj, uint32_t x, float (&c)[3]) __attribute__((always_inline)) {
        const float *src[3];
#pragma unroll
        for (uint32_t s = 1u; s <= 3u; ++s)
            if (jj == j + s) {
                const size_t o = at(j + s, x, a.jobs[j + s].dst_pitch);
#pragma unroll
                for (int k = 0; k < 3; ++k) src[k] = a.jobs[j + s].dst[k] + o;
            }
        if (jj > j + 3u) {
            const size_t o = at(jj, x, a.jobs[jj].dst_pitch);
#pragma unroll
            for (int k = 0; k < 3; ++k) src[k] = a.jobs[jj].dst[k] + o;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = *src[k];
    };
    float ca[3] = { 0.0f, 0.0f, 0.0f }, cb[3] = { 0.0f, 0.0f, 0.0f };
    if (la) colours(la, px, ca);
    if (lb) {
        if (lb == la && lb >= j + 2u) {  // one ancestor for the whole quad
#pragma unroll
            for (int k = 0; k < 3; ++k) cb[k] = ca[k];
        } else {
            colours(lb, px + 2u, cb);
        }
    }
    const size_t to = (size_t)y * J.dst_pitch + px;
    if (la && lb && unknown[0] && unknown[1] && unknown[2] && unknown[3]) {  // a whole quad, all of it unknown
#pragma unroll
        for (int k = 0; k < 3; ++k) *reinterpret_cast<mip_f4 *>(J.dst[k] + to) = mip_f4{ ca[k], ca[k], cb[k], cb[k] };
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (la && unknown[0]) J.dst[k][to] = ca[k];
        if (la && unknown[1]) J.dst[k][to + 1u] = ca[k];
        if (lb && unknown[2]) J.dst[k][to + 2u] = cb[k];
        if (lb && unknown[3]) J.dst[k][to + 3u] = cb[k];
    }
}

// a first launch: a constant channel reads nothing, a resident one has a plane, and level 0's colour has its three planes;
// below it: three state planes and the weight plane.  The state planes go together.
template <class Args>
static bool alpha_pull_args_ok(const Args &a, bool first)
{
    if (first ? a.const_mask > 15u : a.const_mask != 0u) return false;
    for (uint32_t c = 0; c < 4; ++c)
        if (!((a.const_mask >> c) & 1u) && !a.src[c]) return false;
    for (uint32_t c = 0; c < 3; ++c) {
        if ((a.state[c] != nullptr) != (a.state[0] != nullptr)) return false;
        if (first && !a.dst0[c]) return false;
    }
    return !first || a.dst0_pitch >= a.w;
}

hipError_t launch_alpha_pull_pyramid(const AlphaPullPyramidArgs &a, bool first, bool nt, hipStream_t s)
{
    dim3 grid;
    if (!alpha_pull_args_ok(a, first) || !mip_pyramid_grid(a.w, a.h, a.n, 1, &grid)) return hipErrorInvalidValue;
    for (uint32_t j = 0; j < a.n; ++j)
        if (!a.dst[0][j] || !a.dst[1][j] || !a.dst[2][j] || !a.wdst[j]) return hipErrorInvalidValue;
    if (first) {
        if (nt) alpha_pull_pyramid_kernel<true, true><<<grid, 256, 0, s>>>(a);
        else alpha_pull_pyramid_kernel<false, true><<<grid, 256, 0, s>>>(a);
    } else {
        if (nt) alpha_pull_pyramid_kernel<true, false><<<grid, 256, 0, s>>>(a);
        else alpha_pull_pyramid_kernel<false, false><<<grid, 256, 0, s>>>(a);
    }
    return hipGetLastError();
}

hipError_t launch_alpha_pull_level(const AlphaPullLevelArgs &a, bool first, bool nt, hipStream_t s)
{
    dim3 grid;
    if (!alpha_pull_args_ok(a, first)) return hipErrorInvalidValue;
    if (first && a.w == 1 && a.h == 1) {  // level 0 alone: one thread
        if (a.wdst || a.dst[0] || a.dst[1] || a.dst[2] || a.state[0]) return hipErrorInvalidValue;
        grid = dim3(1);
    } else if (!a.wdst || !a.dst[0] || !a.dst[1] || !a.dst[2] || !mip_level_grid(a.w, a.h, 1, &grid)) {
        return hipErrorInvalidValue;
    }
    if (first) {
        if (nt) alpha_pull_level_kernel<true, true><<<grid, 256, 0, s>>>(a);
        else alpha_pull_level_kernel<false, true><<<grid, 256, 0, s>>>(a);
    } else {
        if (nt) alpha_pull_level_kernel<true, false><<<grid, 256, 0, s>>>(a);
        else alpha_pull_level_kernel<false, false><<<grid, 256, 0, s>>>(a);
    }
    return hipGetLastError();
}

hipError_t launch_alpha_push(const AlphaPushArgs &a, uint32_t wgs, hipStream_t s)
{
    if (a.levels < 1 || a.levels > KC_ALPHA_MAX_LEVELS || wgs == 0 || wgs > 0x7fffffffu) return hipErrorInvalidValue;
    uint32_t at = 0;
    for (uint32_t k = 0; k < a.levels; ++k) {
        const AlphaPushJob &J = a.jobs[k];
        if (!J.dst[0] || !J.dst[1] || !J.dst[2] || (k && !J.wsrc) || J.w == 0 || J.h == 0 || J.dst_pitch < J.w || (J.wsrc && J.w_pitch < J.w))
            return hipErrorInvalidValue;
        if (J.first_wg != at || J.wgs != alpha_push_job_wgs(J.w, J.h)) return hipErrorInvalidValue;
        at += J.wgs;
    }
    if (at != wgs) return hipErrorInvalidValue;
    alpha_push_kernel<<<dim3(wgs), 256, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace kc
