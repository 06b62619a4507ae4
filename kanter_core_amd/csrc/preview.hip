// Previews (kc_image_previews, preview.cpp): rects of mip levels of many images as RGBA8, one launch per pass of the batch.
//   preview_kernel  a 1-D grid over the workgroups of all jobs of a pass; a workgroup finds its job in the prefix table (the
//                   search and the job's fields are wave-uniform, so scalar).
//     n >= 1  the workgroup owns one 64 x 64 source tile and reduces it n levels with the steps mip_pyramid_kernel runs
//             (mip_steps.h, the one copy: in lane, across lanes, 64 bytes of LDS per plane; the loads stay here, their addresses
//             are preview_walk.h's), every distinct resident plane in turn.  Only level n is stored, and
//             only its texels inside the rect: packed R | G << 8 | B << 16 | A << 24 through streaming.h's quantisers (the last
//             pass), or one float per plane into the scratch the next pass reads.  The bits are the level-by-level chain's: the
//             same box in the same order on the same texels, each level rounded to f32 (tests/test_gpu_previews.py ties the two).
//     n == 0  a thread owns four texels of a rect row: a 16-byte load per plane where the address allows, scalar loads otherwise,
//             one to four dword stores.  A job without resident planes (an all-constant image) loads nothing.
// Every index comes from preview_walk.h, which tests/host/preview_walk_check.cpp walks on the CPU.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // quant_u8 / quant_u8_srgb
#include "mip_steps.h"  // the box and the tile steps

// Loads and stores through pointers that come out of the job table: the compiler cannot see that they are global memory and
// would use flat instructions, which count against the LDS / scalar counter as well and hold the cross-lane steps back.
#if defined(__HIP_DEVICE_COMPILE__)
#define PV_GLOBAL __attribute__((address_space(1)))
#else
#define PV_GLOBAL
#endif
template <bool NT, class V>
static __device__ __forceinline__ V pv_ld(const V *p)
{
    const PV_GLOBAL V *g = (const PV_GLOBAL V *)p;
    if constexpr (NT) return __builtin_nontemporal_load(g);
    else return *g;
}
template <class V>
static __device__ __forceinline__ void pv_st(V *p, V v)
{
    *(PV_GLOBAL V *)p = v;
}

static __device__ __forceinline__ float pv_pick(uint32_t s, float v0, float v1, float v2, float v3, float c)
{
    return s == 0u ? v0 : s == 1u ? v1 : s == 2u ? v2 : s == 3u ? v3 : c;
}

// texel (r, g, b, a) as to_u8_kernel packs it: Gray is (v, v, v, 255), alpha stays linear under sRGB
template <bool SRGB>
static __device__ __forceinline__ uint32_t pv_pack(const PreviewJob &J, float v0, float v1, float v2, float v3, const uint32_t *T)
{
    const float r = pv_pick(pw_slot_of(J, 0u), v0, v1, v2, v3, J.cval[0]);
    const uint32_t qr = SRGB ? quant_u8_srgb(r, T) : quant_u8(r);
    if (J.gray) return qr | (qr << 8) | (qr << 16) | (255u << 24);
    const float g = pv_pick(pw_slot_of(J, 1u), v0, v1, v2, v3, J.cval[1]);
    const float b = pv_pick(pw_slot_of(J, 2u), v0, v1, v2, v3, J.cval[2]);
    const float a = pv_pick(pw_slot_of(J, 3u), v0, v1, v2, v3, J.cval[3]);
    const uint32_t qg = SRGB ? quant_u8_srgb(g, T) : quant_u8(g);
    const uint32_t qb = SRGB ? quant_u8_srgb(b, T) : quant_u8(b);
    return qr | (qg << 8) | (qb << 16) | (quant_u8(a) << 24);
}

template <bool SRGB, bool NT>  // NT: the pass's sources do not fit the cache budget (cache_policy_mask, as mip.cpp decides)
__global__ __launch_bounds__(256) void preview_kernel(const PreviewJob *__restrict__ jobs, const uint32_t *__restrict__ prefix, uint32_t count)
{
    __shared__ float l4[4][16];
    __shared__ uint32_t srgb_t[SRGB ? 257 : 1];
    const uint32_t t = threadIdx.x;
    if constexpr (SRGB) {
        srgb_t[t] = kSrgbThresholdBits[t];  // 256 threads
        if (t == 0u) srgb_t[256] = 0xffffffffu;
        __syncthreads();
    }
    const uint32_t ji = pw_find_job(prefix, count, blockIdx.x);
    const PreviewJob &J = jobs[ji];
    const uint32_t local = blockIdx.x - prefix[ji];  // prefix[ji] <= blockIdx.x (pw_find_job)
    const uint32_t n = J.n, np = J.n_planes;

    if (n == 0u) {
        uint32_t X, Y, cnt;
        if (!pw_n0_quad(J, local, t, &X, &Y, &cnt)) return;
        float v[4][4];
#pragma unroll
        for (uint32_t s = 0; s < 4u; ++s) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[s][e] = 0.0f;
            if (s >= np) continue;
            const float *p = J.src[s] + pw_n0_src_offset(J.src_pitch[s], X, Y);
            if (pw_n0_wide(X)) {
                const mip_f4 q = pv_ld<NT>(reinterpret_cast<const mip_f4 *>(p));
#pragma unroll
                for (int e = 0; e < 4; ++e) v[s][e] = q[e];
            } else {
#pragma unroll
                for (uint32_t e = 0; e < 4u; ++e)
                    if (e < cnt) v[s][e] = pv_ld<NT>(p + e);
            }
        }
        size_t off;
        if (!pw_dst_offset(J, X, Y, &off)) return;
        // a level-0 job is always the last pass of its request (pw_plan: the passes that write scratch reduce six levels)
        uint32_t *o = static_cast<uint32_t *>(J.dst[0]) + off;
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e)
            if (e < cnt) pv_st(o + e, pv_pack<SRGB>(J, v[0][e], v[1][e], v[2][e], v[3][e], srgb_t));
        return;
    }

    uint32_t tX, tY;
    pw_tile(J, local, &tX, &tY);
    const uint32_t tx = t & 15u, ty = t >> 4;
    float val[4][4];  // [slot][e]: the level-n values this thread holds (pw_out_texel says which texels they are)
    // The planes in turn through two sets of registers: the next plane's four loads are issued before this one is reduced, so two
    // planes' rows are in flight per thread (np is uniform over the workgroup)
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) val[s][e] = 0.0f;
    auto load = [&](uint32_t s, MipRows &q) __attribute__((always_inline)) {
        const float *src = J.src[s];
        const uint32_t sp = J.src_pitch[s];
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) q.r[i] = pv_ld<NT>(reinterpret_cast<const mip_f4 *>(src + pw_src_offset(J, sp, tX, tY, tx, ty, i)));
    };
    // mip_steps.h's tile walk with the plain rule, one plane at a time; only level n is kept
    auto reduce = [&](const MipRows (&q)[1], uint32_t s) __attribute__((always_inline)) {
        mip_tile_reduce(q, tx, ty, l4 + s, MipPlainRule(), [&](uint32_t k, const float (&v)[1][4]) __attribute__((always_inline)) {
            if (k != n) return false;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e == 0 || k == 1u) val[s][e] = v[0][e];
            return true;
        });
    };
    MipRows pa[1], pb[1];
    load(0u, pa[0]);
    if (np > 1u) load(1u, pb[0]);
    reduce(pa, 0u);
    if (np > 1u) {
        if (np > 2u) load(2u, pa[0]);
        reduce(pb, 1u);
        if (np > 2u) {
            if (np > 3u) load(3u, pb[0]);
            reduce(pa, 2u);
            if (np > 3u) reduce(pb, 3u);
        }
    }
    if (n >= 5u) {  // uniform over the workgroup
        __syncthreads();
#pragma unroll
        for (uint32_t s = 0; s < 4u; ++s) {
            if (s >= np) continue;
            mip_tile_tail<1>(l4 + s, n == 5u, n == 6u, t, MipPlainRule(),
                             [&](uint32_t, const float (&v)[1][4]) __attribute__((always_inline)) { val[s][0] = v[0][0]; });
        }
    }
#pragma unroll
    for (uint32_t e = 0; e < 4u; ++e) {
        uint32_t X, Y;
        size_t off;
        if (!pw_out_texel(n, tX, tY, t, e, &X, &Y) || !pw_dst_offset(J, X, Y, &off)) continue;
        if (J.last) {
            pv_st(static_cast<uint32_t *>(J.dst[0]) + off, pv_pack<SRGB>(J, val[0][e], val[1][e], val[2][e], val[3][e], srgb_t));
        } else {
#pragma unroll
            for (uint32_t s = 0; s < 4u; ++s)
                if (s < np) pv_st(static_cast<float *>(J.dst[s]) + off, val[s][e]);
        }
    }
}

hipError_t launch_preview(const PreviewJob *jobs, const uint32_t *prefix, uint32_t count, uint32_t workgroups, bool srgb, bool nt, hipStream_t s)
{
    if (!jobs || !prefix || count == 0 || workgroups == 0 || workgroups > 0x7fffffffu) return hipErrorInvalidValue;
    const dim3 grid(workgroups);
    if (srgb && nt) preview_kernel<true, true><<<grid, 256, 0, s>>>(jobs, prefix, count);
    else if (srgb) preview_kernel<true, false><<<grid, 256, 0, s>>>(jobs, prefix, count);
    else if (nt) preview_kernel<false, true><<<grid, 256, 0, s>>>(jobs, prefix, count);
    else preview_kernel<false, false><<<grid, 256, 0, s>>>(jobs, prefix, count);
    return hipGetLastError();
}

}  // namespace kc
