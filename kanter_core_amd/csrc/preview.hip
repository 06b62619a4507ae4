// Previews (kc_image_previews, preview.cpp): rects of mip levels of many images as RGBA8, one launch per pass of the batch.
//   preview_kernel  a 1-D grid over the workgroups of all jobs of a pass; a workgroup finds its job in the prefix table (the
//                   search and the job's fields are wave-uniform, so scalar).
//     n >= 1  the workgroup owns one 64 x 64 source tile and reduces it n levels with mip_pyramid_kernel's steps (mip.hip: in
//             lane, across lanes, 64 bytes of LDS per plane), every distinct resident plane in turn.  Only level n is stored, and
//             only its texels inside the rect: packed R | G << 8 | B << 16 | A << 24 through streaming.h's quantisers (the last
//             pass), or one float per plane into the scratch the next pass reads.  The bits are the level-by-level chain's: the
//             same box in the same order on the same texels, each level rounded to f32 (tests/test_gpu_previews.py ties the two).
//     n == 0  a thread owns four texels of a rect row: a 16-byte load per plane where the address allows, scalar loads otherwise,
//             one to four dword stores.  A job without resident planes (an all-constant image) loads nothing.
// Every index comes from preview_walk.h, which tests/host/preview_walk_check.cpp walks on the CPU.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // quant_u8 / quant_u8_srgb

typedef float pv_f4 __attribute__((ext_vector_type(4)));

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

static __device__ __forceinline__ float pv_box(float a, float b, float c, float d) { return ((a + b) + (c + d)) * 0.25f; }

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

// mip_pyramid_kernel's steps on one plane's 4 x 4 texels per thread, down to level n (1 .. 6, uniform over the workgroup): v = the
// level-n values of levels 1 to 4 (level 1: the 2 x 2 patch, row-major; levels 2 to 4: v[0], for levels 3 and 4 valid in the
// lanes whose tx and ty are multiples of 2 and 4); for levels 5 and 6 the 4 x 4 level-4 values go to l4 and the caller finishes
// behind one barrier.  Every lane takes part, in range or not: the exchanges need all 64 lanes of a wave.
static __device__ __forceinline__ void pv_reduce(const pv_f4 (&p)[4], uint32_t n, uint32_t tx, uint32_t ty, float *l4, float (&v)[4])
{
    float v1[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        v1[r][0] = pv_box(p[2 * r][0], p[2 * r][1], p[2 * r + 1][0], p[2 * r + 1][1]);
        v1[r][1] = pv_box(p[2 * r][2], p[2 * r][3], p[2 * r + 1][2], p[2 * r + 1][3]);
    }
    if (n == 1u) {
        v[0] = v1[0][0];
        v[1] = v1[0][1];
        v[2] = v1[1][0];
        v[3] = v1[1][1];
        return;
    }
    const float v2 = pv_box(v1[0][0], v1[0][1], v1[1][0], v1[1][1]);
    if (n == 2u) {
        v[0] = v2;
        return;
    }
    float hs = v2 + __shfl_xor(v2, 1, 64);
    const float v3 = (hs + __shfl_xor(hs, 16, 64)) * 0.25f;
    if (n == 3u) {
        v[0] = v3;
        return;
    }
    hs = v3 + __shfl_xor(v3, 2, 64);
    const float v4 = (hs + __shfl_xor(hs, 32, 64)) * 0.25f;
    if (n == 4u) {
        v[0] = v4;
        return;
    }
    if (!(tx & 3u) && !(ty & 3u)) l4[(ty >> 2) * 4u + (tx >> 2)] = v4;
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
                const pv_f4 q = pv_ld<NT>(reinterpret_cast<const pv_f4 *>(p));
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
    auto load = [&](uint32_t s, pv_f4 (&q)[4]) {
        const float *src = J.src[s];
        const uint32_t sp = J.src_pitch[s];
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) q[i] = pv_ld<NT>(reinterpret_cast<const pv_f4 *>(src + pw_src_offset(J, sp, tX, tY, tx, ty, i)));
    };
    pv_f4 pa[4], pb[4];
    load(0u, pa);
    if (np > 1u) load(1u, pb);
    pv_reduce(pa, n, tx, ty, l4[0], val[0]);
    if (np > 1u) {
        if (np > 2u) load(2u, pa);
        pv_reduce(pb, n, tx, ty, l4[1], val[1]);
        if (np > 2u) {
            if (np > 3u) load(3u, pb);
            pv_reduce(pa, n, tx, ty, l4[2], val[2]);
            if (np > 3u) pv_reduce(pb, n, tx, ty, l4[3], val[3]);
        }
    }
    if (n >= 5u) {  // uniform over the workgroup
        __syncthreads();
#pragma unroll
        for (uint32_t s = 0; s < 4u; ++s) {
            if (s >= np) continue;
            if (n == 5u) {
                if (t < 4u) {
                    const float *q = l4[s] + 8u * (t >> 1) + 2u * (t & 1u);
                    val[s][0] = pv_box(q[0], q[1], q[4], q[5]);
                }
            } else if (t == 0u) {
                float v5[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float *q = l4[s] + 8 * (k >> 1) + 2 * (k & 1);
                    v5[k] = pv_box(q[0], q[1], q[4], q[5]);
                }
                val[s][0] = pv_box(v5[0], v5[1], v5[2], v5[3]);
            }
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
