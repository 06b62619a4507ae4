// Mip chains (kc_image_build_mips, mip.cpp): the 2x2 box of include/kanter_core_amd.h,
//     d(x, y) = ((s(x0, y0) + s(x1, y0)) + (s(x0, y1) + s(x1, y1))) * 0.25f,   x0 = 2x, x1 = min(2x + 1, w - 1), y likewise,
// three f32 additions in that order and one multiplication, every level rounded to f32 before the next is made -- so the fused
// kernel and the level-by-level one give the same bits (tests/mip_ref.py is the same rule in numpy).
//   mip_pyramid_kernel  one workgroup carries a 64 x 64 tile of the source level down up to six levels: while both extents
//                       still halve, texel (x, y) of level k is a function of the source texels [x 2^k, (x + 1) 2^k) x
//                       [y 2^k, (y + 1) 2^k) alone, all of them inside the image (x < (w >> k) means (x + 1) 2^k <= w), so a
//                       tile needs nothing of its neighbours, no clamp ever applies and what the out-of-image lanes of a partial
//                       tile hold never reaches a stored texel: their loads are moved to a valid address, their stores guarded.
//   mip_level_kernel    one level of any size, with the clamps: the levels after one extent has reached 1, and every level
//                       under KC_MIP_PER_LEVEL.
// Both take all distinct resident planes of the image in one launch (the plane is a grid index, pointers and pitches a table in
// the argument block).  f32 addition commutes bit for bit (NaN payloads are not part of the contract), which is what lets the
// cross-lane steps use symmetric exchanges.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // ld_policy / st_policy

typedef float mip_f4 __attribute__((ext_vector_type(4)));
typedef float mip_f2 __attribute__((ext_vector_type(2)));

static __device__ __forceinline__ float mip_box(float a, float b, float c, float d) { return ((a + b) + (c + d)) * 0.25f; }

// Thread (tx, ty) of the 16 x 16 workgroup holds rows 4 ty .. 4 ty + 3, columns 4 tx .. 4 tx + 3 of the tile: four 16-byte loads
// issued up front.  Levels 1 and 2 are in-lane (a 2 x 2 patch, then one value); a wave holds four ty rows, so levels 3 and 4
// are exchanges between its lanes (tx ^ 1, ty ^ 1, then tx ^ 2, ty ^ 2: lanes ^ 1, ^ 16, ^ 2, ^ 32); level 5 pairs the waves and
// level 6 is the whole tile: the 4 x 4 level-4 values go through LDS and one barrier.  n (1..6) levels are stored.
template <bool NT>  // NT: the source does not fit the cache budget: its loads and the level-1 stores are nontemporal
__global__ __launch_bounds__(256) void mip_pyramid_kernel(const MipPyramidArgs a)
{
#ifndef KC_MIP_LDS_TILE
    __shared__ float l4[16];
#endif
    const uint32_t t = threadIdx.x, tx = t & 15u, ty = t >> 4, pl = blockIdx.z;
    const uint32_t w = a.w, h = a.h, n = a.n;
    const float *src = a.src[pl];
    const uint32_t sp = a.src_pitch[pl];
    // rows are readable in whole float4 quads up to 4 ceil(w / 4) floats and no further (kc_plane_wrap)
    const uint32_t q = min(blockIdx.x * 16u + tx, (w + 3u) / 4u - 1u);
    mip_f4 p[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t r = min(blockIdx.y * 64u + 4u * ty + (uint32_t)i, h - 1u);
        p[i] = ld_policy<NT>(reinterpret_cast<const mip_f4 *>(src + (size_t)r * sp + 4u * q));
    }
    float v1[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        v1[r][0] = mip_box(p[2 * r][0], p[2 * r][1], p[2 * r + 1][0], p[2 * r + 1][1]);
        v1[r][1] = mip_box(p[2 * r][2], p[2 * r][3], p[2 * r + 1][2], p[2 * r + 1][3]);
    }
    {
        float *d = a.dst[pl][0];
        const uint32_t W = w >> 1, H = h >> 1, x = blockIdx.x * 32u + 2u * tx;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint32_t y = blockIdx.y * 32u + 2u * ty + (uint32_t)r;
            float *o = d + (size_t)y * a.dst_pitch[0] + x;
            if (y < H && x + 1u < W) st_policy<NT>(reinterpret_cast<mip_f2 *>(o), mip_f2{ v1[r][0], v1[r][1] });
            else if (y < H && x < W) *o = v1[r][0];
        }
    }
    // every lane goes on, in range or not: the exchanges below need all 64 lanes of a wave
    const float v2 = mip_box(v1[0][0], v1[0][1], v1[1][0], v1[1][1]);
    if (n >= 2u) {
        const uint32_t x = blockIdx.x * 16u + tx, y = blockIdx.y * 16u + ty;
        if (x < (w >> 2) && y < (h >> 2)) a.dst[pl][1][(size_t)y * a.dst_pitch[1] + x] = v2;
    }
#ifdef KC_MIP_LDS_TILE
    // The other form of levels 3 to 6 (tuning builds, tools/build_variant.sh; the same bits, profiles/mip_times.txt has both
    // times): the 16 x 16 level-2 tile goes through LDS and the first wave finishes alone, lane (x, y) of 8 x 8 at level 3.
    __shared__ float l2[16 * 17];
    if (n < 3u) return;
    l2[ty * 17u + tx] = v2;
    __syncthreads();
    if (t >= 64u) return;
    {
        const uint32_t lx = t & 7u, ly = t >> 3;
        const float *s = l2 + (2u * ly) * 17u + 2u * lx;
        float v = mip_box(s[0], s[1], s[17], s[18]);
        uint32_t x = blockIdx.x * 8u + lx, y = blockIdx.y * 8u + ly;
        if (x < (w >> 3) && y < (h >> 3)) a.dst[pl][2][(size_t)y * a.dst_pitch[2] + x] = v;
#pragma unroll
        for (uint32_t k = 4u; k <= 6u; ++k) {  // level k: lanes ^ (1, 8), ^ (2, 16), ^ (4, 32)
            const uint32_t m = 1u << (k - 4u);
            const float hsum = v + __shfl_xor(v, (int)m, 64);
            v = (hsum + __shfl_xor(hsum, (int)(8u * m), 64)) * 0.25f;
            x = blockIdx.x * (64u >> k) + (lx >> (k - 3u));
            y = blockIdx.y * (64u >> k) + (ly >> (k - 3u));
            const uint32_t low = 2u * m - 1u;
            if (n >= k && !(lx & low) && !(ly & low) && x < (w >> k) && y < (h >> k)) a.dst[pl][k - 1u][(size_t)y * a.dst_pitch[k - 1u] + x] = v;
        }
    }
#else
    float hs = v2 + __shfl_xor(v2, 1, 64);
    const float v3 = (hs + __shfl_xor(hs, 16, 64)) * 0.25f;
    if (n >= 3u && !(tx & 1u) && !(ty & 1u)) {
        const uint32_t x = blockIdx.x * 8u + (tx >> 1), y = blockIdx.y * 8u + (ty >> 1);
        if (x < (w >> 3) && y < (h >> 3)) a.dst[pl][2][(size_t)y * a.dst_pitch[2] + x] = v3;
    }
    hs = v3 + __shfl_xor(v3, 2, 64);
    const float v4 = (hs + __shfl_xor(hs, 32, 64)) * 0.25f;
    if (n >= 4u && !(tx & 3u) && !(ty & 3u)) {
        const uint32_t x = blockIdx.x * 4u + (tx >> 2), y = blockIdx.y * 4u + (ty >> 2);
        if (x < (w >> 4) && y < (h >> 4)) a.dst[pl][3][(size_t)y * a.dst_pitch[3] + x] = v4;
    }
    if (n < 5u) return;  // uniform over the launch: no workgroup meets the barrier
    if (!(tx & 3u) && !(ty & 3u)) l4[(ty >> 2) * 4u + (tx >> 2)] = v4;
    __syncthreads();
    if (t < 4u) {
        const uint32_t cx = t & 1u, cy = t >> 1;
        const float *s = l4 + 8u * cy + 2u * cx;
        const float v5 = mip_box(s[0], s[1], s[4], s[5]);
        const uint32_t x = blockIdx.x * 2u + cx, y = blockIdx.y * 2u + cy;
        if (x < (w >> 5) && y < (h >> 5)) a.dst[pl][4][(size_t)y * a.dst_pitch[4] + x] = v5;
    }
    if (t == 0u && n >= 6u && blockIdx.x < (w >> 6) && blockIdx.y < (h >> 6)) {
        float v5[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float *s = l4 + 8 * (k >> 1) + 2 * (k & 1);
            v5[k] = mip_box(s[0], s[1], s[4], s[5]);
        }
        a.dst[pl][5][(size_t)blockIdx.y * a.dst_pitch[5] + blockIdx.x] = mip_box(v5[0], v5[1], v5[2], v5[3]);
    }
#endif
}

// One thread per quad of output texels, rows in order.  A whole quad (4 q + 3 < W, hence source columns up to 8 q + 7 <= w - 1)
// is two 16-byte loads per source row and one 16-byte store; the tail of a row is scalar, with the column clamp.
template <bool NT>
__global__ __launch_bounds__(256) void mip_level_kernel(const MipLevelArgs a)
{
    const uint32_t W = max(a.w >> 1, 1u), H = max(a.h >> 1, 1u), quads = (W + 3u) / 4u;
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= quads * H) return;
    const uint32_t y = idx / quads, q = idx - y * quads, pl = blockIdx.y;
    const float *r0 = a.src[pl] + (size_t)(2u * y) * a.src_pitch[pl];
    const float *r1 = a.src[pl] + (size_t)min(2u * y + 1u, a.h - 1u) * a.src_pitch[pl];
    float *o = a.dst[pl] + (size_t)y * a.dst_pitch + 4u * q;
    if (4u * q + 3u < W) {
        const mip_f4 t0 = ld_policy<NT>(reinterpret_cast<const mip_f4 *>(r0 + 8u * q));
        const mip_f4 t1 = ld_policy<NT>(reinterpret_cast<const mip_f4 *>(r0 + 8u * q + 4u));
        const mip_f4 b0 = ld_policy<NT>(reinterpret_cast<const mip_f4 *>(r1 + 8u * q));
        const mip_f4 b1 = ld_policy<NT>(reinterpret_cast<const mip_f4 *>(r1 + 8u * q + 4u));
        const mip_f4 d = { mip_box(t0[0], t0[1], b0[0], b0[1]), mip_box(t0[2], t0[3], b0[2], b0[3]),
                           mip_box(t1[0], t1[1], b1[0], b1[1]), mip_box(t1[2], t1[3], b1[2], b1[3]) };
        st_policy<NT>(reinterpret_cast<mip_f4 *>(o), d);
        return;
    }
    for (uint32_t x = 4u * q; x < W; ++x) {
        const uint32_t x0 = 2u * x, x1 = min(2u * x + 1u, a.w - 1u);
        o[x - 4u * q] = mip_box(r0[x0], r0[x1], r1[x0], r1[x1]);
    }
}

hipError_t launch_mip_pyramid(const MipPyramidArgs &a, uint32_t n_planes, bool nt, hipStream_t s)
{
    if (a.w < 2 || a.h < 2 || a.n < 1 || a.n > 6 || n_planes < 1 || n_planes > 4) return hipErrorInvalidValue;
    if ((a.w >> a.n) == 0 || (a.h >> a.n) == 0) return hipErrorInvalidValue;  // both extents halve n times
    const uint64_t gx = ((uint64_t)a.w + 63) / 64, gy = ((uint64_t)a.h + 63) / 64;
    if (gx > 0x7fffffffull || gy > 65535ull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)gx, (unsigned)gy, n_planes);
    if (nt) mip_pyramid_kernel<true><<<grid, 256, 0, s>>>(a);
    else mip_pyramid_kernel<false><<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mip_level(const MipLevelArgs &a, uint32_t n_planes, bool nt, hipStream_t s)
{
    if (a.w == 0 || a.h == 0 || (a.w == 1 && a.h == 1) || n_planes < 1 || n_planes > 4) return hipErrorInvalidValue;
    const uint64_t W = a.w > 1 ? a.w >> 1 : 1, H = a.h > 1 ? a.h >> 1 : 1;
    const uint64_t total = (W + 3) / 4 * H;
    if (total > (1ull << 31)) return hipErrorInvalidValue;  // the kernel's quad index is 32-bit
    const dim3 grid((unsigned)((total + 255) / 256), n_planes);
    if (nt) mip_level_kernel<true><<<grid, 256, 0, s>>>(a);
    else mip_level_kernel<false><<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace kc
