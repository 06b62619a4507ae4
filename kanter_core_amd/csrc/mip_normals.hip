// Mip chains of normal maps (KC_MIP_NORMALS; kc_image_build_mips, mip.cpp): mip.hip's two walks with R, G, B coupled in one
// thread.  A texel of level k is the 2 x 2 box of each channel (mip.hip's expression and clamps), then, on the three boxes b,
//     v = b * 2.0f - 1.0f,   l = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z),   u = l > 0 && l < inf ? v / l : (0, 0, 1),   d = u * 0.5f + 0.5f
// -- every level normalised and rounded to f32 before the next is made, so the fused kernel and the level-by-level one give the
// same bits (tests/mip_normals_ref.py is the same rule in numpy).  The comparison is false for NaN: a zero vector, an
// underflowed or overflowed sum and a NaN or infinity in any channel all store (0.5, 0.5, 1.0), and no level >= 1 holds a NaN.
//   normal_pyramid_kernel  mip_pyramid_kernel's tile walk: one workgroup per 64 x 64 source tile, up to six levels.  In the
//                          cross-lane steps every lane of an exchange group holds bit-equal sums (f32 addition commutes) and
//                          normalises its own copy, so the groups stay bit-equal all the way down.
//   normal_level_kernel    mip_level_kernel's: one level of any size, with the clamps.
// A channel is a resident plane, a constant (a value and a bit in the argument block: its loads are that value, its pointer is
// never formed) or the loads of an earlier channel that aliases it; all three are uniform over the launch, and three planes of
// their own -- every level >= 1, every HeightToNormal result -- take a path without those branches.  sqrtf and / are
// the build's correctly rounded ones (-fhip-fp32-correctly-rounded-divide-sqrt), nothing is contracted (-ffp-contract=off).
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // ld_policy / st_policy

typedef float nrm_f4 __attribute__((ext_vector_type(4)));
typedef float nrm_f2 __attribute__((ext_vector_type(2)));

static __device__ __forceinline__ float nrm_box(float a, float b, float c, float d) { return ((a + b) + (c + d)) * 0.25f; }

// b: the boxes of R, G, B in, the stored texel out
static __device__ __forceinline__ void normal_texel(float b[3])
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

static constexpr uint32_t kNormalOwnPlanes = 0u | 1u << 2 | 2u << 4;  // `from` when every channel reads its own plane

static __device__ __forceinline__ nrm_f4 nrm_splat(float v) { return nrm_f4{ v, v, v, v }; }

// mip_pyramid_kernel's thread layout (mip.hip): thread (tx, ty) of 16 x 16 holds rows 4 ty .. 4 ty + 3, columns 4 tx .. 4 tx + 3
// of the tile, of each of R, G, B: twelve 16-byte loads issued up front.  Levels 1 and 2 are in-lane, 3 and 4 exchanges between
// the lanes of a wave (^ 1, ^ 16, then ^ 2, ^ 32), 5 and 6 go through LDS and one barrier.  n (1..6) levels are stored.
template <bool NT>  // NT: the source does not fit the cache budget: its loads and the level-1 stores are nontemporal
__global__ __launch_bounds__(256) void normal_pyramid_kernel(const NormalPyramidArgs a)
{
    __shared__ float l4[3][16];
    const uint32_t t = threadIdx.x, tx = t & 15u, ty = t >> 4;
    const uint32_t w = a.w, h = a.h, n = a.n;
    // rows are readable in whole float4 quads up to 4 ceil(w / 4) floats and no further (kc_plane_wrap)
    const uint32_t q = min(blockIdx.x * 16u + tx, (w + 3u) / 4u - 1u);
    nrm_f4 p[3][4];
    auto load = [&](int c, nrm_f4 o[4]) {
        const float *src = a.src[c];
        const uint32_t sp = a.src_pitch[c];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t r = min(blockIdx.y * 64u + 4u * ty + (uint32_t)i, h - 1u);
            o[i] = ld_policy<NT>(reinterpret_cast<const nrm_f4 *>(src + (size_t)r * sp + 4u * q));
        }
    };
    if (a.const_mask == 0u && a.from == kNormalOwnPlanes) {  // three planes, the usual case: twelve loads and nothing between them
#pragma unroll
        for (int c = 0; c < 3; ++c) load(c, p[c]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t from = (a.from >> (2 * c)) & 3u;
            if ((a.const_mask >> c) & 1u) {
#pragma unroll
                for (int i = 0; i < 4; ++i) p[c][i] = nrm_splat(a.cval[c]);
            } else if (c >= 1 && from == 0u) {
#pragma unroll
                for (int i = 0; i < 4; ++i) p[c][i] = p[0][i];
            } else if (c == 2 && from == 1u) {
#pragma unroll
                for (int i = 0; i < 4; ++i) p[c][i] = p[1][i];
            } else {
                load(c, p[c]);
            }
        }
    }
    float v1[3][2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float b[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) b[c] = nrm_box(p[c][2 * r][2 * j], p[c][2 * r][2 * j + 1], p[c][2 * r + 1][2 * j], p[c][2 * r + 1][2 * j + 1]);
            normal_texel(b);
#pragma unroll
            for (int c = 0; c < 3; ++c) v1[c][r][j] = b[c];
        }
    {
        const uint32_t W = w >> 1, H = h >> 1, x = blockIdx.x * 32u + 2u * tx;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float *d = a.dst[c][0];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const uint32_t y = blockIdx.y * 32u + 2u * ty + (uint32_t)r;
                float *o = d + (size_t)y * a.dst_pitch[0] + x;
                if (y < H && x + 1u < W) st_policy<NT>(reinterpret_cast<nrm_f2 *>(o), nrm_f2{ v1[c][r][0], v1[c][r][1] });
                else if (y < H && x < W) *o = v1[c][r][0];
            }
        }
    }
    // every lane goes on, in range or not: the exchanges below need all 64 lanes of a wave
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = nrm_box(v1[c][0][0], v1[c][0][1], v1[c][1][0], v1[c][1][1]);
    normal_texel(v);
    if (n >= 2u) {
        const uint32_t x = blockIdx.x * 16u + tx, y = blockIdx.y * 16u + ty;
        if (x < (w >> 2) && y < (h >> 2)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a.dst[c][1][(size_t)y * a.dst_pitch[1] + x] = v[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float hs = v[c] + __shfl_xor(v[c], 1, 64);
        v[c] = (hs + __shfl_xor(hs, 16, 64)) * 0.25f;
    }
    normal_texel(v);  // the four lanes of a group hold the same three sums, hence the same texel
    if (n >= 3u && !(tx & 1u) && !(ty & 1u)) {
        const uint32_t x = blockIdx.x * 8u + (tx >> 1), y = blockIdx.y * 8u + (ty >> 1);
        if (x < (w >> 3) && y < (h >> 3)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a.dst[c][2][(size_t)y * a.dst_pitch[2] + x] = v[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float hs = v[c] + __shfl_xor(v[c], 2, 64);
        v[c] = (hs + __shfl_xor(hs, 32, 64)) * 0.25f;
    }
    normal_texel(v);
    if (n >= 4u && !(tx & 3u) && !(ty & 3u)) {
        const uint32_t x = blockIdx.x * 4u + (tx >> 2), y = blockIdx.y * 4u + (ty >> 2);
        if (x < (w >> 4) && y < (h >> 4)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a.dst[c][3][(size_t)y * a.dst_pitch[3] + x] = v[c];
        }
    }
    if (n < 5u) return;  // uniform over the launch: no workgroup meets the barrier
    if (!(tx & 3u) && !(ty & 3u)) {
#pragma unroll
        for (int c = 0; c < 3; ++c) l4[c][(ty >> 2) * 4u + (tx >> 2)] = v[c];
    }
    __syncthreads();
    // texel (cx, cy) of the tile's 2 x 2 level 5, from the 4 x 4 level-4 values
    auto level5 = [&](uint32_t cx, uint32_t cy, float o[3]) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float *s = l4[c] + 8u * cy + 2u * cx;
            o[c] = nrm_box(s[0], s[1], s[4], s[5]);
        }
        normal_texel(o);
    };
    if (t < 4u) {
        const uint32_t cx = t & 1u, cy = t >> 1;
        float v5[3];
        level5(cx, cy, v5);
        const uint32_t x = blockIdx.x * 2u + cx, y = blockIdx.y * 2u + cy;
        if (x < (w >> 5) && y < (h >> 5)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a.dst[c][4][(size_t)y * a.dst_pitch[4] + x] = v5[c];
        }
    }
    if (t == 0u && n >= 6u && blockIdx.x < (w >> 6) && blockIdx.y < (h >> 6)) {
        float v5[4][3], v6[3];
#pragma unroll
        for (int k = 0; k < 4; ++k) level5((uint32_t)(k & 1), (uint32_t)(k >> 1), v5[k]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v6[c] = nrm_box(v5[0][c], v5[1][c], v5[2][c], v5[3][c]);
        normal_texel(v6);
#pragma unroll
        for (int c = 0; c < 3; ++c) a.dst[c][5][(size_t)blockIdx.y * a.dst_pitch[5] + blockIdx.x] = v6[c];
    }
}

// One thread per quad of output texels, rows in order, as mip_level_kernel: a whole quad (4 q + 3 < W, hence source columns up
// to 8 q + 7 <= w - 1) is two 16-byte loads per source row and channel and one 16-byte store per channel; the tail of a row is
// scalar, with the column clamp.
template <bool NT>
__global__ __launch_bounds__(256) void normal_level_kernel(const NormalLevelArgs a)
{
    const uint32_t W = max(a.w >> 1, 1u), H = max(a.h >> 1, 1u), quads = (W + 3u) / 4u;
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= quads * H) return;
    const uint32_t y = idx / quads, q = idx - y * quads;
    const uint32_t y0 = 2u * y, y1 = min(2u * y + 1u, a.h - 1u);
    const size_t o = (size_t)y * a.dst_pitch + 4u * q;
    if (4u * q + 3u < W) {
        nrm_f4 b[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t from = (a.from >> (2 * c)) & 3u;
            if ((a.const_mask >> c) & 1u) {
                b[c] = nrm_splat(nrm_box(a.cval[c], a.cval[c], a.cval[c], a.cval[c]));
            } else if (c >= 1 && from == 0u) {
                b[c] = b[0];
            } else if (c == 2 && from == 1u) {
                b[c] = b[1];
            } else {
                const float *r0 = a.src[c] + (size_t)y0 * a.src_pitch[c], *r1 = a.src[c] + (size_t)y1 * a.src_pitch[c];
                const nrm_f4 t0 = ld_policy<NT>(reinterpret_cast<const nrm_f4 *>(r0 + 8u * q));
                const nrm_f4 t1 = ld_policy<NT>(reinterpret_cast<const nrm_f4 *>(r0 + 8u * q + 4u));
                const nrm_f4 b0 = ld_policy<NT>(reinterpret_cast<const nrm_f4 *>(r1 + 8u * q));
                const nrm_f4 b1 = ld_policy<NT>(reinterpret_cast<const nrm_f4 *>(r1 + 8u * q + 4u));
                b[c] = nrm_f4{ nrm_box(t0[0], t0[1], b0[0], b0[1]), nrm_box(t0[2], t0[3], b0[2], b0[3]),
                               nrm_box(t1[0], t1[1], b1[0], b1[1]), nrm_box(t1[2], t1[3], b1[2], b1[3]) };
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v[3] = { b[0][j], b[1][j], b[2][j] };
            normal_texel(v);
            b[0][j] = v[0];
            b[1][j] = v[1];
            b[2][j] = v[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) st_policy<NT>(reinterpret_cast<nrm_f4 *>(a.dst[c] + o), b[c]);
        return;
    }
    for (uint32_t x = 4u * q; x < W; ++x) {
        const uint32_t x0 = 2u * x, x1 = min(2u * x + 1u, a.w - 1u);
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t from = (a.from >> (2 * c)) & 3u;
            if ((a.const_mask >> c) & 1u) {
                v[c] = nrm_box(a.cval[c], a.cval[c], a.cval[c], a.cval[c]);
            } else if (c >= 1 && from == 0u) {
                v[c] = v[0];
            } else if (c == 2 && from == 1u) {
                v[c] = v[1];
            } else {
                const float *r0 = a.src[c] + (size_t)y0 * a.src_pitch[c], *r1 = a.src[c] + (size_t)y1 * a.src_pitch[c];
                v[c] = nrm_box(r0[x0], r0[x1], r1[x0], r1[x1]);
            }
        }
        normal_texel(v);
#pragma unroll
        for (int c = 0; c < 3; ++c) a.dst[c][o + (x - 4u * q)] = v[c];
    }
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
    if (a.w < 2 || a.h < 2 || a.n < 1 || a.n > 6 || !normal_channels_ok(a.src, a.const_mask, a.from)) return hipErrorInvalidValue;
    if ((a.w >> a.n) == 0 || (a.h >> a.n) == 0) return hipErrorInvalidValue;  // both extents halve n times
    const uint64_t gx = ((uint64_t)a.w + 63) / 64, gy = ((uint64_t)a.h + 63) / 64;
    if (gx > 0x7fffffffull || gy > 65535ull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)gx, (unsigned)gy);
    if (nt) normal_pyramid_kernel<true><<<grid, 256, 0, s>>>(a);
    else normal_pyramid_kernel<false><<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_normal_level(const NormalLevelArgs &a, bool nt, hipStream_t s)
{
    if (a.w == 0 || a.h == 0 || (a.w == 1 && a.h == 1) || !normal_channels_ok(a.src, a.const_mask, a.from)) return hipErrorInvalidValue;
    const uint64_t W = a.w > 1 ? a.w >> 1 : 1, H = a.h > 1 ? a.h >> 1 : 1;
    const uint64_t total = (W + 3) / 4 * H;
    if (total > (1ull << 31)) return hipErrorInvalidValue;  // the kernel's quad index is 32-bit
    const dim3 grid((unsigned)((total + 255) / 256));
    if (nt) normal_level_kernel<true><<<grid, 256, 0, s>>>(a);
    else normal_level_kernel<false><<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace kc
