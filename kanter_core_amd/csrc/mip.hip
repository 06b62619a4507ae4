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
// cross-lane steps use symmetric exchanges.  The steps themselves -- the box, the tile's loads, reduction and stores, the
// one-level step, the launch checks -- are mip_steps.h's, the one copy that mip_normals.hip and preview.hip run too; the kernels
// here are those steps on one plane with the plain rule.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // ld_policy / st_policy
#include "mip_steps.h"  // the box, the tile steps, the one-level step, the launch checks

// mip_steps.h's tile walk on one plane with the plain rule: every level up to n (1..6) is stored.
template <bool NT>  // NT: the source does not fit the cache budget: its loads and the level-1 stores are nontemporal
__global__ __launch_bounds__(256) void mip_pyramid_kernel(const MipPyramidArgs a)
{
    __shared__ float l4[1][16];
    const uint32_t t = threadIdx.x, tx = t & 15u, ty = t >> 4, pl = blockIdx.z;
    const uint32_t w = a.w, h = a.h, n = a.n;
    MipRows p[1];
    mip_tile_load<NT>(a.src[pl], a.src_pitch[pl], w, h, tx, ty, p[0]);
    auto done = [&](uint32_t k, const float (&v)[1][4]) __attribute__((always_inline)) {
        mip_tile_store<NT>(k, v, n, w, h, tx, ty, [&](int, uint32_t j) __attribute__((always_inline)) { return a.dst[pl][j - 1u]; }, a.dst_pitch);
        return k == 4u && n < 5u;  // levels 2 to 4 are made whatever n is: no branch between the exchanges
    };
    mip_tile_reduce(p, tx, ty, l4, MipPlainRule(), done);
    if (n < 5u) return;  // uniform over the launch: no workgroup meets the barrier
    __syncthreads();
    mip_tile_tail<1>(l4, true, n >= 6u, t, MipPlainRule(), done);
}

// mip_steps.h's one-level step on one plane with the plain rule.
template <bool NT>
__global__ __launch_bounds__(256) void mip_level_kernel(const MipLevelArgs a)
{
    const uint32_t pl = blockIdx.y;
    mip_level_step<NT, 1>(a.src + pl, a.src_pitch + pl, a.w, a.h, a.dst + pl, a.dst_pitch, MipPlainRule(), MipOwnPlanes());
}

hipError_t launch_mip_pyramid(const MipPyramidArgs &a, uint32_t n_planes, bool nt, hipStream_t s)
{
    dim3 grid;
    if (!mip_pyramid_grid(a.w, a.h, a.n, n_planes, &grid)) return hipErrorInvalidValue;
    if (nt) mip_pyramid_kernel<true><<<grid, 256, 0, s>>>(a);
    else mip_pyramid_kernel<false><<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mip_level(const MipLevelArgs &a, uint32_t n_planes, bool nt, hipStream_t s)
{
    dim3 grid;
    if (!mip_level_grid(a.w, a.h, n_planes, &grid)) return hipErrorInvalidValue;
    if (nt) mip_level_kernel<true><<<grid, 256, 0, s>>>(a);
    else mip_level_kernel<false><<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace kc
