// Block compression (kc_image_to_bc / kc_image_to_bc_device, bc.cpp): the image as kc_image_to_u8 writes it -> BC1, BC3, BC4 or
// BC5 blocks, by the integer rules of include/kanter_core_amd.h (tests/bc_ref.py is the same rules in numpy).  An HBM-bound
// stream in the form of to_u8_kernel: one thread per 4x4 block, a grid-stride loop over the blocks in row order, so the lanes of
// a wave take consecutive blocks of a block row and each of the block's four pixel rows is one 16-byte load per plane and lane,
// contiguous across the wave (the library's planes, kc_plane_wrap's included, are readable in whole float4 quads).  The texels
// are quantised as they arrive and kept as RGBA8 words; the encoder is integer arithmetic on them; a block leaves in one 8- or
// 16-byte store.  The steps of the stream -- the walk over the blocks and its edge rule, the row loads, the quantiser, the staging of
// the sRGB table -- are bc_blocks.h's; bc7.hip and bc6h.hip run the same loop around their own encoders.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // grid_cap, ld_policy, quant_u8 / quant_u8_srgb: shared with u8.hip
#include "bc_blocks.h"  // BcBlockArgs, the grid, the block walk, the row loaders and the quantiser: shared by the block-compression units

// The channels a format reads: bit c = channel c (R, G, B, A)
static constexpr uint32_t bc_channels(int fmt) { return fmt == 1 ? 0x7u : fmt == 3 ? 0xfu : fmt == 4 ? 0x1u : 0x3u; }

// BC4 of the 16-bit lane at bit `sh` (0 or 16) of the 16 texel words: e0 = max, e1 = min; ramp r = floor((14 (v - e1) + d) / 2d)
// by the exact reciprocal m = ceil(2^21 / 2d) (x = 14 (v - e1) + d < 3826 and the rounding error of m below 2d keep x m >> 21
// exact, and x m < 2^32 in a 24-bit multiply); index = 1, 7, 6, 5, 4, 3, 2, 0 for r = 0..7.
static __device__ __forceinline__ bc_u2 encode_bc4(const uint32_t (&wd)[16], uint32_t sh)
{
    uint32_t e0 = 0u, e1 = 255u;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const uint32_t v = __builtin_amdgcn_ubfe(wd[t], sh, 16u);
        e0 = max(e0, v);
        e1 = min(e1, v);
    }
    const uint32_t d = e0 - e1;
    uint32_t lo = e0 | (e1 << 8), hi = 0u;  // bytes 0..3 and 4..7 of the block
    if (d != 0u) {
        const uint32_t m = (0x200000u + 2u * d - 1u) / (2u * d);
        constexpr uint32_t kIndex = 1u | 7u << 3 | 6u << 6 | 5u << 9 | 4u << 12 | 3u << 15 | 2u << 18;  // r = 7: 0
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const uint32_t v = __builtin_amdgcn_ubfe(wd[t], sh, 16u);
            const uint32_t x = __umul24(14u, v - e1) + d;
            const uint32_t r = __umul24(x, m) >> 21;
            const uint32_t idx = __builtin_amdgcn_ubfe(kIndex, 3u * r, 3u);
            // the 48 index bits start at bit 16 of the block
            const int b = 16 + 3 * t;
            if (b + 3 <= 32) lo |= idx << b;
            else if (b >= 32) hi |= idx << (b - 32);
            else {
                lo |= idx << b;
                hi |= idx >> (32 - b);
            }
        }
    }
    return bc_u2{ lo, hi };
}

// encode_bc1: bc_blocks.h's, which bc1a.hip shares
template <int FMT>
static __device__ __forceinline__ void bc_encode_store(const uint32_t (&rb)[16], const uint32_t (&ga)[16], const BcBlockArgs &a, uint32_t i,
                                                       uint32_t j)
{
    char *p = a.dst + (size_t)j * a.row_pitch;
    if constexpr (FMT == 1) {
        *reinterpret_cast<bc_u2 *>(p + (size_t)i * 8) = encode_bc1(rb, ga);
    } else if constexpr (FMT == 4) {
        *reinterpret_cast<bc_u2 *>(p + (size_t)i * 8) = encode_bc4(rb, 0u);
    } else {
        const bc_u2 x = FMT == 3 ? encode_bc4(ga, 16u) : encode_bc4(rb, 0u);
        const bc_u2 y = FMT == 3 ? encode_bc1(rb, ga) : encode_bc4(ga, 0u);
        *reinterpret_cast<bc_u4 *>(p + (size_t)i * 16) = bc_u4{ x.x, x.y, y.x, y.y };
    }
}

template <int FMT, bool SRGB, bool NT>  // NT: the planes are read once and do not fit the Infinity Cache (cache_policy_mask)
__global__ __launch_bounds__(256) void bc_encode_kernel(Operand r, Operand g, Operand b, Operand al, int gray, const BcBlockArgs a)
{
    __shared__ uint32_t srgb_t[SRGB ? 257 : 1];
    constexpr uint32_t CH = bc_channels(FMT);
    const Operand op[4] = { r, g, b, al };
    const BcWalk k = bc_walk(a.w, a.h, a.bx, a.by);
    uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if constexpr (SRGB) {
        // The first block's first row of loads goes out BEFORE the threshold table is staged (a global read and a barrier that
        // every thread of the workgroup takes, in range or not), as in to_u8_kernel: the table arrives while they are in flight.
        const bool in_range = idx < k.total;
        uint32_t i, j;
        const bool we = bc_block_of(k, idx, i, j);
        bc_f4 v[4];
        if (in_range) bc_load_row<CH, NT>(op, gray, a, i, j, 0, we, v);
        bc_stage_srgb(srgb_t);
        if (!in_range) return;
        uint32_t rb[16], ga[16];
        bc_quantise_row<CH, SRGB>(v, gray, 0, srgb_t, rb, ga);
#pragma unroll
        for (int y = 1; y < 4; ++y) {
            bc_load_row<CH, NT>(op, gray, a, i, j, y, we, v);
            bc_quantise_row<CH, SRGB>(v, gray, y, srgb_t, rb, ga);
        }
        if (we) bc_clamp_columns(a, i, rb, ga);
        bc_encode_store<FMT>(rb, ga, a, i, j);
        idx += gridDim.x * 256u;
    }
    for (; idx < k.total; idx += gridDim.x * 256u) {
        uint32_t i, j;
        const bool we = bc_block_of(k, idx, i, j);
        uint32_t rb[16], ga[16];
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            bc_f4 v[4];
            bc_load_row<CH, NT>(op, gray, a, i, j, y, we, v);
            bc_quantise_row<CH, SRGB>(v, gray, y, srgb_t, rb, ga);
        }
        if (we) bc_clamp_columns(a, i, rb, ga);
        bc_encode_store<FMT>(rb, ga, a, i, j);
    }
}

hipError_t launch_bc_encode(int fmt, int srgb, const Operand op[4], int gray, char *dst, uint64_t row_pitch, uint32_t w, uint32_t h,
                            uint32_t nt_mask, hipStream_t s)
{
    const BcBlockArgs a = bc_block_args(dst, row_pitch, w, h);
    const uint64_t total = (uint64_t)a.bx * a.by;
    if (total == 0) return hipSuccess;
    const uint32_t blocks = bc_grid(total, 1u << 30);
    const bool nt = (nt_mask & 0xffu) != 0;
    if (srgb && fmt != KC_BC1 && fmt != KC_BC3) return hipErrorInvalidValue;  // no such instantiation (BC7: bc7.hip)
#define KC_BC(F, SR, NTL) bc_encode_kernel<F, SR, NTL><<<dim3(blocks), 256, 0, s>>>(op[0], op[1], op[2], op[3], gray, a)
#define KC_BC_NT(F, SR)                                                                                                               \
    do {                                                                                                                             \
        if (nt) KC_BC(F, SR, true);                                                                                                  \
        else KC_BC(F, SR, false);                                                                                                    \
    } while (0)
    switch (fmt) {
    case KC_BC1:
        if (srgb) KC_BC_NT(KC_BC1, true);
        else KC_BC_NT(KC_BC1, false);
        break;
    case KC_BC3:
        if (srgb) KC_BC_NT(KC_BC3, true);
        else KC_BC_NT(KC_BC3, false);
        break;
    case KC_BC4: KC_BC_NT(KC_BC4, false); break;
    case KC_BC5: KC_BC_NT(KC_BC5, false); break;
    default: return hipErrorInvalidValue;
    }
#undef KC_BC_NT
#undef KC_BC
    return hipGetLastError();
}

}  // namespace kc
