// BC1 with punch-through alpha (KC_BC_PUNCH_THROUGH; bc.cpp, bc_decode.cpp): the image as kc_image_to_u8 writes it -> BC1 blocks
// whose texels below the reference byte decode transparent, by the integer rule of include/kanter_core_amd.h
// (tests/bc1a_ref.py is the same rule in numpy), and the error of such an encoding.  Both kernels are bc.hip's and
// bc_decode.hip's streams over bc_blocks.h's steps with all four planes read: one thread per 4x4 block, a grid-stride loop over
// the blocks in row order, a block's four pixel rows one 16-byte load per plane and lane, a block out in one 8-byte store.
// A wave holds all three block classes at once -- 16, 1..15 and no opaque texels -- so the endpoints are ONE masked pass
// (bc_blocks.h's bc1_endpoints<true>: masked min / max and dot products, then the inset and the order by class); only the index
// word has two forms, the four-colour thresholds of plain BC1 and the three distances of the three-colour palette, and a wave
// of one class runs one of them.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // grid_cap, ld_policy, quant_u8 / quant_u8_srgb
#include "bc_blocks.h"  // the block walk, the row loaders, the quantiser, BC1's block and the record fold

// The index word of the three-colour block (c0 <= c1): Q0 = E(c0), Q1 = E(c1), Q2 = (E(c0) + E(c1)) div 2, which is not on
// the line of the other two after the division, so the three squared distances are computed: packed differences, dot products
// of them with themselves.  The lowest j wins a tie; a texel that is not opaque takes index 3.
static __device__ __forceinline__ uint32_t bc1_indices3(const uint32_t (&rb)[16], const uint32_t (&ga)[16], uint32_t opq, uint32_t c0,
                                                        uint32_t c1)
{
    const uint32_t r5 = c0 >> 11, g6 = (c0 >> 5) & 63u, b5 = c0 & 31u;
    const uint32_t s5 = c1 >> 11, h6 = (c1 >> 5) & 63u, c5 = c1 & 31u;
    const uint32_t E0[3] = { (r5 << 3) | (r5 >> 2), (g6 << 2) | (g6 >> 4), (b5 << 3) | (b5 >> 2) };
    const uint32_t E1[3] = { (s5 << 3) | (s5 >> 2), (h6 << 2) | (h6 >> 4), (c5 << 3) | (c5 >> 2) };
    const uint32_t qrb[3] = { E0[0] | (E0[2] << 16), E1[0] | (E1[2] << 16), ((E0[0] + E1[0]) >> 1) | (((E0[2] + E1[2]) >> 1) << 16) };
    const uint32_t qg[3] = { E0[1], E1[1], (E0[1] + E1[1]) >> 1 };
    uint32_t word = 0u;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const uint32_t g = ga[t] & 0xffffu;
        int32_t d[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t drb = pk_sub(rb[t], qrb[j]), dg = pk_sub(g, qg[j]);  // -255..255 per lane
            d[j] = dot2(dg, dg, dot2(drb, drb, 0));
        }
        uint32_t j = d[1] < d[0] ? 1u : 0u;
        j = d[2] < min(d[0], d[1]) ? 2u : j;
        j = ((opq >> t) & 1u) ? j : 3u;
        word |= j << (2 * t);
    }
    return word;
}

// The block of 16 texels under the reference byte `ref` (1..255); alpha is the high half of ga
static __device__ __forceinline__ bc_u2 encode_bc1a(const uint32_t (&rb)[16], const uint32_t (&ga)[16], uint32_t ref)
{
    uint32_t opq = 0u;
#pragma unroll
    for (int t = 0; t < 16; ++t) opq |= ((ga[t] >> 16) >= ref ? 1u : 0u) << t;
    const bool three = opq != 0xffffu;
    uint32_t c0, c1;
    bc1_endpoints<true>(rb, ga, opq, three, c0, c1);
    uint32_t word;
    if (three) word = bc1_indices3(rb, ga, opq, c0, c1);
    else word = bc1_indices4(rb, ga, c0, c1);
    if (opq == 0u) return bc_u2{ 0u, 0xffffffffu };  // c0 = c1 = 0, every index 3
    return bc_u2{ c0 | (c1 << 16), word };
}

template <bool SRGB, bool NT>  // NT: the planes are read once and do not fit the Infinity Cache (cache_policy_mask)
__global__ __launch_bounds__(256) void bc1a_encode_kernel(Operand r, Operand g, Operand b, Operand al, const BcBlockArgs a, uint32_t ref)
{
    __shared__ uint32_t srgb_t[SRGB ? 257 : 1];
    constexpr uint32_t CH = 0xfu;
    const Operand op[4] = { r, g, b, al };
    const BcWalk k = bc_walk(a.w, a.h, a.bx, a.by);
    uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if constexpr (SRGB) {
        // The first block's first row of loads goes out BEFORE the threshold table is staged, as in bc_encode_kernel
        const bool in_range = idx < k.total;
        uint32_t i, j;
        const bool we = bc_block_of(k, idx, i, j);
        bc_f4 v[4];
        if (in_range) bc_load_row<CH, NT>(op, 0, a, i, j, 0, we, v);
        bc_stage_srgb(srgb_t);
        if (!in_range) return;
        uint32_t rb[16], ga[16];
        bc_quantise_row<CH, SRGB>(v, 0, 0, srgb_t, rb, ga);
#pragma unroll
        for (int y = 1; y < 4; ++y) {
            bc_load_row<CH, NT>(op, 0, a, i, j, y, we, v);
            bc_quantise_row<CH, SRGB>(v, 0, y, srgb_t, rb, ga);
        }
        if (we) bc_clamp_columns(a, i, rb, ga);
        *reinterpret_cast<bc_u2 *>(a.dst + (size_t)j * a.row_pitch + (size_t)i * 8) = encode_bc1a(rb, ga, ref);
        idx += gridDim.x * 256u;
    }
    for (; idx < k.total; idx += gridDim.x * 256u) {
        uint32_t i, j;
        const bool we = bc_block_of(k, idx, i, j);
        uint32_t rb[16], ga[16];
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            bc_f4 v[4];
            bc_load_row<CH, NT>(op, 0, a, i, j, y, we, v);
            bc_quantise_row<CH, SRGB>(v, 0, y, srgb_t, rb, ga);
        }
        if (we) bc_clamp_columns(a, i, rb, ga);
        *reinterpret_cast<bc_u2 *>(a.dst + (size_t)j * a.row_pitch + (size_t)i * 8) = encode_bc1a(rb, ga, ref);
    }
}

// bc_compare_kernel's record (words 0-7) under the flag: the source alpha is 255 where the source texel is opaque and 0
// otherwise, and a texel that is not opaque contributes nothing to R, G and B
template <bool SRGB, bool NT>
__global__ __launch_bounds__(256) void bc1a_compare_kernel(Operand r, Operand g, Operand b, Operand al, const BcBlockArgs a, uint32_t ref,
                                                           unsigned long long *partials)
{
    __shared__ uint32_t srgb_t[SRGB ? 257 : 1];
    __shared__ unsigned long long red[4][KC_BC_REC_WORDS];  // per wave
    constexpr uint32_t CH = 0xfu;
    const Operand op[4] = { r, g, b, al };
    if constexpr (SRGB) bc_stage_srgb(srgb_t);
    const BcWalk k = bc_walk(a.w, a.h, a.bx, a.by);
    unsigned long long sse[4] = { 0ull, 0ull, 0ull, 0ull };
    uint32_t mx[4] = { 0u, 0u, 0u, 0u };
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < k.total; idx += gridDim.x * 256u) {
        uint32_t i, j;
        const bool wave_edge = bc_block_of(k, idx, i, j);
        uint32_t rb[16], ga[16];
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            bc_f4 v[4];
            bc_load_row<CH, NT>(op, 0, a, i, j, y, wave_edge, v);  // rows past the height repeat the last one: in bounds
            bc_quantise_row<CH, SRGB>(v, 0, y, srgb_t, rb, ga);
        }
        const bc_u2 blk = ld_policy<NT>(reinterpret_cast<const bc_u2 *>(a.dst + (size_t)j * a.row_pitch + (size_t)i * 8));
        uint32_t px[16];
        decode_bc1(blk.x, blk.y, false, px);
        const uint32_t cols = wave_edge ? min(a.w - 4u * i, 4u) : 4u, rows = wave_edge ? min(a.h - 4u * j, 4u) : 4u;
        uint32_t s[4] = { 0u, 0u, 0u, 0u };  // of this block: 16 * 255^2 fits
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const bool in = !wave_edge || ((uint32_t)(t & 3) < cols && (uint32_t)(t >> 2) < rows);  // replicated edge texels do not count
            const bool opaque = (ga[t] >> 16) >= ref;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t src = c == 3 ? (opaque ? 255u : 0u) : __builtin_amdgcn_ubfe((c & 1) ? ga[t] : rb[t], (c & 2) ? 16u : 0u, 16u);
                const uint32_t dec = (px[t] >> (8 * c)) & 0xffu;
                const uint32_t d = in && (c == 3 || opaque) ? (src > dec ? src - dec : dec - src) : 0u;
                s[c] += d * d;
                mx[c] = max(mx[c], d);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) sse[c] += s[c];
    }
    unsigned long long val[KC_BC_REC_WORDS];
#pragma unroll
    for (uint32_t w = 0; w < KC_BC_REC_WORDS; ++w) val[w] = 0ull;
#pragma unroll
    for (int c = 0; c < 4; ++c) val[c] = sse[c], val[4 + c] = mx[c];
    bc_fold_record<KC_BC_REC_WORDS, 0xffu>(val, red, partials + (size_t)blockIdx.x * KC_BC_REC_WORDS);  // the other words are 0 in every thread
}

hipError_t launch_bc1a_encode(int srgb, const Operand op[4], uint32_t ref, char *dst, uint64_t row_pitch, uint32_t w, uint32_t h, uint32_t nt_mask,
                              hipStream_t s)
{
    const BcBlockArgs a = bc_block_args(dst, row_pitch, w, h);
    const uint64_t total = (uint64_t)a.bx * a.by;
    if (total == 0) return hipSuccess;
    if (ref < 1u || ref > 255u) return hipErrorInvalidValue;
    const uint32_t blocks = bc_grid(total, 1u << 30);
    const bool nt = (nt_mask & 0xffu) != 0;
#define KC_BC1A(SR, NTL) bc1a_encode_kernel<SR, NTL><<<dim3(blocks), 256, 0, s>>>(op[0], op[1], op[2], op[3], a, ref)
    if (srgb) {
        if (nt) KC_BC1A(true, true);
        else KC_BC1A(true, false);
    } else {
        if (nt) KC_BC1A(false, true);
        else KC_BC1A(false, false);
    }
#undef KC_BC1A
    return hipGetLastError();
}

hipError_t launch_bc1a_compare(int srgb, const Operand op[4], uint32_t ref, const char *blocks, uint64_t row_pitch, uint32_t w, uint32_t h,
                               uint32_t nt_mask, uint32_t groups, unsigned long long *partials, unsigned long long *result, hipStream_t s)
{
    const BcBlockArgs a = bc_block_args(const_cast<char *>(blocks), row_pitch, w, h);  // read only here
    if (groups == 0 || a.bx == 0 || a.by == 0 || !partials || !result || ref < 1u || ref > 255u) return hipErrorInvalidValue;
    const bool nt = (nt_mask & 0xffu) != 0;
#define KC_BC1A(SR, NTL) bc1a_compare_kernel<SR, NTL><<<dim3(groups), 256, 0, s>>>(op[0], op[1], op[2], op[3], a, ref, partials)
    if (srgb) {
        if (nt) KC_BC1A(true, true);
        else KC_BC1A(true, false);
    } else {
        if (nt) KC_BC1A(false, true);
        else KC_BC1A(false, false);
    }
#undef KC_BC1A
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_bc_combine(partials, groups, KC_BC_REC_WORDS, 0xf0u, result, s);
}

}  // namespace kc
