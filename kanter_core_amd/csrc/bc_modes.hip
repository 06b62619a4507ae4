// Block decode and the error of an encoding with every mode (KC_BC_ALL_MODES; bc.cpp picks this unit for KC_BC7 and KC_BC6H under
// the flag): BC7 modes 0-7 and the unsigned BC6H modes 1-14, partition tables included, by the integer rules of
// include/kanter_core_amd.h (tests/bc_modes_ref.py is the same rules in numpy).  The streams are bc_decode.hip's and bc6h.hip's,
// built from bc_blocks.h's steps: one thread per 4x4 block, a grid-stride loop over the blocks in row order, the block in one
// 16-byte load, the plane-row store, the encoders' row loaders and quantisers, the record fold, nontemporal instantiations and the
// wave-uniform edge-block test.  The decoders are bc_modes.h's: table-driven, one instruction stream for every mode, the tables
// staged in LDS by the workgroup.  Nothing is left undecoded, so no decoder counts and a decode is one launch.
//   bc7_modes_decode_kernel   / bc6h_modes_decode_kernel    sixteen texels into registers, then the plane rows
//   bc7_modes_compare_kernel  / bc6h_modes_compare_kernel   a texel is decoded inside the error loop and never kept: beside the 32
//                                                           source words a thread holds the block's state, not 16 decoded words
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // grid_cap, ld_policy / st_policy, quant_u8 / quant_u8_srgb
#include "bc_blocks.h"  // the block walk, the row loaders and quantisers, the plane-row store, the record fold and BC6H's rules
#include "bc_modes.h"   // the decoders and their tables

// The decoders' table into LDS by the workgroup's 256 threads (WORDS <= 256): a global read and a barrier that every thread takes
template <uint32_t WORDS, class Word>
static __device__ __forceinline__ void bcm_stage(uint32_t *tab, Word word)
{
    static_assert(WORDS <= 256u, "one word a thread");
    if (threadIdx.x < WORDS) tab[threadIdx.x] = word(threadIdx.x);
    __syncthreads();
}

template <bool NT>
static __device__ __forceinline__ void bcm_load_block(const char *p, uint32_t (&b)[4])
{
    const bc_u4 v = ld_policy<NT>(reinterpret_cast<const bc_u4 *>(p));
    b[0] = v.x, b[1] = v.y, b[2] = v.z, b[3] = v.w;
}

// ---------------------------------------------------------------- decode
template <bool NT>
__global__ __launch_bounds__(256) void bc7_modes_decode_kernel(const BcDecodeArgs a)
{
    __shared__ uint32_t tab[BC7_TAB_WORDS];
    bcm_stage<BC7_TAB_WORDS>(tab, [](uint32_t i) { return bc7_table_word(i); });
    const BcWalk k = bc_walk(a.w, a.h, a.bx, a.by);
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < k.total; idx += gridDim.x * 256u) {
        uint32_t i, j;
        const bool wave_edge = bc_block_of(k, idx, i, j);
        Bc7Block blk;
        bcm_load_block<NT>(a.src + (size_t)j * a.row_pitch + (size_t)i * 16, blk.b);
        bc7_read_header(tab, blk);
        uint32_t px[16];
#pragma unroll
        for (uint32_t t = 0; t < 16u; ++t) px[t] = bc7_texel(blk, tab, t);
        bc_store_planes<4, NT>(a, i, j, wave_edge, [&](int c, int t) {
            return (float)((px[t] >> (8 * c)) & 0xffu) / 255.0f;  // from_u8's IEEE division
        });
    }
}

// Writes dst[0..2] = R, G, B
template <bool NT>
__global__ __launch_bounds__(256) void bc6h_modes_decode_kernel(const BcDecodeArgs a)
{
    __shared__ uint32_t tab[BC6H_TAB_WORDS];
    bcm_stage<BC6H_TAB_WORDS>(tab, [](uint32_t i) { return bc6h_table_word(i); });
    const BcWalk k = bc_walk(a.w, a.h, a.bx, a.by);
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < k.total; idx += gridDim.x * 256u) {
        uint32_t i, j;
        const bool wave_edge = bc_block_of(k, idx, i, j);
        Bc6hBlock blk;
        bcm_load_block<NT>(a.src + (size_t)j * a.row_pitch + (size_t)i * 16, blk.b);
        bc6h_read_header(tab, blk);
        uint32_t rg[16], bl[16];
#pragma unroll
        for (uint32_t t = 0; t < 16u; ++t) bc6h_texel(blk, t, &rg[t], &bl[t]);
        bc_store_planes<3, NT>(a, i, j, wave_edge, [&](int c, int t) { return half_value(c == 0 ? rg[t] & 0xffffu : c == 1 ? rg[t] >> 16 : bl[t]); });
    }
}

// ---------------------------------------------------------------- the error of an encoding
// Record of a workgroup, bc_decode.hip's layout: [0..3] the squared error per channel, [4..7] the largest absolute difference,
// [8] undecoded blocks (0 here), [9..16] BC7 blocks per mode.
template <bool SRGB, bool NT>
__global__ __launch_bounds__(256) void bc7_modes_compare_kernel(Operand r, Operand g, Operand b, Operand al, int gray, const BcBlockArgs a,
                                                                unsigned long long *partials)
{
    __shared__ uint32_t tab[BC7_TAB_WORDS];
    __shared__ uint32_t srgb_t[SRGB ? 257 : 1];
    __shared__ unsigned long long red[4][KC_BC_REC_WORDS];  // per wave
    constexpr uint32_t CH = 0xfu;
    const Operand op[4] = { r, g, b, al };
    if constexpr (SRGB) bc_stage_srgb(srgb_t);
    bcm_stage<BC7_TAB_WORDS>(tab, [](uint32_t i) { return bc7_table_word(i); });
    const BcWalk k = bc_walk(a.w, a.h, a.bx, a.by);
    unsigned long long sse[4] = { 0ull, 0ull, 0ull, 0ull };
    uint32_t mx[4] = { 0u, 0u, 0u, 0u }, modes[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < k.total; idx += gridDim.x * 256u) {
        uint32_t i, j;
        const bool wave_edge = bc_block_of(k, idx, i, j);
        uint32_t rb[16], ga[16];
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            bc_f4 v[4];
            bc_load_row<CH, NT>(op, gray, a, i, j, y, wave_edge, v);  // rows past the height repeat the last one: in bounds
            bc_quantise_row<CH, SRGB>(v, gray, y, srgb_t, rb, ga);
        }
        Bc7Block blk;
        bcm_load_block<NT>(a.dst + (size_t)j * a.row_pitch + (size_t)i * 16, blk.b);
        bc7_read_header(tab, blk);
#pragma unroll
        for (uint32_t m = 0; m < 8; ++m) modes[m] += blk.mode == m ? 1u : 0u;
        const uint32_t cols = wave_edge ? min(a.w - 4u * i, 4u) : 4u, rows = wave_edge ? min(a.h - 4u * j, 4u) : 4u;
        uint32_t s[4] = { 0u, 0u, 0u, 0u };  // of this block: 16 * 255^2 fits
#pragma unroll
        for (uint32_t t = 0; t < 16u; ++t) {
            const bool in = !wave_edge || ((t & 3u) < cols && (t >> 2) < rows);  // replicated edge texels do not count
            const uint32_t px = bc7_texel(blk, tab, t);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t src = __builtin_amdgcn_ubfe((c & 1) ? ga[t] : rb[t], (c & 2) ? 16u : 0u, 16u);
                const uint32_t dec = (px >> (8 * c)) & 0xffu;
                const uint32_t d = in ? (src > dec ? src - dec : dec - src) : 0u;
                s[c] += d * d;
                mx[c] = max(mx[c], d);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) sse[c] += s[c];
    }
    unsigned long long val[KC_BC_REC_WORDS];
#pragma unroll
    for (int c = 0; c < 4; ++c) val[c] = sse[c], val[4 + c] = mx[c];
    val[8] = 0ull;
#pragma unroll
    for (int m = 0; m < 8; ++m) val[9 + m] = modes[m];
    bc_fold_record<KC_BC_REC_WORDS, 0x1feffu>(val, red, partials + (size_t)blockIdx.x * KC_BC_REC_WORDS);  // word 8 is 0 in every thread
}

// [0..2] the squared error of R, G, B over the half bit patterns, [4..6] the largest absolute difference; the other words are 0
template <bool NT>
__global__ __launch_bounds__(256) void bc6h_modes_compare_kernel(Operand r, Operand g, Operand b, int gray, const BcBlockArgs a,
                                                                 unsigned long long *partials)
{
    __shared__ uint32_t tab[BC6H_TAB_WORDS];
    __shared__ unsigned long long red[4][KC_BC_REC_WORDS];  // per wave
    constexpr uint32_t CH = 0x7u;
    const Operand op[4] = { r, g, b, Operand{ nullptr, 0, 1.0f } };
    bcm_stage<BC6H_TAB_WORDS>(tab, [](uint32_t i) { return bc6h_table_word(i); });
    const BcWalk k = bc_walk(a.w, a.h, a.bx, a.by);
    unsigned long long sse[3] = { 0ull, 0ull, 0ull };
    uint32_t mx[3] = { 0u, 0u, 0u };
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < k.total; idx += gridDim.x * 256u) {
        uint32_t i, j;
        const bool wave_edge = bc_block_of(k, idx, i, j);
        uint32_t rg[16], bl[16];
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            bc_f4 v[4];
            bc_load_row<CH, NT>(op, gray, a, i, j, y, wave_edge, v);  // rows past the height repeat the last one: in bounds
            bc6h_quantise_row(v, gray, y, rg, bl);
        }
        Bc6hBlock blk;
        bcm_load_block<NT>(a.dst + (size_t)j * a.row_pitch + (size_t)i * 16, blk.b);
        bc6h_read_header(tab, blk);
        const uint32_t cols = wave_edge ? min(a.w - 4u * i, 4u) : 4u, rows = wave_edge ? min(a.h - 4u * j, 4u) : 4u;
#pragma unroll
        for (uint32_t t = 0; t < 16u; ++t) {
            const bool in = !wave_edge || ((t & 3u) < cols && (t >> 2) < rows);  // replicated edge texels do not count
            uint32_t drg, dbl;
            bc6h_texel(blk, t, &drg, &dbl);
            const uint32_t src[3] = { rg[t] & 0xffffu, rg[t] >> 16, bl[t] }, dec[3] = { drg & 0xffffu, drg >> 16, dbl };
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t d = in ? (src[c] > dec[c] ? src[c] - dec[c] : dec[c] - src[c]) : 0u;  // <= 31743: d * d fits 32 bits
                sse[c] += d * d;  // sixteen of them do not: the sum is 64-bit
                mx[c] = max(mx[c], d);
            }
        }
    }
    unsigned long long val[KC_BC_REC_WORDS];
#pragma unroll
    for (uint32_t w = 0; w < KC_BC_REC_WORDS; ++w) val[w] = 0ull;
#pragma unroll
    for (int c = 0; c < 3; ++c) val[c] = sse[c], val[4 + c] = mx[c];
    bc_fold_record<KC_BC_REC_WORDS, 0x77u>(val, red, partials + (size_t)blockIdx.x * KC_BC_REC_WORDS);  // words 0-2 and 4-6
}

// ---------------------------------------------------------------- launchers
hipError_t launch_bc_modes_decode(int fmt, const BcDecodeArgs &a, uint32_t nt_mask, uint32_t groups, hipStream_t s)
{
    if (groups == 0 || a.bx == 0 || a.by == 0) return hipErrorInvalidValue;
    const bool nt = (nt_mask & 0x100u) != 0;  // the planes written are the launch's stream
    if (fmt == KC_BC7) {
        if (nt) bc7_modes_decode_kernel<true><<<dim3(groups), 256, 0, s>>>(a);
        else bc7_modes_decode_kernel<false><<<dim3(groups), 256, 0, s>>>(a);
    } else if (fmt == KC_BC6H) {
        if (nt) bc6h_modes_decode_kernel<true><<<dim3(groups), 256, 0, s>>>(a);
        else bc6h_modes_decode_kernel<false><<<dim3(groups), 256, 0, s>>>(a);
    } else {
        return hipErrorInvalidValue;  // the other formats have no modes: bc_decode.hip's kernels serve them with and without the flag
    }
    return hipGetLastError();
}

hipError_t launch_bc_modes_compare(int fmt, int srgb, const Operand op[4], int gray, const char *blocks, uint64_t row_pitch, uint32_t w,
                                   uint32_t h, uint32_t nt_mask, uint32_t groups, unsigned long long *partials, unsigned long long *result,
                                   hipStream_t s)
{
    const BcBlockArgs a = bc_block_args(const_cast<char *>(blocks), row_pitch, w, h);  // read only here
    if (groups == 0 || a.bx == 0 || a.by == 0 || !partials || !result) return hipErrorInvalidValue;
    if (srgb && fmt != KC_BC7) return hipErrorInvalidValue;  // no such instantiation
    const bool nt = (nt_mask & 0xffu) != 0;
#define KC_BCM7(SR, NTL) bc7_modes_compare_kernel<SR, NTL><<<dim3(groups), 256, 0, s>>>(op[0], op[1], op[2], op[3], gray, a, partials)
    if (fmt == KC_BC7) {
        if (srgb && nt) KC_BCM7(true, true);
        else if (srgb) KC_BCM7(true, false);
        else if (nt) KC_BCM7(false, true);
        else KC_BCM7(false, false);
    } else if (fmt == KC_BC6H) {
        if (nt) bc6h_modes_compare_kernel<true><<<dim3(groups), 256, 0, s>>>(op[0], op[1], op[2], gray, a, partials);
        else bc6h_modes_compare_kernel<false><<<dim3(groups), 256, 0, s>>>(op[0], op[1], op[2], gray, a, partials);
    } else {
        return hipErrorInvalidValue;
    }
#undef KC_BCM7
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_bc_combine(partials, groups, KC_BC_REC_WORDS, 0xf0u, result, s);
}

}  // namespace kc
