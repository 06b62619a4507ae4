// Block decode and the error of an encoding (kc_image_from_bc / kc_image_bc_compare, bc_decode.cpp): BC1, BC3, BC4, BC5 and the
// single-subset BC7 modes 4, 5 and 6 back to pixels, by the integer rules of include/kanter_core_amd.h (tests/bc_decode_ref.py
// is the same rules in numpy).  Both kernels are bc.hip's stream turned round: one thread per 4x4 block, a grid-stride loop over
// the blocks in row order, so the lanes of a wave hold consecutive blocks of a block row.  A block arrives in one 8- or 16-byte
// load and is expanded in registers to 16 RGBA8 words.
//   bc_decode_kernel   stores the four pixel rows of every resident plane as float4 (b / 255.f, from_u8's IEEE division)
//                      through bc_blocks.h's bc_store_planes, which bc6h.hip's decoder shares.
//   bc_compare_kernel  reads the image's planes as the encoder does (bc_blocks.h), quantises them with the encoder's functions
//                      and sums the squared byte differences over the pixels inside the image.
// The walk over the blocks and its edge rule are bc_blocks.h's.  Counts and sums are reduced per wave (shuffles), then per
// workgroup through LDS, to one record of u64 words per workgroup (bc_fold_record, there too); bc_combine_kernel folds the records into the result, one workgroup per word, without atomics.  Everything is an integer,
// so the result does not depend on the order.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // grid_cap, ld_policy / st_policy, quant_u8 / quant_u8_srgb
#include "bc_blocks.h"  // the block walk, the encoders' row loaders and quantiser, the plane-row store and the record fold

// decode_bc1: bc_blocks.h's
// BC4 of the 8 bytes (lo, hi) into bits sh..sh+7 of px
static __device__ __forceinline__ void decode_bc4(uint32_t lo, uint32_t hi, uint32_t sh, uint32_t (&px)[16])
{
    const uint32_t e0 = lo & 0xffu, e1 = (lo >> 8) & 0xffu;
    const bool eight = e0 > e1;
    // the palette as bytes of two words: indices 0..3 and 4..7
    uint32_t plo = e0 | (e1 << 8), phi = 0u;
#pragma unroll
    for (uint32_t i = 2; i < 8; ++i) {
        const uint32_t v8 = ((8u - i) * e0 + (i - 1u) * e1 + 3u) / 7u;
        const uint32_t v6 = i < 6 ? ((6u - i) * e0 + (i - 1u) * e1 + 2u) / 5u : i == 6 ? 0u : 255u;
        const uint32_t v = eight ? v8 : v6;
        if (i < 4) plo |= v << (8u * i);
        else phi |= v << (8u * (i - 4u));
    }
    const uint64_t bits = ((uint64_t)hi << 32 | lo) >> 16;  // the 48 index bits
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const uint32_t i = (uint32_t)(bits >> (3 * t)) & 7u;
        const uint32_t word = (i & 4u) ? phi : plo;
        px[t] |= __builtin_amdgcn_ubfe(word, 8u * (i & 3u), 8u) << sh;
    }
}

// The interpolation weights as expressions: W2[i] = (64 i + 1) div 3, W3[i] = (64 i + 3) div 7, W4[i] = (64 i + 7) div 15
static __device__ __forceinline__ uint32_t bc7_w2(uint32_t i) { return (64u * i + 1u) / 3u; }
static __device__ __forceinline__ uint32_t bc7_w3(uint32_t i) { return (64u * i + 3u) / 7u; }
static __device__ __forceinline__ uint32_t bc7_w4(uint32_t i) { return (64u * i + 7u) / 15u; }

// BC7 modes 4, 5 and 6 into px; *mode = the block's mode, 8 for the reserved block (byte 0 == 0).  Returns whether the block
// is one of the partitioned modes, which are not decoded (px = 0).
static __device__ __forceinline__ bool decode_bc7(const uint32_t (&b)[4], uint32_t (&px)[16], uint32_t *mode)
{
    const uint32_t byte0 = b[0] & 0xffu;
    const uint32_t m = byte0 ? (uint32_t)__builtin_ctz(byte0) : 8u;
    *mode = m;
    uint32_t e0[4] = { 0u, 0u, 0u, 0u }, e1[4] = { 0u, 0u, 0u, 0u }, rot = 0u;
    // px holds the weights first: colour | alpha << 8
    if (m == 6u) {
        const uint32_t p0 = bc_bits(b, 63, 1), p1 = bc_bits(b, 64, 1);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            e0[c] = 2u * bc_bits(b, 7 + 14 * c, 7) + p0;
            e1[c] = 2u * bc_bits(b, 14 + 14 * c, 7) + p1;
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const uint32_t w = bc7_w4(t == 0 ? bc_bits(b, 65, 3) : bc_bits(b, 68 + 4 * (t - 1), 4));
            px[t] = w | (w << 8);
        }
    } else if (m == 5u) {
        rot = bc_bits(b, 6, 2);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t q0 = bc_bits(b, 8 + 14 * c, 7), q1 = bc_bits(b, 15 + 14 * c, 7);
            e0[c] = (q0 << 1) | (q0 >> 6);
            e1[c] = (q1 << 1) | (q1 >> 6);
        }
        e0[3] = bc_bits(b, 50, 8);
        e1[3] = bc_bits(b, 58, 8);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const uint32_t ic = t == 0 ? bc_bits(b, 66, 1) : bc_bits(b, 67 + 2 * (t - 1), 2);
            const uint32_t ia = t == 0 ? bc_bits(b, 97, 1) : bc_bits(b, 98 + 2 * (t - 1), 2);
            px[t] = bc7_w2(ic) | (bc7_w2(ia) << 8);
        }
    } else if (m == 4u) {
        rot = bc_bits(b, 5, 2);
        const bool sel = bc_bits(b, 7, 1) != 0u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t q0 = bc_bits(b, 8 + 10 * c, 5), q1 = bc_bits(b, 13 + 10 * c, 5);
            e0[c] = (q0 << 3) | (q0 >> 2);
            e1[c] = (q1 << 3) | (q1 >> 2);
        }
        const uint32_t a0 = bc_bits(b, 38, 6), a1 = bc_bits(b, 44, 6);
        e0[3] = (a0 << 2) | (a0 >> 4);
        e1[3] = (a1 << 2) | (a1 >> 4);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const uint32_t w2 = bc7_w2(t == 0 ? bc_bits(b, 50, 1) : bc_bits(b, 51 + 2 * (t - 1), 2));
            const uint32_t w3 = bc7_w3(t == 0 ? bc_bits(b, 81, 2) : bc_bits(b, 83 + 3 * (t - 1), 3));
            px[t] = sel ? (w3 | (w2 << 8)) : (w2 | (w3 << 8));
        }
    } else {
        // reserved or partitioned: the endpoints stay 0 and every texel interpolates to 0
#pragma unroll
        for (int t = 0; t < 16; ++t) px[t] = 0u;
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const uint32_t wc = px[t] & 0xffu, wa = px[t] >> 8;
        uint32_t v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t w = c < 3 ? wc : wa;
            v[c] = ((64u - w) * e0[c] + w * e1[c] + 32u) >> 6;
        }
        // rotation r: alpha and channel r - 1 change places
        const uint32_t al = rot == 0u ? v[3] : rot == 1u ? v[0] : rot == 2u ? v[1] : v[2];
        const uint32_t r = rot == 1u ? v[3] : v[0], g = rot == 2u ? v[3] : v[1], bl = rot == 3u ? v[3] : v[2];
        px[t] = r | (g << 8) | (bl << 16) | (al << 24);
    }
    return m < 4u || m == 7u;
}

// One block of format FMT at p into px; *mode and the return value as decode_bc7's (other formats: mode 8, false)
template <int FMT, bool NT>
static __device__ __forceinline__ bool bc_decode_block(const char *p, uint32_t (&px)[16], uint32_t *mode)
{
    *mode = 8u;
    if constexpr (FMT == KC_BC1 || FMT == KC_BC4) {
        const bc_u2 v = ld_policy<NT>(reinterpret_cast<const bc_u2 *>(p));
        if constexpr (FMT == KC_BC1) decode_bc1(v.x, v.y, false, px);
        else {
#pragma unroll
            for (int t = 0; t < 16; ++t) px[t] = 0xff000000u;
            decode_bc4(v.x, v.y, 0u, px);
        }
        return false;
    } else {
        const bc_u4 v = ld_policy<NT>(reinterpret_cast<const bc_u4 *>(p));
        if constexpr (FMT == KC_BC3) {
            decode_bc1(v.z, v.w, true, px);
#pragma unroll
            for (int t = 0; t < 16; ++t) px[t] &= 0x00ffffffu;
            decode_bc4(v.x, v.y, 24u, px);
            return false;
        } else if constexpr (FMT == KC_BC5) {
#pragma unroll
            for (int t = 0; t < 16; ++t) px[t] = 0xff000000u;
            decode_bc4(v.x, v.y, 0u, px);
            decode_bc4(v.z, v.w, 8u, px);
            return false;
        } else {
            const uint32_t b[4] = { v.x, v.y, v.z, v.w };
            return decode_bc7(b, px, mode);
        }
    }
}

// What the kernels know of a format at compile time (the host's table is bc.cpp's bc_format): the block bytes, the channels the
// comparison reads (bit c = channel c) and the planes a decode writes
static constexpr size_t bc_bytes(int fmt) { return fmt == KC_BC1 || fmt == KC_BC4 ? 8 : 16; }
static constexpr uint32_t bc_channels(int fmt) { return fmt == KC_BC1 ? 0x7u : fmt == KC_BC4 ? 0x1u : fmt == KC_BC5 ? 0x3u : 0xfu; }
static constexpr int bc_decode_planes(int fmt) { return fmt == KC_BC4 ? 1 : fmt == KC_BC5 ? 2 : 4; }

// COUNT (instantiated for BC7, the one format of this unit with modes that are not decoded; BC6H's decoder, which counts too, is
// bc6h.hip's): the workgroup's undecoded blocks go to a.partials[blockIdx.x]
template <int FMT, bool NT, bool COUNT>
__global__ __launch_bounds__(256) void bc_decode_kernel(const BcDecodeArgs a)
{
    [[maybe_unused]] __shared__ unsigned long long red[4][1];  // per wave
    const BcWalk k = bc_walk(a.w, a.h, a.bx, a.by);
    unsigned long long undecoded[1] = { 0ull };
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < k.total; idx += gridDim.x * 256u) {
        uint32_t i, j;
        const bool wave_edge = bc_block_of(k, idx, i, j);
        uint32_t px[16], mode;
        const bool skipped = bc_decode_block<FMT, NT>(a.src + (size_t)j * a.row_pitch + (size_t)i * bc_bytes(FMT), px, &mode);
        if constexpr (COUNT) undecoded[0] += skipped ? 1u : 0u;
        bc_store_planes<bc_decode_planes(FMT), NT>(a, i, j, wave_edge, [&](int c, int t) {
            return (float)((px[t] >> (8 * c)) & 0xffu) / 255.0f;  // from_u8's IEEE division
        });
    }
    if constexpr (COUNT) bc_fold_record<1, 0x1u>(undecoded, red, a.partials + blockIdx.x);
}

// Record of a workgroup, KC_BC_REC_WORDS u64: [0..3] the squared error per channel, [4..7] the largest absolute difference,
// [8] undecoded blocks, [9..16] BC7 blocks per mode.
template <int FMT, bool SRGB, bool NT>
__global__ __launch_bounds__(256) void bc_compare_kernel(Operand r, Operand g, Operand b, Operand al, int gray, const BcBlockArgs a,
                                                         unsigned long long *partials)
{
    __shared__ uint32_t srgb_t[SRGB ? 257 : 1];
    __shared__ unsigned long long red[4][KC_BC_REC_WORDS];  // per wave
    constexpr uint32_t CH = bc_channels(FMT);
    const Operand op[4] = { r, g, b, al };
    if constexpr (SRGB) bc_stage_srgb(srgb_t);
    const BcWalk k = bc_walk(a.w, a.h, a.bx, a.by);
    unsigned long long sse[4] = { 0ull, 0ull, 0ull, 0ull };
    uint32_t mx[4] = { 0u, 0u, 0u, 0u }, undecoded = 0u, modes[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
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
        uint32_t px[16], mode;
        const bool skipped = bc_decode_block<FMT, NT>(a.dst + (size_t)j * a.row_pitch + (size_t)i * bc_bytes(FMT), px, &mode);
        if constexpr (FMT == KC_BC7) {
            undecoded += skipped ? 1u : 0u;
#pragma unroll
            for (uint32_t m = 0; m < 8; ++m) modes[m] += mode == m ? 1u : 0u;
        }
        const uint32_t cols = wave_edge ? min(a.w - 4u * i, 4u) : 4u, rows = wave_edge ? min(a.h - 4u * j, 4u) : 4u;
        uint32_t s[4] = { 0u, 0u, 0u, 0u };  // of this block: 16 * 255^2 fits
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const bool in = !wave_edge || ((uint32_t)(t & 3) < cols && (uint32_t)(t >> 2) < rows);  // replicated edge texels do not count
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (!((CH >> c) & 1u)) continue;
                const uint32_t src = __builtin_amdgcn_ubfe((c & 1) ? ga[t] : rb[t], (c & 2) ? 16u : 0u, 16u);
                const uint32_t dec = (px[t] >> (8 * c)) & 0xffu;
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
    val[8] = undecoded;
#pragma unroll
    for (int m = 0; m < 8; ++m) val[9 + m] = modes[m];
    // the channels the format holds, and BC7's counts: the other words are 0 in every thread
    bc_fold_record<KC_BC_REC_WORDS, CH | CH << 4 | (FMT == KC_BC7 ? 0x1ff00u : 0u)>(val, red, partials + (size_t)blockIdx.x * KC_BC_REC_WORDS);
}

// result[col] = the sum (max_cols bit col set: the maximum) of word col of the `groups` records of rec_words words: one
// workgroup per word
__global__ __launch_bounds__(256) void bc_combine_kernel(const unsigned long long *partials, uint32_t groups, uint32_t rec_words,
                                                         uint32_t max_cols, unsigned long long *result)
{
    __shared__ unsigned long long red[256];
    const uint32_t col = blockIdx.x;
    const bool is_max = (max_cols >> col) & 1u;
    unsigned long long acc = 0ull;
    for (uint32_t r = threadIdx.x; r < groups; r += 256u) {
        const unsigned long long v = partials[(size_t)r * rec_words + col];
        acc = is_max ? (v > acc ? v : acc) : acc + v;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t n = 128u; n > 0u; n >>= 1) {
        if (threadIdx.x < n) {
            const unsigned long long v = red[threadIdx.x + n];
            red[threadIdx.x] = is_max ? (v > red[threadIdx.x] ? v : red[threadIdx.x]) : red[threadIdx.x] + v;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) result[col] = red[0];
}

hipError_t launch_bc_combine(const unsigned long long *partials, uint32_t groups, uint32_t rec_words, uint32_t max_cols,
                             unsigned long long *result, hipStream_t s)
{
    bc_combine_kernel<<<dim3(rec_words), 256, 0, s>>>(partials, groups, rec_words, max_cols, result);
    return hipGetLastError();
}

uint32_t bc_decode_groups(uint32_t w, uint32_t h, bool count)
{
    // one record per workgroup when counting: the grid-stride loop takes the rest
    return bc_grid((uint64_t)((w + 3) / 4) * ((h + 3) / 4), count ? 1u << 16 : 1u << 30);
}

uint32_t bc_compare_groups(uint32_t w, uint32_t h)
{
    // one block a thread, as the encoder, while the records stay few (2^16 of them are 8.5 MiB); the loop takes the rest
    return bc_grid((uint64_t)((w + 3) / 4) * ((h + 3) / 4), 1u << 16);
}

hipError_t launch_bc_decode(int fmt, const BcDecodeArgs &a, bool count, uint32_t nt_mask, uint32_t groups, hipStream_t s)
{
    if (groups == 0 || a.bx == 0 || a.by == 0) return hipErrorInvalidValue;
    // of this unit's formats only BC7 has modes that are not decoded (BC6H counts too, in its own unit: launch_bc6h_decode)
    if (count && (fmt != KC_BC7 || !a.partials || !a.result)) return hipErrorInvalidValue;
    const bool nt = (nt_mask & 0x100u) != 0;  // the planes written are the launch's stream
#define KC_BCD(F, NTL, CNT) bc_decode_kernel<F, NTL, CNT><<<dim3(groups), 256, 0, s>>>(a)
#define KC_BCD_NT(F)                                                                                                                  \
    do {                                                                                                                             \
        if (nt) KC_BCD(F, true, false);                                                                                              \
        else KC_BCD(F, false, false);                                                                                                \
    } while (0)
    switch (fmt) {
    case KC_BC1: KC_BCD_NT(KC_BC1); break;
    case KC_BC3: KC_BCD_NT(KC_BC3); break;
    case KC_BC4: KC_BCD_NT(KC_BC4); break;
    case KC_BC5: KC_BCD_NT(KC_BC5); break;
    case KC_BC7:
        if (!count) KC_BCD_NT(KC_BC7);
        else if (nt) KC_BCD(KC_BC7, true, true);
        else KC_BCD(KC_BC7, false, true);
        break;
    default: return hipErrorInvalidValue;
    }
#undef KC_BCD_NT
#undef KC_BCD
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !count) return e;
    return launch_bc_combine(a.partials, groups, 1u, 0u, a.result, s);
}

hipError_t launch_bc_compare(int fmt, int srgb, const Operand op[4], int gray, const char *blocks, uint64_t row_pitch, uint32_t w, uint32_t h,
                             uint32_t nt_mask, uint32_t groups, unsigned long long *partials, unsigned long long *result, hipStream_t s)
{
    const BcBlockArgs a = bc_block_args(const_cast<char *>(blocks), row_pitch, w, h);  // read only here
    if (groups == 0 || a.bx == 0 || a.by == 0 || !partials || !result) return hipErrorInvalidValue;
    if (srgb && fmt != KC_BC1 && fmt != KC_BC3 && fmt != KC_BC7) return hipErrorInvalidValue;  // no such instantiation
    const bool nt = (nt_mask & 0xffu) != 0;
#define KC_BCC(F, SR, NTL) bc_compare_kernel<F, SR, NTL><<<dim3(groups), 256, 0, s>>>(op[0], op[1], op[2], op[3], gray, a, partials)
#define KC_BCC_NT(F, SR)                                                                                                              \
    do {                                                                                                                             \
        if (nt) KC_BCC(F, SR, true);                                                                                                 \
        else KC_BCC(F, SR, false);                                                                                                   \
    } while (0)
    switch (fmt) {
    case KC_BC1:
        if (srgb) KC_BCC_NT(KC_BC1, true);
        else KC_BCC_NT(KC_BC1, false);
        break;
    case KC_BC3:
        if (srgb) KC_BCC_NT(KC_BC3, true);
        else KC_BCC_NT(KC_BC3, false);
        break;
    case KC_BC7:
        if (srgb) KC_BCC_NT(KC_BC7, true);
        else KC_BCC_NT(KC_BC7, false);
        break;
    case KC_BC4: KC_BCC_NT(KC_BC4, false); break;
    case KC_BC5: KC_BCC_NT(KC_BC5, false); break;
    default: return hipErrorInvalidValue;
    }
#undef KC_BCC_NT
#undef KC_BCC
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_bc_combine(partials, groups, KC_BC_REC_WORDS, 0xf0u, result, s);
}

}  // namespace kc
