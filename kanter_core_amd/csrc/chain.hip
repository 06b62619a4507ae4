// The Mix-chain interpreter kernels: chain_kernel runs a step program of any length on up to four input planes (what a
// program runs through until specialize.cpp has compiled a kernel for it; one-step programs: chain1.hip), chain_kernel_k0
// the programs without an input plane -- and fill_kernel, a constant plane.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // ld_policy / st_policy
#include "chain_apply.inc"  // splat4, f4, kc_powf, apply1<CODE>: shared with chain1.hip
#include "chain_interp.inc"  // apply4 / apply4c, KC_CODE_SWITCH*, chain_run: shared by chain.hip, resize_tile.hip and upsample.hip

// Fused Mix chain (src/node/mix.rs:136-192 applied N times without materialising the
// intermediates).  K = distinct input planes, U = float4 per thread per decode, MODE = op set.
// Algorithmic HBM bytes per pixel: 4 * (planes read + 1 written), whatever N is.
// NT: the launch's cache policy marks streams (ChainProgram::nt_mask != 0): every full-size input is read and the result stored
// with the nontemporal hint.  (The interpreter runs a program's first two sightings only; it does not distinguish which input
// the policy would have kept cacheable -- the kernels compiled for the program do.)
template <int K, int U, int MODE, bool NT = false>
__global__ __launch_bounds__(256) void chain_kernel(const ChainProgram P)
{
    __shared__ double pow_lds[MODE >= 2 ? KC_POW_TABLE_DOUBLES : 1];
    PowCtx pw{};
    if constexpr (MODE >= 2) pw = pow_setup(pow_lds);
    const PowCtx *pow_tab = &pw;
    const uint32_t b = blockIdx.y;
    const uint32_t total = P.rows * P.row_units;
    const bool flat = P.rows == 1;
    const f4 *inp[K];
    uint32_t ipitch[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        inp[k] = reinterpret_cast<const f4 *>(P.in[b][k]);
        ipitch[k] = P.in_pitch[b][k];
    }
    f4 *outp = reinterpret_cast<f4 *>(P.out[b]);
    const uint32_t opitch = P.out_pitch[b];
    const uint32_t step = gridDim.x * (256u * U);

    for (uint32_t base = blockIdx.x * (256u * U) + threadIdx.x; base < total; base += step) {
        f4 in[K][U];
        f4 acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t idx = base + u * 256u;
            uint32_t row = 0, col = idx;
            if (!flat) {
                row = idx / P.row_units;
                col = idx - row * P.row_units;
            }
#pragma unroll
            for (int k = 0; k < K; ++k)
                in[k][u] = idx < total ? ld_policy<NT>(&inp[k][row * ipitch[k] + col]) : f4{ 0.0f, 0.0f, 0.0f, 0.0f };
        }

        chain_run<K, U, MODE>(P, b, in, acc, pow_tab);

        // output offsets are recomputed here rather than kept live across the program (VGPRs)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t idx = base + u * 256u;
            uint32_t row = 0, col = idx;
            if (!flat) {
                row = idx / P.row_units;
                col = idx - row * P.row_units;
            }
            if (idx < total) st_policy<NT>(&outp[row * opitch + col], acc[u]);
        }
    }
}

// Zero-input chain (constant start, constant operands only): still one pass of stores.
template <int MODE>
__global__ __launch_bounds__(256) void chain_kernel_k0(const ChainProgram P)
{
    __shared__ double pow_lds[MODE >= 2 ? KC_POW_TABLE_DOUBLES : 1];
    PowCtx pw{};
    if constexpr (MODE >= 2) pw = pow_setup(pow_lds);
    const PowCtx *tab = &pw;
    const uint32_t b = blockIdx.y;
    const uint32_t total = P.rows * P.row_units;
    const bool flat = P.rows == 1;
    f4 *outp = reinterpret_cast<f4 *>(P.out[b]);
    const uint32_t opitch = P.out_pitch[b];
    f4 acc[1];
    acc[0] = f4{ P.start_c[b], P.start_c[b], P.start_c[b], P.start_c[b] };
    for (uint32_t i = 0; i < P.n_ops; ++i) {
        const ChainStepRec r = (i & 1u) ? P.step[b][i / 2].b : P.step[b][i / 2].a;
        const uint32_t w = r.word;
        const float c = r.c;
        f4 nxt[1];
#define KC_APPLY_C(CODE, DST, SRC) apply4c<CODE, 1>(DST, SRC, c, tab)
        KC_CODE_SWITCH(KC_APPLY_C, nxt, acc)
#undef KC_APPLY_C
        acc[0] = nxt[0];
    }
    const uint32_t step = gridDim.x * 256u;
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += step) {
        uint32_t row = 0, col = idx;
        if (!flat) {
            row = idx / P.row_units;
            col = idx - row * P.row_units;
        }
        outp[row * opitch + col] = acc[0];
    }
}

template <int U, int MODE>
static hipError_t launch_chain_k(const ChainProgram &p, dim3 grid, hipStream_t s, ChainVariant *var)
{
    // the nontemporal form exists for the default shapes only (U = 4 without pow, U = 1 with): tuning overrides stay plain
    constexpr bool HAS_NT = (MODE < 2 && U == 4) || (MODE == 2 && U == 1);
    if (var) {
        var->k = (int)p.n_in;
        var->u = p.n_in == 0 ? 1 : U;
        var->mode = MODE;
        var->nt = false;
    }
    if constexpr (HAS_NT) {
        if (p.nt_mask != 0) {
            if (var) var->nt = p.n_in >= 1 && p.n_in <= 4;
            switch (p.n_in) {
            case 1: chain_kernel<1, U, MODE, true><<<grid, 256, 0, s>>>(p); return hipGetLastError();
            case 2: chain_kernel<2, U, MODE, true><<<grid, 256, 0, s>>>(p); return hipGetLastError();
            case 3: chain_kernel<3, U, MODE, true><<<grid, 256, 0, s>>>(p); return hipGetLastError();
            case 4: chain_kernel<4, U, MODE, true><<<grid, 256, 0, s>>>(p); return hipGetLastError();
            default: break;
            }
        }
    }
    switch (p.n_in) {
    case 0: chain_kernel_k0<MODE><<<grid, 256, 0, s>>>(p); break;
    case 1: chain_kernel<1, U, MODE><<<grid, 256, 0, s>>>(p); break;
    case 2: chain_kernel<2, U, MODE><<<grid, 256, 0, s>>>(p); break;
    case 3: chain_kernel<3, U, MODE><<<grid, 256, 0, s>>>(p); break;
    case 4: chain_kernel<4, U, MODE><<<grid, 256, 0, s>>>(p); break;
    default:
        if (var) var->k = -1;
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int U, int MODE>
static hipError_t launch_chain_u(const ChainProgram &p, int batch, uint64_t total, int max_blocks, hipStream_t s, ChainVariant *var)
{
    uint64_t blocks = (total + 256 * U - 1) / (256 * U);
    if (blocks > (uint64_t)max_blocks) blocks = max_blocks;
    return launch_chain_k<U, MODE>(p, dim3((unsigned)blocks, batch, 1), s, var);
}

hipError_t launch_chain(const ChainProgram &p, int batch, int mode, int max_blocks, int unroll, hipStream_t s, ChainVariant *var)
{
    if (batch < 1 || batch > KC_CHAIN_MAX_BATCH || p.n_ops > KC_CHAIN_MAX_OPS || p.n_ops < 1) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)p.rows * p.row_units;
    if (total == 0) return hipSuccess;
    if (total > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (mode >= 2) return launch_chain_u<1, 2>(p, batch, total, max_blocks, s, var);
    if (mode == 1) return launch_chain_u<4, 1>(p, batch, total, max_blocks, s, var);
    // U = float4 per lane per decode.  U = 4 (74-106 VGPRs, 4-6 waves/SIMD) is the measured optimum
    // on MI355X for 1-64 step chains: U = 2 doubles the scalar decode work per pixel, U = 8 drops to
    // 2-3 waves/SIMD (profiles/r01_chain_unroll.md).  KC_CHAIN_UNROLL / kc_set_option("chain_unroll") override for tuning.
    switch (unroll) {
    case 1: return launch_chain_u<1, 0>(p, batch, total, max_blocks, s, var);
    case 2: return launch_chain_u<2, 0>(p, batch, total, max_blocks, s, var);
    case 6: return launch_chain_u<6, 0>(p, batch, total, max_blocks, s, var);
    case 8: return launch_chain_u<8, 0>(p, batch, total, max_blocks, s, var);
    default: return launch_chain_u<4, 0>(p, batch, total, max_blocks, s, var);
    }
}

// vec![v; n] (src/slot_image.rs:28-64): only when a constant plane must really exist in HBM.
__global__ __launch_bounds__(256) void fill_kernel(float4 *dst, uint32_t pitch4, uint32_t row_units, uint32_t rows,
                                                   float v)
{
    const uint32_t total = rows * row_units;
    const float4 val = splat4(v);
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        const uint32_t row = idx / row_units;
        const uint32_t col = idx - row * row_units;
        dst[row * pitch4 + col] = val;
    }
}

hipError_t launch_fill(float *dst, uint32_t pitch_floats, uint32_t w, uint32_t h, float v, hipStream_t s)
{
    const uint32_t row_units = (w + 3) / 4;
    const uint64_t total = (uint64_t)row_units * h;
    if (total == 0) return hipSuccess;
    uint64_t blocks = (total + 255) / 256;
    // (a 64 MiB plane: 13.0 / 12.0 / 11.2 us with 1024 / 4096 / 16384 workgroups -- profiles/r04_write_bench.txt; 11.2 us = 6.0 TB/s
    // is what the memory system takes as writes from any kernel shape tried there)
    if (blocks > 16384) blocks = 16384;
    fill_kernel<<<dim3((unsigned)blocks), 256, 0, s>>>(reinterpret_cast<float4 *>(dst), pitch_floats / 4, row_units, h,
                                                        v);
    return hipGetLastError();
}

}  // namespace kc
