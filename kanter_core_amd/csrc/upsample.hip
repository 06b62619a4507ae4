// ------------------------------------------------------------------------------------------
// Integer-ratio up-sampling (upsample.h, upsample_chain.inc): the fused resample + chain kernel and the plain resize
// kernel for out = R x in.  Replaces resize_chain_kernel / resize_lds_kernel where the host's check holds; same
// operations per sample, bit-identical output.
// ------------------------------------------------------------------------------------------
#include "kc_internal.hpp"

namespace kc {

#include "chain_apply.inc"  // f4, apply1<CODE>
#include "chain_interp.inc"  // apply4 / apply4c, KC_CODE_SWITCH*, chain_run: shared by chain.hip, resize_tile.hip and upsample.hip
#include "upsample_chain.inc"

// Rows per thread (one trip per workgroup, see upsample_chain.inc).  KC_UP_RU at build time overrides (tuning).
#ifndef KC_UP_RU
#define KC_UP_RU 4
#endif
static_assert(KC_UP_RU == KC_UPSAMPLE_ROWS, "kc_internal.hpp sizes the tiles for this many rows per thread");

template <int K, int RU>
struct UpInterpreted {  // the chain as the step interpreter runs it (first sightings, no hiprtc)
    const ChainProgram &P;
    __device__ __forceinline__ void operator()(const f4 (&in)[K][RU], f4 (&acc)[RU]) const { chain_run<K, RU, 0>(P, blockIdx.z, in, acc); }
};

template <int RU>
struct UpStore {  // no chain: the resampled plane itself is the result
    __device__ __forceinline__ void operator()(const f4 (&in)[1][RU], f4 (&acc)[RU]) const
    {
#pragma unroll
        for (int u = 0; u < RU; ++u) acc[u] = in[0][u];
    }
};

#ifdef KC_UP_HARDWIRE  // tuning builds only: config #2's program ((A + U) * A - U) in place of the interpreter
template <int K, int RU>
struct UpHardwired {
    __device__ __forceinline__ void operator()(const f4 (&in)[K][RU], f4 (&acc)[RU]) const
    {
#pragma unroll
        for (int u = 0; u < RU; ++u) acc[u] = (in[0][u] + in[K - 1][u]) * in[0][u] - in[K - 1][u];
    }
};
#endif

#ifdef KC_UP_SGPR
#define KC_UP_ATTR __attribute__((amdgpu_num_sgpr(KC_UP_SGPR)))
#else
#define KC_UP_ATTR
#endif
template <int K, int T, bool WIDE, bool HALF>  // HALF: the horizontal ratio is 2 (upsample.h)
__global__ __launch_bounds__(256) KC_UP_ATTR void upsample_chain_kernel(const ChainProgram P, const UpsampleArgs U)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
#ifdef KC_UP_HARDWIRE
    upsample_chain_tile<K, T, KC_UP_RU, WIDE, 0u, HALF>(P, U, lds, UpHardwired<K, KC_UP_RU>{});
#else
    upsample_chain_tile<K, T, KC_UP_RU, WIDE, 0u, HALF>(P, U, lds, UpInterpreted<K, KC_UP_RU>{ P });
#endif
}

template <int T, bool WIDE, bool NTS, bool HALF>  // NTS: the resampled planes are stored nontemporal (cache_policy_mask)
__global__ __launch_bounds__(256) void upsample_kernel(const UpsamplePlanes P, const UpsampleArgs U)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    upsample_chain_tile<1, T, KC_UP_RU, WIDE, (NTS ? 0x100u : 0u), HALF>(P, U, lds, UpStore<KC_UP_RU>{});
}

template <int K, bool WIDE>
static hipError_t launch_upsample_chain_k(const ChainProgram &p, const UpsampleArgs &u, dim3 grid, size_t lds, hipStream_t s)
{
    const bool half = u.H.ratio == 2;
    switch (u.H.taps) {
    case 1:
        if (half) upsample_chain_kernel<K, 1, WIDE, true><<<grid, 256, lds, s>>>(p, u);
        else upsample_chain_kernel<K, 1, WIDE, false><<<grid, 256, lds, s>>>(p, u);
        break;
    case 3:
        if (half) upsample_chain_kernel<K, 3, WIDE, true><<<grid, 256, lds, s>>>(p, u);
        else upsample_chain_kernel<K, 3, WIDE, false><<<grid, 256, lds, s>>>(p, u);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_upsample_chain(const ChainProgram &p, int batch, const UpsampleArgs &u, hipStream_t s)
{
    if (u.H.n_out == 0 || u.V.n_out == 0) return hipSuccess;
    if (!upsample_args_ok(u, batch) || p.n_ops < 1 || p.n_ops > KC_CHAIN_MAX_OPS) return hipErrorInvalidValue;
    const size_t lds = upsample_lds_bytes(u);
    const dim3 grid = upsample_grid(u, batch);
    const bool wide = u.tile_w == 1024;
    switch (p.n_in) {
    case 1: return wide ? launch_upsample_chain_k<1, true>(p, u, grid, lds, s) : launch_upsample_chain_k<1, false>(p, u, grid, lds, s);
    case 2: return wide ? launch_upsample_chain_k<2, true>(p, u, grid, lds, s) : launch_upsample_chain_k<2, false>(p, u, grid, lds, s);
    case 3: return wide ? launch_upsample_chain_k<3, true>(p, u, grid, lds, s) : launch_upsample_chain_k<3, false>(p, u, grid, lds, s);
    case 4: return wide ? launch_upsample_chain_k<4, true>(p, u, grid, lds, s) : launch_upsample_chain_k<4, false>(p, u, grid, lds, s);
    default: return hipErrorInvalidValue;
    }
}

template <bool WIDE, bool NTS>
static hipError_t launch_upsample_w(const UpsamplePlanes &p, const UpsampleArgs &u, dim3 grid, size_t lds, hipStream_t s)
{
#define KC_UP_LAUNCH(T)                                                                 \
    do {                                                                               \
        if (u.H.ratio == 2) upsample_kernel<T, WIDE, NTS, true><<<grid, 256, lds, s>>>(p, u);  \
        else upsample_kernel<T, WIDE, NTS, false><<<grid, 256, lds, s>>>(p, u);        \
    } while (0)
    switch (u.H.taps) {
    case 1: KC_UP_LAUNCH(1); break;
    case 3: KC_UP_LAUNCH(3); break;
    case 5: KC_UP_LAUNCH(5); break;
    case 7: KC_UP_LAUNCH(7); break;
    default: return hipErrorInvalidValue;
    }
#undef KC_UP_LAUNCH
    return hipGetLastError();
}

hipError_t launch_upsample(const UpsamplePlanes &p, int batch, const UpsampleArgs &u, hipStream_t s)
{
    if (u.H.n_out == 0 || u.V.n_out == 0) return hipSuccess;
    if (!upsample_args_ok(u, batch)) return hipErrorInvalidValue;
    const size_t lds = upsample_lds_bytes(u);
    const dim3 grid = upsample_grid(u, batch);
    const bool nts = (p.nt_mask & 0x100u) != 0;
    if (u.tile_w == 1024) return nts ? launch_upsample_w<true, true>(p, u, grid, lds, s) : launch_upsample_w<true, false>(p, u, grid, lds, s);
    return nts ? launch_upsample_w<false, true>(p, u, grid, lds, s) : launch_upsample_w<false, false>(p, u, grid, lds, s);
}

}  // namespace kc
