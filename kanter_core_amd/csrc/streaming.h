// What the streaming kernels share -- u8.hip (to_u8, from_u8), h2n.hip (height_to_normal), devimage.hip (device-memory images),
// stats.hip, mip_coverage.hip, bc.hip, and chain.hip for the policy loads / stores: the grid cap of their grid-stride loops, loads /
// stores with a launch's cache policy, the wave histogram step and the two 8-bit quantisers.
// Included inside namespace kc by each unit; every definition is static, each unit keeps its own copy.
#pragma once

// Grid cap of the grid-stride streaming kernels (to_u8, from_u8, height_to_normal); the tune_cap option overrides (tuning).
// Default: no cap, one quad / pixel per thread -- from_u8 58.1 -> 50.4 us, height_to_normal 56.8 -> 55.4 us at 4096^2
// against 8192 workgroups looping twice (profiles/r02_kernel_times.txt); to_u8 does not care.
[[maybe_unused]] static uint64_t grid_cap(uint64_t dflt)  // (chain.hip takes its grid from the caller)
{
    const int cap = options().tune_cap;
    return cap > 0 ? (uint64_t)cap : dflt;
}

// Loads / stores with the launch's cache policy (ChainProgram::nt_mask; runtime.cpp, cache_policy_mask) as a compile-time
// property: NT = the stream does not fit the Infinity Cache and is marked nontemporal.
template <bool NT, class V>
static __device__ __forceinline__ V ld_policy(const V *p)
{
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT, class V>
static __device__ __forceinline__ void st_policy(V *p, V v)
{
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// One pixel of every lane into the wave's LDS histogram `wh` (stats.hip, mip_coverage.hip): bin b, counted where `in`.  When every counted pixel of the wave falls in one bin (a mask that is
// mostly 0, values clamped to 0 or 1), one lane adds the wave's count: 64 lanes on one LDS address would serialise the atomics.
static __device__ __forceinline__ void hist_add(uint32_t *wh, uint32_t b, bool in)
{
    const uint32_t b0 = __builtin_amdgcn_readfirstlane(b);  // may be a pixel past the row's end: it only picks the path
    if (__ballot(in && b != b0) == 0) {
        const uint32_t cnt = (uint32_t)__popcll(__ballot(in));
        if (__lane_id() == __builtin_ctzll(__ballot(1))) atomicAdd(&wh[b0], cnt);
    } else if (in) {
        atomicAdd(&wh[b], 1u);
    }
}

// ------------------------------------------------------------------------------------------
// u8 boundary.  to_u8 / to_u8_srgb: src/slot_image.rs:141-207, srgb_to_linear:
// src/slot_data.rs:100-109.  ((v.clamp(0,1) * 255.).min(255.)) as u8: truncation, NaN -> 255.
// ------------------------------------------------------------------------------------------
static __device__ __forceinline__ uint32_t quant_u8(float v)
{
    float x = v;
    if (x < 0.0f) x = 0.0f;
    if (x > 1.0f) x = 1.0f;  // NaN falls through both
    x = x * 255.0f;
    if (!(x <= 255.0f)) x = 255.0f;  // f32::min(255.): NaN -> 255
    return (uint32_t)x;               // 0 <= x <= 255: truncation
}

// to_u8_srgb as a step function.  q(x) = ((srgb_to_linear(x.clamp(0, 1)) * 255.).min(255.)) as u8 is non-decreasing in x, so
// q(x) = #{v : x >= T[v]} with T[v] the smallest float that exports as >= v.  The table (srgb_thresholds.inc) is generated
// with libm's powf -- what the reference's f32::powf calls -- and the identity is checked there for every float in [0, 1]
// (tools/gen_srgb_thresholds.c), so this form returns exactly what the reference's power does, without computing one: a
// hardware log2 / exp2 estimate lands within a level of the answer and two table comparisons settle it.
#include "srgb_thresholds.inc"

static __device__ __forceinline__ uint32_t quant_u8_srgb(float v, const uint32_t *T)
{
    float x = v;
    if (x < 0.0f) x = 0.0f;
    if (x > 1.0f) x = 1.0f;
    if (x != x) return 255u;  // NaN survives the clamp and the power; f32::min(255.) then returns 255
    const uint32_t xb = __float_as_uint(x);  // non-negative floats order like their bit patterns
    if ((int32_t)xb <= 0) return 0u;         // +0.0, and -0.0 (which passes the clamp): srgb_to_linear returns s itself
    const float est = 255.0f * __builtin_amdgcn_exp2f(2.4f * __builtin_amdgcn_logf((x + 0.055f) * (1.0f / 1.055f)));
    // The estimate is within one level of the answer for every float in [0, 1] (checked exhaustively on the device by
    // profiles/srgb_exhaustive.py: all 1 065 353 217 of them through this kernel against the table's definition), so one
    // comparison each way settles it: no data-dependent loop.  T[0] = 0 and the sentinel T[256] = 0xffffffff keep the
    // look-ups inside the table at both ends.
    const uint32_t q = xb < T[1] ? 0u : (uint32_t)fminf(est, 255.0f);
    return q + (xb >= T[q + 1u] ? 1u : 0u) - (xb < T[q] ? 1u : 0u);
}
