// Per-channel min, max, NaN count and u8 histograms of an image's planes (kc_image_channel_stats, stats.cpp).  A read-only
// streaming reduction in the form of the other streaming kernels: one launch covers the image's distinct resident planes (1-4
// "slots", each a pointer and a pitch), a grid-stride loop over pixel quads with 16-byte loads and the launch's cache policy, the
// last quad of a row masked.  Each workgroup leaves one partial record; channel_stats_combine_kernel sums the records into the
// result.  Everything is an integer (order keys, counts), so the result does not depend on the order of the summation.
//
// Partial record of a workgroup (rec_words u32): [0..3] min key of slot 0..3, [4..7] max key, [8..11] NaN count, [12..15]
// unused, then with HIST 256 bin counts per slot.  The result holds the same words as u64, summed / min'd / max'd over the records.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // ld_policy, hist_add, quant_u8 / quant_u8_srgb: the bins are what the u8 exports write

typedef float st_f4 __attribute__((ext_vector_type(4)));

// The total order of the non-NaN floats (-0.0 < +0.0, infinities included) as unsigned integers
static __device__ __forceinline__ uint32_t order_key(uint32_t b) { return (b >> 31) ? ~b : (b | 0x80000000u); }
static __device__ __forceinline__ bool nan_bits(uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u; }

template <int N, bool NT, bool HIST, bool SRGB>
static __device__ __forceinline__ void stats_quads(const StatsArgs &a, uint32_t *wh, const uint32_t *T, uint32_t (&kmin)[4],
                                                   uint32_t (&kmax)[4], uint32_t (&nan)[4])
{
    const uint32_t row_units = (a.w + 3) / 4;
    const uint32_t total = row_units * a.h;
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        const uint32_t y = idx / row_units;
        const uint32_t q = idx - y * row_units;
        const uint32_t valid = min(a.w - 4 * q, 4u);  // pixels of the quad inside the row: the rest is padding, never counted
        st_f4 v[N];
#pragma unroll
        for (int s = 0; s < N; ++s) v[s] = ld_policy<NT>(reinterpret_cast<const st_f4 *>(a.ptr[s] + (size_t)y * a.pitch[s] + 4 * q));
#pragma unroll
        for (int s = 0; s < N; ++s)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const uint32_t bits = __float_as_uint(v[s][p]);
                const bool in = p < (int)valid, nn = nan_bits(bits);
                nan[s] += (in && nn) ? 1u : 0u;
                const uint32_t k = order_key(bits);
                kmin[s] = min(kmin[s], (in && !nn) ? k : 0xffffffffu);
                kmax[s] = max(kmax[s], (in && !nn) ? k : 0u);
            }
        if constexpr (HIST) {
#pragma unroll
            for (int s = 0; s < N; ++s) {
                const bool srgb_q = SRGB && ((a.srgb >> s) & 1u);
#pragma unroll
                for (int p = 0; p < 4; ++p) hist_add(wh + s * 256, srgb_q ? quant_u8_srgb(v[s][p], T) : quant_u8(v[s][p]), p < (int)valid);
            }
        }
    }
}

template <bool NT, bool HIST, bool SRGB>
__global__ __launch_bounds__(256) void channel_stats_kernel(const StatsArgs a)
{
    __shared__ uint32_t hist[HIST ? 4 * 4 * 256 : 1];  // per wave: 4 slots x 256 bins
    __shared__ uint32_t srgb_t[SRGB ? 257 : 1];
    __shared__ uint32_t red[4][12];  // per wave: min keys, max keys, NaN counts of the 4 slots
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if constexpr (HIST) {
#pragma unroll
        for (int i = 0; i < 16; ++i) hist[i * 256 + threadIdx.x] = 0u;
    }
    if constexpr (SRGB) {
        srgb_t[threadIdx.x] = kSrgbThresholdBits[threadIdx.x];  // 256 threads, as image_export_kernel stages it
        if (threadIdx.x == 0) srgb_t[256] = 0xffffffffu;         // sentinel: nothing is >= it
    }
    if (blockIdx.x == 0)  // the identities the combine kernel's atomics start from (it runs after this launch)
        for (uint32_t i = threadIdx.x; i < a.rec_words; i += 256u) a.result[i] = i < 4 ? 0xffffffffull : 0ull;
    if constexpr (HIST || SRGB) __syncthreads();
    uint32_t kmin[4] = { 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu }, kmax[4] = { 0u, 0u, 0u, 0u }, nan[4] = { 0u, 0u, 0u, 0u };
    uint32_t *wh = hist + (HIST ? wave * 1024u : 0u);
    switch (a.n) {
    case 1: stats_quads<1, NT, HIST, SRGB>(a, wh, srgb_t, kmin, kmax, nan); break;
    case 2: stats_quads<2, NT, HIST, SRGB>(a, wh, srgb_t, kmin, kmax, nan); break;
    case 3: stats_quads<3, NT, HIST, SRGB>(a, wh, srgb_t, kmin, kmax, nan); break;
    default: stats_quads<4, NT, HIST, SRGB>(a, wh, srgb_t, kmin, kmax, nan); break;
    }
    // the wave, then the workgroup's four waves
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (s >= (int)a.n) break;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            kmin[s] = min(kmin[s], (uint32_t)__shfl_xor((int)kmin[s], off));
            kmax[s] = max(kmax[s], (uint32_t)__shfl_xor((int)kmax[s], off));
            nan[s] += (uint32_t)__shfl_xor((int)nan[s], off);
        }
        if (lane == 0) red[wave][s] = kmin[s], red[wave][4 + s] = kmax[s], red[wave][8 + s] = nan[s];
    }
    __syncthreads();
    uint32_t *rec = a.partials + (size_t)blockIdx.x * a.rec_words;
    if (threadIdx.x < 12 && (threadIdx.x & 3) < a.n) {
        const uint32_t t = threadIdx.x;
        uint32_t r = red[0][t];
        for (int w = 1; w < 4; ++w) r = t < 4 ? min(r, red[w][t]) : t < 8 ? max(r, red[w][t]) : r + red[w][t];
        rec[t] = r;
    }
    if constexpr (HIST) {
        for (uint32_t s = 0; s < a.n; ++s) {
            const uint32_t i = s * 256u + threadIdx.x;
            rec[16u + i] = hist[i] + hist[1024u + i] + hist[2048u + i] + hist[3072u + i];
        }
    }
}

// Sums the records: blockIdx.x = 64 result words, blockIdx.y = a run of rows (records); four rows at a time per column, then one
// atomic per column and block into the result.
constexpr uint32_t KC_STATS_COMBINE_ROWS = 64;
__global__ __launch_bounds__(256) void channel_stats_combine_kernel(const uint32_t *partials, uint32_t groups, uint32_t rec_words,
                                                                    unsigned long long *result)
{
    __shared__ unsigned long long red[4][64];
    const uint32_t lane = threadIdx.x & 63, sub = threadIdx.x >> 6;
    const uint32_t col = blockIdx.x * 64u + lane;
    const uint32_t r0 = blockIdx.y * KC_STATS_COMBINE_ROWS, r1 = min(groups, r0 + KC_STATS_COMBINE_ROWS);
    const int kind = col < 4 ? 0 : col < 8 ? 1 : (col < 12 || col >= 16) ? 2 : 3;  // min, max, sum, unused
    const bool used = col < rec_words && kind != 3;
    unsigned long long acc = kind == 0 ? 0xffffffffull : 0ull;
    if (used)
        for (uint32_t r = r0 + sub; r < r1; r += 4) {
            const unsigned long long v = partials[(size_t)r * rec_words + col];
            acc = kind == 0 ? (v < acc ? v : acc) : kind == 1 ? (v > acc ? v : acc) : acc + v;
        }
    red[sub][lane] = acc;
    __syncthreads();
    if (sub == 0 && used) {
        for (int k = 1; k < 4; ++k) {
            const unsigned long long v = red[k][lane];
            acc = kind == 0 ? (v < acc ? v : acc) : kind == 1 ? (v > acc ? v : acc) : acc + v;
        }
        if (kind == 0) atomicMin(result + col, acc);
        else if (kind == 1) atomicMax(result + col, acc);
        else atomicAdd(result + col, acc);
    }
}

// Workgroups of a launch: as many as stay resident at once on the device's CUs (the kernel is a stream: it needs loads in
// flight, not a large grid), no more than the quads need; the tune_cap option overrides.
uint32_t channel_stats_groups(uint32_t w, uint32_t h, bool hist, bool srgb, uint32_t cus)
{
    static int resident[3] = { 0, 0, 0 };  // per form; the cache-policy variants use the same resources
    int &r = resident[hist ? (srgb ? 2 : 1) : 0];
    if (r == 0) {
        hipError_t e = !hist ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&r, channel_stats_kernel<false, false, false>, 256, 0)
                       : !srgb ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&r, channel_stats_kernel<false, true, false>, 256, 0)
                               : hipOccupancyMaxActiveBlocksPerMultiprocessor(&r, channel_stats_kernel<false, true, true>, 256, 0);
        if (e != hipSuccess || r < 1) {
            (void)hipGetLastError();
            r = 4;
        }
    }
    const uint64_t quads = (uint64_t)((w + 3) / 4) * h;
    uint64_t groups = std::min<uint64_t>((quads + 255) / 256, grid_cap((uint64_t)r * cus));
    return (uint32_t)std::max<uint64_t>(groups, 1);
}

hipError_t launch_channel_stats(const StatsArgs &a, bool hist, bool srgb, bool nt, uint32_t groups, hipStream_t s)
{
    if (groups == 0 || a.n < 1 || a.n > 4) return hipErrorInvalidValue;
    if (srgb && !hist) return hipErrorInvalidValue;
#define KC_STATS(NT, H, SR) channel_stats_kernel<NT, H, SR><<<dim3(groups), 256, 0, s>>>(a)
    if (!hist) {
        if (nt) KC_STATS(true, false, false);
        else KC_STATS(false, false, false);
    } else if (!srgb) {
        if (nt) KC_STATS(true, true, false);
        else KC_STATS(false, true, false);
    } else {
        if (nt) KC_STATS(true, true, true);
        else KC_STATS(false, true, true);
    }
#undef KC_STATS
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 cgrid((a.rec_words + 63) / 64, (groups + KC_STATS_COMBINE_ROWS - 1) / KC_STATS_COMBINE_ROWS);
    channel_stats_combine_kernel<<<cgrid, 256, 0, s>>>(a.partials, groups, a.rec_words, a.result);
    return hipGetLastError();
}

}  // namespace kc
