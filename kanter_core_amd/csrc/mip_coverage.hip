// Alpha-test coverage of mip chains (KC_MIP_COVERAGE, mip.cpp): the share of texels whose alpha passes a renderer's test stays
// what it was at level 0.  For that every level's alpha is scaled so that its T-th largest value lands on the reference, and the
// T-th largest of a plane is an exact selection: a radix select on the header's key (alpha clamped to [0, 1]; non-negative
// floats order as their bit patterns, 30 significant bits), three passes of 10 bits.  Each pass is one count launch over all
// levels of the chain, through a job table in the launch's arguments (kc_internal.hpp), and one pick launch; a scale launch
// writes the new planes.  Counts are integers: per-wave LDS histograms, flushed with vector atomics to one histogram per level,
// so the result does not depend on the launch shape or on the order of the atomics.  The planes are read again by every pass,
// so the loads carry no cache hint.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // hist_add, quant_u8

typedef float cv_f4 __attribute__((ext_vector_type(4)));

// The header's key: a clamped to [0, 1], NaN -> 1.0f, -0.0 and everything not greater than 0 -> +0.0f
static __device__ __forceinline__ uint32_t coverage_key(float a)
{
    float k = a > 0.0f ? a : 0.0f;  // NaN: 0 here
    k = k > 1.0f ? 1.0f : k;
    if (a != a) k = 1.0f;
    return __float_as_uint(k);
}

// The job of workgroup `wg`: first_wg rises with the level
static __device__ __forceinline__ uint32_t coverage_job_of(const CoverageArgs &a, uint32_t wg)
{
    uint32_t j = 0;
    while (j + 1u < a.levels && wg >= a.jobs[j + 1u].first_wg) ++j;
    return j;
}

__global__ __launch_bounds__(256) void coverage_count_kernel(const CoverageArgs a, uint32_t pass, uint32_t first_wg)
{
    __shared__ uint32_t hist[4 * KC_COVERAGE_BINS];  // per wave
    __shared__ uint32_t covered_wg;
    const uint32_t wg = first_wg + blockIdx.x;
    const uint32_t j = coverage_job_of(a, wg);
    const CoverageJob J = a.jobs[j];
    const bool select = j > 0u;  // level 0 is only counted
    uint32_t prefix = 0u;
    if (select && pass > 0u) {
        if (a.rec[j].done) return;  // uniform: the level keeps the plain alpha
        prefix = a.rec[j].prefix;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) hist[i * 256 + threadIdx.x] = 0u;
    if (threadIdx.x == 0) covered_wg = 0u;
    __syncthreads();
    uint32_t *wh = hist + (threadIdx.x >> 6) * KC_COVERAGE_BINS;
    // pass p bins bits [20 - 10 p, 30 - 10 p) of the keys whose bits above them equal the prefix (pass 0: bits 30, 31 are 0, as
    // is the zeroed record's prefix)
    const uint32_t shift = 20u - 10u * pass;
    const uint32_t rb = __float_as_uint(a.r_b);
    const uint32_t row_units = (J.w + 3u) / 4u, total = row_units * J.h, stride = J.wgs * 256u;
    uint32_t covered = 0u;
    // two quads per trip, both loads first: a level has few workgroups (coverage_job_wgs), so each thread keeps two loads in flight
    for (uint32_t idx = (wg - J.first_wg) * 256u + threadIdx.x; idx < total; idx += 2u * stride) {
        const bool two = idx + stride < total;
        const uint32_t idx1 = two ? idx + stride : idx;
        const uint32_t y0 = idx / row_units, q0 = idx - y0 * row_units, y1 = idx1 / row_units, q1 = idx1 - y1 * row_units;
        const cv_f4 v[2] = { *reinterpret_cast<const cv_f4 *>(J.src + (size_t)y0 * J.src_pitch + 4u * q0),
                             *reinterpret_cast<const cv_f4 *>(J.src + (size_t)y1 * J.src_pitch + 4u * q1) };
        // texels of each quad inside its row: the rest is padding, never counted
        const uint32_t valid[2] = { min(J.w - 4u * q0, 4u), two ? min(J.w - 4u * q1, 4u) : 0u };
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const uint32_t key = coverage_key(v[u][p]);
                const bool in = p < (int)valid[u];
                covered += (in && key >= rb) ? 1u : 0u;
                if (select) hist_add(wh, (key >> shift) & (KC_COVERAGE_BINS - 1u), in && (key >> (shift + 10u)) == prefix);
            }
    }
    if (pass == 0u) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) covered += (uint32_t)__shfl_xor((int)covered, off);
        if ((threadIdx.x & 63u) == 0u && covered) atomicAdd(&covered_wg, covered);
    }
    __syncthreads();
    if (pass == 0u && threadIdx.x == 0 && covered_wg) atomicAdd(&a.rec[j].plain_covered, (unsigned long long)covered_wg);
    if (select) {
        uint32_t *gh = a.hist + (size_t)j * KC_COVERAGE_BINS;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t b = (uint32_t)i * 256u + threadIdx.x;
            const uint32_t n = hist[b] + hist[KC_COVERAGE_BINS + b] + hist[2u * KC_COVERAGE_BINS + b] + hist[3u * KC_COVERAGE_BINS + b];
            if (n) atomicAdd(&gh[b], n);
        }
    }
}

// kc_mip_coverage_scale on the device: the same three operations (the build's IEEE divide, nothing fused) and the same loop
static __device__ __forceinline__ float coverage_scale(float v, float r_b, uint32_t ref)
{
    const float ve = v > 0x1p-16f ? v : 0x1p-16f;
    float s = r_b / ve;
    while (quant_u8(ve * s) < ref) s = __uint_as_float(__float_as_uint(s) + 1u);  // s > 0 and finite: the next f32 above it
    return s;
}

// One workgroup per level.  The level's histogram holds the counts of the pass; thread t owns bins 4 t .. 4 t + 3.
__global__ __launch_bounds__(256) void coverage_pick_kernel(const CoverageArgs a, uint32_t pass)
{
    __shared__ uint32_t part[256];
    const uint32_t k = blockIdx.x, t = threadIdx.x;
    CoverageRecord *R = a.rec + k;
    const unsigned long long n_k = (unsigned long long)a.jobs[k].w * a.jobs[k].h;
    if (k == 0u) {  // level 0 is the image: C_0 in both counts
        if (pass == 0u && t == 0u) {
            R->texels = n_k;
            R->target = R->plain_covered;
            R->scale = 1.0f;
            R->done = 1u;
        }
        return;
    }
    if (pass > 0u && R->done) return;
    uint32_t rank = R->rank;
    if (pass == 0u) {
        const unsigned long long n_0 = (unsigned long long)a.jobs[0].w * a.jobs[0].h, c_0 = a.rec[0].plain_covered;
        unsigned long long target = 0ull;
        if (c_0) {
            target = (c_0 * n_k + n_0 / 2ull) / n_0;  // c_0, n_0 <= 2^31 and n_k <= 2^29: exact in 64 bits
            target = target < 1ull ? 1ull : target;
            target = target > n_k ? n_k : target;
        }
        const bool plain = target == 0ull || R->plain_covered == target;
        __syncthreads();  // everyone has read the record
        if (t == 0u) {
            R->texels = n_k;
            R->target = target;
            if (plain) {
                R->scale = 1.0f;
                R->done = 1u;
            }
        }
        if (plain) return;
        rank = (uint32_t)target;
    }
    uint32_t *gh = a.hist + (size_t)k * KC_COVERAGE_BINS + 4u * t;
    uint32_t n[4], mine = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        n[i] = gh[i];
        gh[i] = 0u;  // for the next pass
        mine += n[i];
    }
    part[t] = mine;
    __syncthreads();
    uint32_t above = 0u;  // the texels of this pass in the bins above this thread's
    for (uint32_t u = t + 1u; u < 256u; ++u) above += part[u];
    // the one bin with above < rank <= above + n: the rank is at most the texels the pass counted
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        if (above < rank && rank <= above + n[i]) {
            const uint32_t prefix = (R->prefix << 10) | (4u * t + (uint32_t)i);
            R->prefix = prefix;
            R->rank = rank - above;
            if (pass == 2u) {
                const float v = __uint_as_float(prefix);
                R->v = v;
                R->scale = coverage_scale(v, a.r_b, a.ref);
                R->done = 1u;
            }
        }
        above += n[i];
    }
}

// d = p * s, one f32 multiplication, nothing clamped; a level with s == 1 is copied.  One thread per quad, the tail of a row
// texel by texel.
__global__ __launch_bounds__(256) void coverage_scale_kernel(const CoverageArgs a, uint32_t first_wg)
{
    const uint32_t wg = first_wg + blockIdx.x;
    const uint32_t j = coverage_job_of(a, wg);
    const CoverageJob J = a.jobs[j];
    const float s = a.rec[j].scale;
    const bool copy = s == 1.0f;
    const uint32_t row_units = (J.w + 3u) / 4u, total = row_units * J.h, stride = J.wgs * 256u;
    for (uint32_t idx = (wg - J.first_wg) * 256u + threadIdx.x; idx < total; idx += stride) {
        const uint32_t y = idx / row_units, q = idx - y * row_units;
        const float *src = J.src + (size_t)y * J.src_pitch + 4u * q;
        float *dst = J.dst + (size_t)y * J.dst_pitch + 4u * q;
        if (4u * q + 3u < J.w) {
            const cv_f4 p = *reinterpret_cast<const cv_f4 *>(src);
            *reinterpret_cast<cv_f4 *>(dst) = copy ? p : p * s;
        } else {
            for (uint32_t x = 0; 4u * q + x < J.w; ++x) dst[x] = copy ? src[x] : src[x] * s;
        }
    }
}

static bool coverage_args_ok(const CoverageArgs &a)
{
    return a.rec && a.hist && a.levels >= 1 && a.levels <= KC_COVERAGE_MAX_LEVELS && a.ref >= 1 && a.ref <= 255;
}

hipError_t launch_coverage_count(const CoverageArgs &a, uint32_t pass, uint32_t first_wg, uint32_t wgs, hipStream_t s)
{
    if (!coverage_args_ok(a) || pass > 2 || wgs == 0 || wgs > 0x7fffffffu - first_wg) return hipErrorInvalidValue;
    coverage_count_kernel<<<dim3(wgs), 256, 0, s>>>(a, pass, first_wg);
    return hipGetLastError();
}

hipError_t launch_coverage_pick(const CoverageArgs &a, uint32_t pass, hipStream_t s)
{
    if (!coverage_args_ok(a) || pass > 2) return hipErrorInvalidValue;
    coverage_pick_kernel<<<dim3(a.levels), 256, 0, s>>>(a, pass);
    return hipGetLastError();
}

hipError_t launch_coverage_scale(const CoverageArgs &a, uint32_t first_wg, uint32_t wgs, hipStream_t s)
{
    if (!coverage_args_ok(a) || a.levels < 2 || first_wg == 0 || wgs == 0 || wgs > 0x7fffffffu - first_wg) return hipErrorInvalidValue;
    coverage_scale_kernel<<<dim3(wgs), 256, 0, s>>>(a, first_wg);
    return hipGetLastError();
}

}  // namespace kc
