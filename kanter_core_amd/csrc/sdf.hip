// Signed distance fields of cutout alpha (kc_image_distance_field, sdf.cpp): the header's rule as a separable exact Euclidean
// transform.  A texel within reach of the cap has |dx| <= S and |dy| <= S, so both passes look no further than S texels.
//
// sdf_columns_kernel: lanes sit on adjacent columns (a row of a wave is one 256-byte load), a thread owns one column of a band
// of KC_SDF_BAND rows.  Two running sweeps: down from the halo above the band, up from the halo below it; each keeps the
// distance to the last inside and the last outside texel seen, capped at S + 1, and a texel takes the one of the other class.
// The halo rows are only classified; the band's rows are loaded once, their classes kept as a 64-bit mask and the down
// sweep's distances as 64 bytes in 16 registers (every index is static once the loops are unrolled: no scratch), so the up
// sweep reads no memory inside the band and stores min(up, down) with the class bit: one 16-bit word per texel (SdfArgs).
// With KC_SDF_WRAP the halo rows are taken modulo the height; row y - k and row y + (h - k) are then the same row, seen at
// distance min(k, h - k) by one of the two sweeps, which is the torus distance.  A halo never exceeds h - 1 rows: beyond that
// every row has been seen at a smaller distance.
//
// sdf_rows_kernel: a workgroup stages KC_SDF_SEG words and a halo of S words either side of KC_SDF_ROWS rows in LDS (taken
// modulo the width with KC_SDF_WRAP; a word that does not exist is SDF_NONE), each as the column distance it offers a texel of
// either class -- g of a neighbour of the other class is 0 --, then every lane takes min(dx^2 + g(x +- dx)^2)
// going outwards and stops as soon as dx^2 reaches the best so far -- which
// starts at min(g(x)^2, cap), so dx never passes S.  The value rule in f64 (IEEE sqrt, divide and add), rounded to f32 once.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // ld_policy, st_policy, quant_u8: "inside" is the covered test of mip_coverage.hip

constexpr uint32_t SDF_NONE = 0x200u;   // a staged word beyond the image
constexpr uint32_t SDF_FAR = 1u << 12;  // its distance: its square is above every cap (254^2 + 255) and leaves room for dx^2

static __device__ __forceinline__ void sdf_step(bool in, uint32_t far, uint32_t &d_in, uint32_t &d_out)
{
    const uint32_t ni = min(d_in + 1u, far), no = min(d_out + 1u, far);
    d_in = in ? 0u : ni;
    d_out = in ? no : 0u;
}

template <bool NT, bool WRAP>
__global__ __launch_bounds__(256) void sdf_columns_kernel(const SdfArgs a)
{
    const uint32_t ntx = (a.w + KC_SDF_SEG - 1u) / KC_SDF_SEG;
    const uint32_t band = blockIdx.x / ntx;
    const uint32_t x = (blockIdx.x - band * ntx) * KC_SDF_SEG + threadIdx.x;
    if (x >= a.w) return;
    const uint32_t y0 = band * KC_SDF_BAND, rows = min(KC_SDF_BAND, a.h - y0), y1 = y0 + rows;
    const uint32_t far = a.spread + 1u, reach = min(a.spread, a.h - 1u);
    const float *col = a.src + x;
    const size_t pitch = a.src_pitch;

    // down: the halo above, then the band
    uint32_t d_in = far, d_out = far;
    {
        const uint32_t n = WRAP ? reach : min(reach, y0);
        uint32_t r = WRAP ? (y0 + a.h - n) % a.h : y0 - n;
#pragma unroll 8
        for (uint32_t k = 0; k < n; ++k) {
            sdf_step(quant_u8(ld_policy<NT>(col + r * pitch)) >= a.ref, far, d_in, d_out);
            r = r + 1u == a.h ? 0u : r + 1u;
        }
    }
    unsigned long long cls = 0ull;
    uint32_t up[KC_SDF_BAND / 4];
#pragma unroll
    for (uint32_t i = 0; i < KC_SDF_BAND / 4; ++i) up[i] = 0u;
#pragma unroll
    for (uint32_t i = 0; i < KC_SDF_BAND; ++i)  // rows past a short band load its last row again: no branch between the loads
        cls |= (unsigned long long)(quant_u8(ld_policy<NT>(col + min(y0 + i, y1 - 1u) * pitch)) >= a.ref ? 1u : 0u) << i;
#pragma unroll
    for (uint32_t i = 0; i < KC_SDF_BAND; ++i) {
        if (i < rows) {
            const bool in = (cls >> i) & 1ull;
            sdf_step(in, far, d_in, d_out);
            up[i >> 2] |= (in ? d_out : d_in) << (8u * (i & 3u));
        }
    }

    // up: the halo below, then the band from its last row
    d_in = far, d_out = far;
    {
        const uint32_t n = WRAP ? reach : min(reach, a.h - y1);
        uint32_t r = WRAP ? (y1 - 1u + n) % a.h : y1 - 1u + n;
#pragma unroll 8
        for (uint32_t k = 0; k < n; ++k) {
            sdf_step(quant_u8(ld_policy<NT>(col + r * pitch)) >= a.ref, far, d_in, d_out);
            r = r == 0u ? a.h - 1u : r - 1u;
        }
    }
    uint16_t *out = a.mid + x;
#pragma unroll
    for (uint32_t j = 0; j < KC_SDF_BAND; ++j) {
        const uint32_t i = KC_SDF_BAND - 1u - j;
        if (i < rows) {
            const bool in = (cls >> i) & 1ull;
            sdf_step(in, far, d_in, d_out);
            const uint32_t g = min(in ? d_out : d_in, (up[i >> 2] >> (8u * (i & 3u))) & 255u);
            out[(size_t)(y0 + i) * a.w] = (uint16_t)(g | (in ? 0x100u : 0u));
        }
    }
}

// The header's value rule on a capped squared distance
static __device__ __forceinline__ float sdf_value(uint32_t d2c, bool in, uint32_t spread, uint32_t cap)
{
    if (d2c >= cap) return in ? 1.0f : 0.0f;
    const double d = sqrt((double)d2c);
    const double sd = in ? d - 0.5 : 0.5 - d;
    return (float)(0.5 + sd / (2.0 * (double)spread));
}

// the column distance a staged word offers a texel of class c: 0 where the neighbour itself is of the other class
static __device__ __forceinline__ uint32_t sdf_offer(uint32_t t, uint32_t c)
{
    const uint32_t g = ((t >> 8) & 1u) == c ? (t & 255u) : 0u;
    return (t & SDF_NONE) ? SDF_FAR : g;
}

template <bool NT, bool WRAP>
__global__ __launch_bounds__(256) void sdf_rows_kernel(const SdfArgs a)
{
    // per row two images of the staged words: what each offers a texel of class 0 and of class 1 (sdf_offer), so that the scan
    // below is two reads, a minimum, a square and an add per step
    __shared__ uint16_t tile[KC_SDF_ROWS][2][KC_SDF_SEG + 2 * KC_SDF_MAX_SPREAD];
    const uint32_t ntx = (a.w + KC_SDF_SEG - 1u) / KC_SDF_SEG;
    const uint32_t ty = blockIdx.x / ntx;
    const uint32_t x0 = (blockIdx.x - ty * ntx) * KC_SDF_SEG, y0 = ty * KC_SDF_ROWS;
    const uint32_t rows = min(KC_SDF_ROWS, a.h - y0);
    const uint32_t reach = min(a.spread, a.w - 1u), span = KC_SDF_SEG + 2u * reach;
    const uint32_t first = WRAP ? (x0 + a.w - reach) % a.w : 0u;  // x0 - reach modulo the width
#pragma unroll
    for (uint32_t j = 0; j < KC_SDF_ROWS; ++j) {
        if (j < rows) {
            const uint16_t *row = a.mid + (size_t)(y0 + j) * a.w;
            for (uint32_t i = threadIdx.x; i < span; i += 256u) {
                uint32_t t;
                if constexpr (WRAP) {
                    t = row[(first + i) % a.w];
                } else {
                    const long long gx = (long long)x0 - (long long)reach + (long long)i;
                    t = (gx >= 0 && gx < (long long)a.w) ? (uint32_t)row[gx] : SDF_NONE;
                }
                tile[j][0][i] = (uint16_t)sdf_offer(t, 0u);
                tile[j][1][i] = (uint16_t)sdf_offer(t, 1u);
            }
        }
    }
    __syncthreads();
    const uint32_t x = x0 + threadIdx.x;
    if (x >= a.w) return;
    const uint32_t cap = a.spread * a.spread + a.spread + 1u;
#pragma unroll
    for (uint32_t j = 0; j < KC_SDF_ROWS; ++j) {
        if (j < rows) {
            // the texel's own word offers its class its distance (>= 1) and the other class 0
            const uint32_t own1 = tile[j][1][reach + threadIdx.x], g = own1 | tile[j][0][reach + threadIdx.x], c = own1 != 0u ? 1u : 0u;
            const uint16_t *mid = &tile[j][c][reach + threadIdx.x];
            uint32_t best = min(g * g, cap);
            for (uint32_t dx = 1; dx <= reach && dx * dx < best; ++dx) {
                const uint32_t o = min((uint32_t)*(mid - dx), (uint32_t)mid[dx]);
                best = min(best, dx * dx + o * o);
            }
            st_policy<NT>(a.dst + (size_t)(y0 + j) * a.dst_pitch + x, sdf_value(best, c != 0u, a.spread, cap));
        }
    }
}

hipError_t launch_sdf_columns(const SdfArgs &a, bool wrap, bool nt, hipStream_t s)
{
    const uint64_t groups = sdf_columns_groups(a.w, a.h);
    if (!a.src || !a.mid || a.w == 0 || a.h == 0 || groups > 0x7fffffffull || a.ref < 1 || a.ref > 255 || a.spread < 1 || a.spread > KC_SDF_MAX_SPREAD)
        return hipErrorInvalidValue;
#define KC_SDF(NT, WR) sdf_columns_kernel<NT, WR><<<dim3((uint32_t)groups), 256, 0, s>>>(a)
    if (nt) {
        if (wrap) KC_SDF(true, true);
        else KC_SDF(true, false);
    } else {
        if (wrap) KC_SDF(false, true);
        else KC_SDF(false, false);
    }
#undef KC_SDF
    return hipGetLastError();
}

hipError_t launch_sdf_rows(const SdfArgs &a, bool wrap, bool nt, hipStream_t s)
{
    const uint64_t groups = sdf_rows_groups(a.w, a.h);
    if (!a.mid || !a.dst || a.w == 0 || a.h == 0 || groups > 0x7fffffffull || a.spread < 1 || a.spread > KC_SDF_MAX_SPREAD) return hipErrorInvalidValue;
#define KC_SDF(NT, WR) sdf_rows_kernel<NT, WR><<<dim3((uint32_t)groups), 256, 0, s>>>(a)
    if (nt) {
        if (wrap) KC_SDF(true, true);
        else KC_SDF(true, false);
    } else {
        if (wrap) KC_SDF(false, true);
        else KC_SDF(false, false);
    }
#undef KC_SDF
    return hipGetLastError();
}

}  // namespace kc
