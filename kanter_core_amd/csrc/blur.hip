// Separable Gaussian blur (kc_image_blur, blur.cpp): the header's texel rule along one axis, for every selected plane of an image
// in one launch (blockIdx.y is the plane).  Both kernels stage their taps in LDS with the clamp or the modulo applied while
// staging, so the tap loop has no edge logic, and run the rule in its own order -- the outermost pair first, every operation
// rounded on its own (the build's -ffp-contract=off) -- on four independent texels per lane; going from pair k to pair k - 1
// moves each texel's two taps one step inwards, so four adjacent texels share all but two of their taps: a lane keeps the two
// windows of four in registers and reads two new values per pair, 2 R + 6 reads for four texels.  The weights are read from the
// argument block with a wave-uniform index: scalar loads.
//
// blur_rows_kernel: a wave per row, a lane per four adjacent texels of a segment of KC_BLUR_SEG: its own quad comes with one
// 16-byte load, the two halos of R and a row's last, partial quad with 4-byte loads through the edge rule.  A row's KC_BLUR_SEG + 2 R
// staged floats are dealt out by index modulo 4 into four sub-arrays of BLUR_SUB floats, so the read of tap u by every lane --
// element 4 lane + u -- is a run of 64 consecutive floats of one sub-array (no bank conflict; side by side they would be 16 bytes
// apart, four lanes to a bank), and BLUR_SUB % 32 == 8 spreads the 32 consecutive elements a staging store writes over 32 banks.
//
// blur_columns_kernel: a lane per four adjacent columns (one float4 of a row, 16 lanes per 256-byte row of the tile) of four
// adjacent rows of a band of KC_BLUR_BAND; the tile is KC_BLUR_BAND + 2 R rows of KC_BLUR_COLS floats, 48 KiB at R = 64: three
// workgroups per CU.  Rows are 64 banks long, so the 16-byte reads of a lane group -- parts of two rows -- never meet on a bank.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // ld_policy, st_policy

constexpr uint32_t BLUR_SUB = (KC_BLUR_SEG + 2u * KC_BLUR_MAX_RADIUS) / 4u + 8u;
static_assert(BLUR_SUB % 32u == 8u && KC_BLUR_SEG == 256u && KC_BLUR_ROWS == 4u, "blur_rows_kernel: a wave per row, a lane per quad");
static_assert(KC_BLUR_COLS == 64u && KC_BLUR_BAND == 64u, "blur_columns_kernel: 16 x 16 lanes of 4 x 4 texels");

typedef float blur_f4 __attribute__((ext_vector_type(4)));  // four adjacent texels of a row; arithmetic on it is elementwise

// position `i` of an axis of n texels as staged slot e sees it: i = start - R + e, clamped, or first + e modulo n
template <bool WRAP>
static __device__ __forceinline__ uint32_t blur_tap_index(uint32_t start, uint32_t first, uint32_t R, uint32_t e, uint32_t n)
{
    if constexpr (WRAP) {
        return (first + e) % n;
    } else {
        const long long g = (long long)start - (long long)R + (long long)e;
        return g < 0 ? 0u : (g >= (long long)n ? n - 1u : (uint32_t)g);
    }
}

template <bool NT, bool WRAP>
__global__ __launch_bounds__(256) void blur_rows_kernel(const BlurArgs a)
{
    __shared__ float tile[KC_BLUR_ROWS][4u * BLUR_SUB];
    const uint32_t ntx = (a.w + KC_BLUR_SEG - 1u) / KC_BLUR_SEG;
    const uint32_t ty = blockIdx.x / ntx;
    const uint32_t x0 = (blockIdx.x - ty * ntx) * KC_BLUR_SEG;
    const uint32_t j = threadIdx.x >> 6, lane = threadIdx.x & 63u, pl = blockIdx.y;
    const uint32_t y = ty * KC_BLUR_ROWS + j;
    const uint32_t R = a.radius;
    const float *row = a.src[pl] + (size_t)min(y, a.h - 1u) * a.src_pitch[pl];  // a wave past the last row stages it again
    float *s = tile[j];
    const uint32_t first = WRAP ? (x0 + a.w - R % a.w) % a.w : 0u;  // x0 - R modulo the width
    auto put = [&](uint32_t e, float v) { s[(e & 3u) * BLUR_SUB + (e >> 2)] = v; };
    // the segment's own texels, elements R + 4 lane + i: one 16-byte load where the whole quad lies in the row, the general
    // index otherwise (the row's last quad, and what the clamp or the modulo supplies beyond the width)
    const uint32_t x = x0 + 4u * lane;
    if (x + 3u < a.w) {
        const blur_f4 v = ld_policy<NT>((const blur_f4 *)(row + x));
        put(R + 4u * lane, v.x), put(R + 4u * lane + 1u, v.y), put(R + 4u * lane + 2u, v.z), put(R + 4u * lane + 3u, v.w);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) put(R + 4u * lane + i, ld_policy<NT>(row + blur_tap_index<WRAP>(x0, first, R, R + 4u * lane + i, a.w)));
    }
    for (uint32_t t = lane; t < 2u * R; t += 64u) {  // the two halos: elements 0..R-1 and R + SEG..2 R + SEG - 1
        const uint32_t e = t < R ? t : t + KC_BLUR_SEG;
        put(e, ld_policy<NT>(row + blur_tap_index<WRAP>(x0, first, R, e, a.w)));
    }
    __syncthreads();
    if (x >= a.w || y >= a.h) return;
    // tap j of texel i of the lane is staged element 4 lane + u, u = i + R + j
    auto ld = [&](uint32_t u) { return s[(u & 3u) * BLUR_SUB + (u >> 2) + lane]; };
    float l0 = ld(0u), l1 = ld(1u), l2 = ld(2u), l3 = ld(3u);
    float r0 = ld(2u * R), r1 = ld(2u * R + 1u), r2 = ld(2u * R + 2u), r3 = ld(2u * R + 3u);
    float wk = a.weights[R];
    float acc0 = wk * (l0 + r0), acc1 = wk * (l1 + r1), acc2 = wk * (l2 + r2), acc3 = wk * (l3 + r3);
#pragma unroll 4
    for (uint32_t k = R - 1u; k >= 1u; --k) {
        l0 = l1, l1 = l2, l2 = l3, l3 = ld(R - k + 3u);
        r3 = r2, r2 = r1, r1 = r0, r0 = ld(R + k);
        wk = a.weights[k];
        acc0 = acc0 + wk * (l0 + r0);
        acc1 = acc1 + wk * (l1 + r1);
        acc2 = acc2 + wk * (l2 + r2);
        acc3 = acc3 + wk * (l3 + r3);
    }
    // the windows stand at k = 1: l_i is element i + R - 1 and r_i element i + R + 1, so the four centres are l1, l2, l3, r2
    wk = a.weights[0];
    acc0 = acc0 + wk * l1;
    acc1 = acc1 + wk * l2;
    acc2 = acc2 + wk * l3;
    acc3 = acc3 + wk * r2;
    float *o = a.dst[pl] + (size_t)y * a.dst_pitch[pl] + x;
    if (x + 3u < a.w) {
        *(blur_f4 *)o = blur_f4{ acc0, acc1, acc2, acc3 };
    } else {
        o[0] = acc0;
        if (x + 1u < a.w) o[1] = acc1;
        if (x + 2u < a.w) o[2] = acc2;
    }
}

template <bool NT, bool WRAP>
__global__ __launch_bounds__(256) void blur_columns_kernel(const BlurArgs a)
{
    extern __shared__ blur_f4 band_tile[];  // rows of KC_BLUR_COLS / 4 quads
    constexpr uint32_t Q = KC_BLUR_COLS / 4u;
    const uint32_t ntx = (a.w + KC_BLUR_COLS - 1u) / KC_BLUR_COLS;
    const uint32_t band = blockIdx.x / ntx;
    const uint32_t x0 = (blockIdx.x - band * ntx) * KC_BLUR_COLS, y0 = band * KC_BLUR_BAND;
    const uint32_t tx = threadIdx.x & (Q - 1u), tr = threadIdx.x / Q, pl = blockIdx.y;
    const uint32_t x = x0 + 4u * tx, R = a.radius;
    // a short last band stages what its rows, rounded up to a lane's four, read
    const uint32_t staged = min(KC_BLUR_BAND, (a.h - y0 + 3u) & ~3u) + 2u * R;
    const uint32_t first = WRAP ? (y0 + a.h - R % a.h) % a.h : 0u;  // y0 - R modulo the height
    if (x < a.w) {
        const float *col = a.src[pl] + x;
        const size_t pitch = a.src_pitch[pl];
        for (uint32_t r = tr; r < staged; r += 256u / Q) {
            const float *p = col + blur_tap_index<WRAP>(y0, first, R, r, a.h) * pitch;
            blur_f4 v;
            if (x + 3u < a.w) {
                v = *(const blur_f4 *)p;
            } else {  // the last quad of a row: nothing beyond the width is read
                v = blur_f4{ p[0], 0.0f, 0.0f, 0.0f };
                if (x + 1u < a.w) v.y = p[1];
                if (x + 2u < a.w) v.z = p[2];
            }
            band_tile[r * Q + tx] = v;
        }
    }
    __syncthreads();
    const uint32_t o = 4u * tr;  // the lane's first row in the band
    if (x >= a.w || y0 + o >= a.h) return;
    // tap j of row o + i is staged row o + u, u = i + R + j
    auto ld = [&](uint32_t u) { return band_tile[(o + u) * Q + tx]; };
    blur_f4 l0 = ld(0u), l1 = ld(1u), l2 = ld(2u), l3 = ld(3u);
    blur_f4 r0 = ld(2u * R), r1 = ld(2u * R + 1u), r2 = ld(2u * R + 2u), r3 = ld(2u * R + 3u);
    float wk = a.weights[R];
    blur_f4 acc0 = wk * (l0 + r0), acc1 = wk * (l1 + r1), acc2 = wk * (l2 + r2), acc3 = wk * (l3 + r3);
#pragma unroll 4
    for (uint32_t k = R - 1u; k >= 1u; --k) {
        l0 = l1, l1 = l2, l2 = l3, l3 = ld(R - k + 3u);
        r3 = r2, r2 = r1, r1 = r0, r0 = ld(R + k);
        wk = a.weights[k];
        acc0 = acc0 + wk * (l0 + r0);
        acc1 = acc1 + wk * (l1 + r1);
        acc2 = acc2 + wk * (l2 + r2);
        acc3 = acc3 + wk * (l3 + r3);
    }
    wk = a.weights[0];  // the centres, as in the rows kernel
    const blur_f4 out[4] = { acc0 + wk * l1, acc1 + wk * l2, acc2 + wk * l3, acc3 + wk * r2 };
    float *dst = a.dst[pl] + x;
    const size_t pitch = a.dst_pitch[pl];
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const uint32_t y = y0 + o + i;
        if (y < a.h) {
            float *p = dst + y * pitch;
            if (x + 3u < a.w) {
                st_policy<NT>((blur_f4 *)p, out[i]);
            } else {
                st_policy<NT>(p, out[i].x);
                if (x + 1u < a.w) st_policy<NT>(p + 1, out[i].y);
                if (x + 2u < a.w) st_policy<NT>(p + 2, out[i].z);
            }
        }
    }
}

// what both launchers ask of an argument block: planes in range, every row 16-byte aligned, a radius the tiles were sized for
static bool blur_args_ok(const BlurArgs &a)
{
    if (a.w == 0 || a.h == 0 || a.radius < 1 || a.radius > KC_BLUR_MAX_RADIUS || a.planes < 1 || a.planes > 4) return false;
    for (uint32_t p = 0; p < a.planes; ++p)
        if (!a.src[p] || !a.dst[p] || ((uintptr_t)a.src[p] & 15) || ((uintptr_t)a.dst[p] & 15) || (a.src_pitch[p] & 3) || (a.dst_pitch[p] & 3) ||
            a.src_pitch[p] < a.w || a.dst_pitch[p] < a.w)
            return false;
    return true;
}

hipError_t launch_blur_rows(const BlurArgs &a, bool wrap, bool nt, hipStream_t s)
{
    const uint64_t groups = blur_rows_groups(a.w, a.h);
    if (!blur_args_ok(a) || groups > 0x7fffffffull) return hipErrorInvalidValue;
#define KC_BLUR(NT, WR) blur_rows_kernel<NT, WR><<<dim3((uint32_t)groups, a.planes), 256, 0, s>>>(a)
    if (nt) {
        if (wrap) KC_BLUR(true, true);
        else KC_BLUR(true, false);
    } else {
        if (wrap) KC_BLUR(false, true);
        else KC_BLUR(false, false);
    }
#undef KC_BLUR
    return hipGetLastError();
}

hipError_t launch_blur_columns(const BlurArgs &a, bool wrap, bool nt, hipStream_t s)
{
    const uint64_t groups = blur_columns_groups(a.w, a.h);
    if (!blur_args_ok(a) || groups > 0x7fffffffull) return hipErrorInvalidValue;
    const size_t lds = blur_columns_lds(a.radius);
#define KC_BLUR(NT, WR) blur_columns_kernel<NT, WR><<<dim3((uint32_t)groups, a.planes), 256, lds, s>>>(a)
    if (nt) {
        if (wrap) KC_BLUR(true, true);
        else KC_BLUR(true, false);
    } else {
        if (wrap) KC_BLUR(false, true);
        else KC_BLUR(false, false);
    }
#undef KC_BLUR
    return hipGetLastError();
}

}  // namespace kc
