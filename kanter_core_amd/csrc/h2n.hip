// ------------------------------------------------------------------------------------------
// HeightToNormal: src/node/height_to_normal.rs:16-77 with the toroidal wrap of
// src/node/process_shared.rs:31-65; nalgebra 0.29 normalize = v / sqrt((x*x + y*y) + z*z).
// 4 B read + 12 B written per pixel (alpha is a constant plane).
// ------------------------------------------------------------------------------------------
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // grid_cap, st_policy

typedef float f4 __attribute__((ext_vector_type(4)));

static __device__ __forceinline__ void vnorm3(float x, float y, float z, float &ox, float &oy, float &oz)
{
    const float n = sqrtf((x * x + y * y) + z * z);
    ox = x / n;
    oy = y / n;
    oz = z / n;
}

// 0.0f / n for a norm n that is never zero here (n >= 1/width > 0): +0 unless n is NaN.  Saves two
// of the nine IEEE divisions per pixel; this kernel is bound by divide / sqrt issue, not by HBM.
static __device__ __forceinline__ float zero_over(float n) { return n != n ? n : 0.0f; }

// Several IEEE divisions by one denominator.  This is the compiler's own correctly rounded f32
// division (v_div_scale / v_rcp / Newton steps / v_div_fmas / v_div_fixup) with the steps that depend
// only on the denominator done once -- valid where v_div_scale would not rescale and v_div_fixup
// would not intervene: b normal with a normal reciprocal, a == 0 or |a| >= 2^-103, a / b normal and
// exponent(a) - exponent(b) < 96.  h2n_px establishes those bounds before taking this path.
struct SharedDenominator {
    float nb, r;  // -b, reciprocal after one Newton step
};

static __device__ __forceinline__ SharedDenominator shared_denominator(float b)
{
    const float r0 = __builtin_amdgcn_rcpf(b);
    const float e = __builtin_fmaf(-b, r0, 1.0f);
    return { -b, __builtin_fmaf(e, r0, r0) };
}

template <bool MAY_BE_ZERO = true>
static __device__ __forceinline__ float divide_by(const SharedDenominator &d, float a)
{
    const float m = a * d.r;
    const float f2 = __builtin_fmaf(d.nb, m, a);
    const float f3 = __builtin_fmaf(f2, d.r, m);
    const float f4 = __builtin_fmaf(d.nb, f3, a);
    const float q = __builtin_fmaf(f4, d.r, f3);
    // b > 0: the quotient has a's sign; for a == -0 the steps above give +0, so put the sign back
    return MAY_BE_ZERO ? __builtin_copysignf(q, a) : q;
}

// sqrt for normal x without the compiler's denormal scaling and +-1 ulp fix-up: the rsq / Newton /
// residual sequence LLVM itself uses when denormals are flushed.  Correctly rounded on [2^-96, 2^100)
// (every value checked against sqrtf: profiles/exact_math_check.hip).
static __device__ __forceinline__ float sqrt_normal(float x)
{
    const float y = __builtin_amdgcn_rsqf(x);
    const float s0 = x * y;
    const float h0 = y * 0.5f;
    const float e = __builtin_fmaf(-h0, s0, 0.5f);
    const float h = __builtin_fmaf(h0, e, h0);
    const float s = __builtin_fmaf(s0, e, s0);
    const float d = __builtin_fmaf(-s, s, x);
    return __builtin_fmaf(d, h, s);
}

static __device__ __forceinline__ void h2n_px(float px, float up, float left, float pdx, float pdy, float &r, float &g,
                                              float &b)
{
    // tangent = (pdx, 0, px - left) / |.|, bitangent = (0, pdy, up - px) / |.|;
    // |v| = sqrt((x*x + y*y) + z*z) and x*x + 0*0 == x*x exactly
    const float tz0 = px - left, bz0 = up - px;
    const float q1 = pdx * pdx + tz0 * tz0, q2 = pdy * pdy + bz0 * bz0;
    // Height steps that are 0 or within [2^-40, 2^7] (and 2^-16 <= pdx, pdy <= 1: sizes are at most
    // 65535) keep every operation below inside the bounds of sqrt_normal / SharedDenominator:
    // q1, q2 in [2^-32, 2^15], n1, n2 in [2^-16, 2^7.5], tangent parts in {0} u [2^-47.5, 1], cross
    // products in {0} u [2^-71, 1], cz >= 2^-47, so |cross|^2 in [2^-94, 3].
    const float atz = fabsf(tz0), abz = fabsf(bz0);
    const bool tame = (tz0 == 0.0f || (atz >= 0x1p-40f && atz <= 0x1p7f)) && (bz0 == 0.0f || (abz >= 0x1p-40f && abz <= 0x1p7f));
    float nx, ny, nz;
    if (tame) {
        const SharedDenominator d1 = shared_denominator(sqrt_normal(q1)), d2 = shared_denominator(sqrt_normal(q2));
        const float tx = divide_by<false>(d1, pdx), tz = divide_by(d1, tz0);
        const float by = divide_by<false>(d2, pdy), bz = divide_by(d2, bz0);
        const float ty = 0.0f, bx = 0.0f;  // 0 / n
        const float cx = ty * bz - tz * by;
        const float cy = tz * bx - tx * bz;
        const float cz = tx * by - ty * bx;
        const SharedDenominator d3 = shared_denominator(sqrt_normal((cx * cx + cy * cy) + cz * cz));
        nx = divide_by(d3, cx);
        ny = divide_by(d3, cy);
        nz = divide_by<false>(d3, cz);  // cz = tx * by > 0
    } else {
        const float n1 = sqrtf(q1), n2 = sqrtf(q2);
        const float tx = pdx / n1, ty = zero_over(n1), tz = tz0 / n1;
        const float bx = zero_over(n2), by = pdy / n2, bz = bz0 / n2;
        const float cx = ty * bz - tz * by;
        const float cy = tz * bx - tx * bz;
        const float cz = tx * by - ty * bx;
        vnorm3(cx, cy, cz, nx, ny, nz);
    }
    r = nx * 0.5f + 0.5f;
    g = ny * 0.5f + 0.5f;
    b = nz * 0.5f + 0.5f;
}

// The same arithmetic for the 4 pixels of a quad at once, written on 4-wide vectors so that the Newton / residual
// steps of the shared-denominator division and of the square root become packed instructions (v_pk_fma_f32,
// v_pk_mul_f32: two pixels per instruction) -- this kernel is bound by vector-instruction issue, not by HBM.
// Element by element these are exactly the operations of h2n_px's `tame` branch (same instructions, same order);
// a quad with any pixel outside that range goes through h2n_px pixel by pixel.
typedef float f2 __attribute__((ext_vector_type(2)));
template <class V> static __device__ __forceinline__ V fmaV(V a, V b, V c) { return __builtin_elementwise_fma(a, b, c); }
template <class V> static __device__ __forceinline__ V splatV(float v)
{
    V o;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(V) / sizeof(float)); ++i) o[i] = v;
    return o;
}
template <class V> static __device__ __forceinline__ V rsqV(V x)
{
    V o;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(V) / sizeof(float)); ++i) o[i] = __builtin_amdgcn_rsqf(x[i]);
    return o;
}
template <class V> static __device__ __forceinline__ V copysignV(V mag, V sgn)
{
    V o;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(V) / sizeof(float)); ++i) o[i] = __builtin_copysignf(mag[i], sgn[i]);
    return o;
}
template <class V> struct SharedDenominatorV {
    V nb, r;
};
// The denominator-only part of the division by n = sqrt_normal(x), with the reciprocal seeded by the rsq the square root
// starts from anyway instead of a separate v_rcp_f32 of n: y = rsq(x) is 1 / n to ~2^-22, one Newton step on n takes it to
// the same ~2^-45 the rcp-seeded step reaches, and the quotient's correction steps are the same.  Transcendental
// instructions run at a quarter of the packed-math rate: this halves them (6 -> 3 per pixel).  Checked against a / sqrtf(x)
// over 3 x 2^34 (a, x) pairs in the ranges h2n_quad establishes (profiles/exact_math_check.hip, r02_exact_math_check.txt).
template <class V> static __device__ __forceinline__ SharedDenominatorV<V> sqrt_denominatorV(V x)
{
    const V half = splatV<V>(0.5f), one = splatV<V>(1.0f);
    const V y = rsqV(x);
    const V s0 = x * y;
    const V h0 = y * half;
    const V e = fmaV(-h0, s0, half);
    const V h = fmaV(h0, e, h0);
    const V s = fmaV(s0, e, s0);
    const V d = fmaV(-s, s, x);
    const V n = fmaV(d, h, s);  // sqrt_normal(x)
    const V er = fmaV(-n, y, one);
    return { -n, fmaV(er, y, y) };
}

template <bool MAY_BE_ZERO, class V>
static __device__ __forceinline__ V divide_byV(const SharedDenominatorV<V> &d, V a)
{
    const V m = a * d.r;
    const V f2_ = fmaV(d.nb, m, a);
    const V f3 = fmaV(f2_, d.r, m);
    const V f4_ = fmaV(d.nb, f3, a);
    const V q = fmaV(f4_, d.r, f3);
    return MAY_BE_ZERO ? copysignV(q, a) : q;
}

// The tame path on V = 2 or 4 pixels: element by element exactly the operations of h2n_px's `tame` branch.
template <class V>
static __device__ __forceinline__ void h2n_fast(V tz0, V bz0, float pdx, float pdy, V &r, V &g, V &b)
{
    const V vdx = splatV<V>(pdx), vdy = splatV<V>(pdy), half = splatV<V>(0.5f);
    const V q1 = vdx * vdx + tz0 * tz0, q2 = vdy * vdy + bz0 * bz0;
    const SharedDenominatorV<V> d1 = sqrt_denominatorV(q1), d2 = sqrt_denominatorV(q2);
    const V tx = divide_byV<false>(d1, vdx), tz = divide_byV<true>(d1, tz0);
    const V by = divide_byV<false>(d2, vdy), bz = divide_byV<true>(d2, bz0);
    // t = (tx, 0, tz), b = (0, by, bz): the cross product's products with the two zero components (0 / n = +0) vanish.
    //   cx = 0 * bz - tz * by = -(tz * by),  cy = tz * 0 - tx * bz = -(tx * bz),  cz = tx * by - 0 * 0 = tx * by
    // exactly, for the finite values of this path -- except the SIGN of a zero result (+-0 - +-0), which cannot reach the
    // output: cx and cy enter as squares and as (+-0 / n) * 0.5 + 0.5 = 0.5.
    const V cx = -(tz * by);
    const V cy = -(tx * bz);
    const V cz = tx * by;
    const SharedDenominatorV<V> d3 = sqrt_denominatorV((cx * cx + cy * cy) + cz * cz);
    const V nx = divide_byV<true>(d3, cx), ny = divide_byV<true>(d3, cy), nz = divide_byV<false>(d3, cz);
    r = nx * half + half;
    g = ny * half + half;
    b = nz * half + half;
}

static __device__ __forceinline__ bool tame1(float d)
{
    const float a = fabsf(d);
    return d == 0.0f || (a >= 0x1p-40f && a <= 0x1p7f);
}

// px, up, left: the quad's heights, the heights above them, the heights to their left
static __device__ __forceinline__ void h2n_quad(f4 px, f4 up, f4 left, float pdx, float pdy, f4 &r, f4 &g, f4 &b)
{
    const f4 tz0 = px - left, bz0 = up - px;
    const bool tame = tame1(tz0.x) && tame1(tz0.y) && tame1(tz0.z) && tame1(tz0.w) && tame1(bz0.x) && tame1(bz0.y) &&
                      tame1(bz0.z) && tame1(bz0.w);
    if (!tame) {
        float rr[4], gg[4], bb[4];
        h2n_px(px.x, up.x, left.x, pdx, pdy, rr[0], gg[0], bb[0]);
        h2n_px(px.y, up.y, left.y, pdx, pdy, rr[1], gg[1], bb[1]);
        h2n_px(px.z, up.z, left.z, pdx, pdy, rr[2], gg[2], bb[2]);
        h2n_px(px.w, up.w, left.w, pdx, pdy, rr[3], gg[3], bb[3]);
        r = f4{ rr[0], rr[1], rr[2], rr[3] };
        g = f4{ gg[0], gg[1], gg[2], gg[3] };
        b = f4{ bb[0], bb[1], bb[2], bb[3] };
        return;
    }
    // (as two pairs in sequence the fast path fits 62 VGPRs = 8 waves per SIMD, and is no faster: 50.1-50.5 against 51.3 us,
    // profiles/r03_h2n_ab.txt -- the kernel is bound by vector issue and its hazard nops, not by occupancy)
    h2n_fast<f4>(tz0, bz0, pdx, pdy, r, g, b);
}

// BAND = false: the whole plane, rows wrap around (row -1 = row h - 1).  BAND = true: a row band -- `hgt` holds
// h + 1 rows, the band's rows preceded by the row above its first one (the caller's halo: the previous band's last
// row, or the image's last row for the band that starts at row 0); `full_h` is the height of the whole image, which
// is what the bitangent's 1 / height means (src/node/height_to_normal.rs:38).
// TILED: a workgroup is 2^tq column quads x 256 / 2^tq rows instead of 256 consecutive quads of one row, and the grid is
// (column block, row group) with the column block fastest.  Workgroups go to the 8 XCDs in turn (id % 8), so with a multiple of
// 8 column blocks per row a column block stays on ONE XCD all the way down the image: the row above, which every pixel reads,
// is in this workgroup or was loaded a moment ago by the same XCD -- an L2 hit instead of a second trip over the fabric for
// the whole plane (4096^2: 51.0 -> 43.7 us, 0.66 -> 0.77 of the HBM peak; profiles/r03_h2n_tiled_ab.txt).
template <bool BAND, bool NT, bool TILED>  // NT: the three result planes do not fit the Infinity Cache (cache_policy_mask)
__global__ __launch_bounds__(256) void height_to_normal_kernel(const float *__restrict__ hgt, uint32_t hpitch,
                                                               uint32_t w, uint32_t h, uint32_t full_h,
                                                               float *__restrict__ nx, float *__restrict__ ny,
                                                               float *__restrict__ nz, uint32_t opitch, uint32_t tq)
{
    const uint32_t row_units = (w + 3) / 4;
    const uint32_t total = row_units * h;
    const float pdx = 1.0f / (float)w;
    const float pdy = 1.0f / (float)full_h;
    auto pixel_quad = [&](uint32_t y, uint32_t q) {
        const uint32_t yc = BAND ? y + 1 : y;                          // row of this pixel in `hgt`
        const uint32_t yu = BAND ? y : (y == 0 ? h - 1 : y - 1);       // row above it
        const float *rowp = hgt + (size_t)yc * hpitch;
        const f4 cur = *reinterpret_cast<const f4 *>(rowp + 4 * q);
        const f4 upv = *reinterpret_cast<const f4 *>(hgt + (size_t)yu * hpitch + 4 * q);
        const float lft = q == 0 ? rowp[w - 1] : rowp[4 * q - 1];
        f4 r, g, b;
        h2n_quad(cur, upv, f4{ lft, cur.x, cur.y, cur.z }, pdx, pdy, r, g, b);
        const size_t o = (size_t)y * opitch + 4 * q;
        st_policy<NT>(reinterpret_cast<f4 *>(nx + o), r);
        st_policy<NT>(reinterpret_cast<f4 *>(ny + o), g);
        st_policy<NT>(reinterpret_cast<f4 *>(nz + o), b);
    };
    if (TILED) {  // the grid covers the image: one quad per thread
        const uint32_t q = (blockIdx.x << tq) + (threadIdx.x & ((1u << tq) - 1u)), y = (blockIdx.y << (8u - tq)) + (threadIdx.x >> tq);
        if (q < row_units && y < h) pixel_quad(y, q);
    } else {
        for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
            const uint32_t y = idx / row_units;
            pixel_quad(y, idx - y * row_units);
        }
    }
}

// h = rows to produce; band != 0: `hgt` has h + 1 rows (halo row first) and full_h is the whole image's height.
hipError_t launch_height_to_normal(const float *hgt, uint32_t hpitch, uint32_t w, uint32_t h, uint32_t full_h, int band,
                                   float *nx, float *ny, float *nz, uint32_t opitch, uint32_t nt_mask, hipStream_t s, H2nVariant *var)
{
    const bool nts = (nt_mask & 0x100u) != 0;  // the height plane is re-read by neighbouring rows: never marked
    const uint64_t total = (uint64_t)((w + 3) / 4) * h;
    if (total == 0) return hipSuccess;
    const uint32_t row_units = (w + 3) / 4;
    // Tile width: 128, 64 or 32 quads, the widest that cuts the row into a multiple of 8 column blocks (widths that are
    // multiples of 4096, 2048 or 1024 pixels), else the widest the row holds -- rows shared inside the workgroup pay even when
    // the column blocks wander over the XCDs (3000^2: 29.5 -> 26.3 us).  KC_H2N_TILED=0: the plain mapping (A/B).
    uint32_t tq = 0;
    for (uint32_t t : { 7u, 6u, 5u })
        if (!tq && row_units % (8u << t) == 0) tq = t;
    for (uint32_t t : { 7u, 6u, 5u })
        if (!tq && row_units >= (1u << t)) tq = t;
    bool tiled = options().h2n_tiled != 0 && tq != 0;
    if (!tq) tq = 7;
    if ((((uint64_t)h + (256u >> tq) - 1) >> (8u - tq)) >= 65536u) tiled = false;
    uint64_t blocks = (total + 255) / 256;
    if (blocks > grid_cap(1u << 30)) blocks = grid_cap(1u << 30);
    const dim3 grid = tiled ? dim3((row_units + (1u << tq) - 1u) >> tq, (h + (256u >> tq) - 1u) >> (8u - tq)) : dim3((unsigned)blocks);
    if (!band) full_h = h;
#define KC_H2N(BAND, NT)                                                                                                         \
    do {                                                                                                                         \
        if (tiled) height_to_normal_kernel<BAND, NT, true><<<grid, 256, 0, s>>>(hgt, hpitch, w, h, full_h, nx, ny, nz, opitch, tq);   \
        else height_to_normal_kernel<BAND, NT, false><<<grid, 256, 0, s>>>(hgt, hpitch, w, h, full_h, nx, ny, nz, opitch, tq);        \
    } while (0)
    if (band && nts) KC_H2N(true, true);
    else if (band) KC_H2N(true, false);
    else if (nts) KC_H2N(false, true);
    else KC_H2N(false, false);
#undef KC_H2N
    if (var) *var = H2nVariant{ true, band != 0, nts, tiled ? tq : 0u };
    return hipGetLastError();
}

}  // namespace kc
