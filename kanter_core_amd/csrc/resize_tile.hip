// The tiled resamplers: a workgroup owns a tile of the output, runs the vertical pass into LDS and the horizontal pass out of
// it (resize_lds_kernel: windows of up to 8 taps in registers; resize_wide_kernel: wider ones; resize_chain_kernel: the
// resampled tile feeds a Mix chain instead of being stored) -- and the two-pass pair through an HBM intermediate they replace.
// The wave-uniform down-samplers are resize_down.hip and down2.hip, the integer-ratio up-samplers upsample.hip.
#include "kc_internal.hpp"

namespace kc {

#include "chain_apply.inc"  // f4, apply1<CODE>
#include "chain_interp.inc"  // apply4 / apply4c, KC_CODE_SWITCH*, chain_run: shared by chain.hip, resize_tile.hip and upsample.hip
#include "resample.inc"  // clamp01_nan_passthrough: shared by resize_tile.hip and resize_down.hip

// Pass 1 of the two-pass form: tmp[oy][x] = sum_j src[left_v[oy] + j][x] * w_v[oy][j].
__global__ __launch_bounds__(256) void resize_vertical_kernel(const float *__restrict__ src, uint32_t spitch,
                                                              uint32_t sw, float *__restrict__ tmp, uint32_t tpitch,
                                                              TapsDev V)
{
    const uint32_t oy = blockIdx.y;
    const uint32_t left = V.left[oy];
    const uint32_t n = V.count[oy];
    const float *w = V.w + (size_t)oy * V.stride;
    for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < sw; x += gridDim.x * 256u) {
        float t = 0.0f;
        for (uint32_t j = 0; j < n; ++j) t += src[(size_t)(left + j) * spitch + x] * w[j];
        tmp[(size_t)oy * tpitch + x] = t;
    }
}

// Pass 2: dst[oy][ox] = clamp(sum_j tmp[oy][left_h[ox] + j] * w_h[ox][j], 0, 1).
__global__ __launch_bounds__(256) void resize_horizontal_kernel(const float *__restrict__ tmp, uint32_t tpitch,
                                                                float *__restrict__ dst, uint32_t dpitch,
                                                                uint32_t dw, TapsDev H)
{
    const uint32_t oy = blockIdx.y;
    for (uint32_t ox = blockIdx.x * 256u + threadIdx.x; ox < dw; ox += gridDim.x * 256u) {
        const uint32_t left = H.left[ox];
        const uint32_t n = H.count[ox];
        const float *w = H.w + (size_t)ox * H.stride;
        float t = 0.0f;
        for (uint32_t j = 0; j < n; ++j) t += tmp[(size_t)oy * tpitch + left + j] * w[j];
        dst[(size_t)oy * dpitch + ox] = clamp01_nan_passthrough(t);
    }
}

hipError_t launch_resize_vertical(const float *src, uint32_t spitch, uint32_t sw, float *tmp, uint32_t tpitch,
                                  uint32_t dh, TapsDev v, hipStream_t s)
{
    if (sw == 0 || dh == 0) return hipSuccess;
    uint32_t bx = (sw + 255) / 256;
    if (bx > 64) bx = 64;
    resize_vertical_kernel<<<dim3(bx, dh), 256, 0, s>>>(src, spitch, sw, tmp, tpitch, v);
    return hipGetLastError();
}

hipError_t launch_resize_horizontal(const float *tmp, uint32_t tpitch, float *dst, uint32_t dpitch, uint32_t dw,
                                    uint32_t dh, TapsDev h, hipStream_t s)
{
    if (dw == 0 || dh == 0) return hipSuccess;
    uint32_t bx = (dw + 255) / 256;
    if (bx > 64) bx = 64;
    resize_horizontal_kernel<<<dim3(bx, dh), 256, 0, s>>>(tmp, tpitch, dst, dpitch, dw, h);
    return hipGetLastError();
}

// Single-pass tiled form: each workgroup owns a tile_h x tile_w output tile.
//   phase 1 vertical pass HBM -> LDS: (tile row, 4-column group) items dealt out to all lanes; a
//           lane reads its item's source rows with 16-byte loads, several in flight, weights from
//           the LDS copy of the tile rows' tap table (resize_vpass_items).  Rows shared by
//           neighbouring output rows are re-read through L1/L2, not HBM.  The intermediate the
//           two-pass form would write to HBM (tile_h x ncp floats) never leaves the CU;
//   phase 2 horizontal pass out of LDS: every thread owns 4 consecutive output columns for the
//           whole tile, so its tap windows and weights sit in registers and the
//           four results leave as one 16-byte store -- or, in resize_chain_kernel, feed the Mix
//           chain that consumes the resampled plane without ever being written.
// Same operands, same order, same roundings as the two-pass form: bit-identical output.
// Algorithmic bytes per output pixel = 4 * (1 + in_px / out_px).
struct ResizeTile {
    uint32_t x0, y0, x1, y1, th, c0;
    const float *tmp;  // tile_h x ncp vertical-pass intermediate in LDS
};

template <int MAXT>
struct ResizeCols {  // the 4 output columns a thread owns: window start (tile-relative), weights, which taps exist
    typedef float f2 __attribute__((ext_vector_type(2)));
    uint32_t hl[4];
    f2 w01[MAXT], w23[MAXT];  // the weights of columns 0, 1 and 2, 3 as the packed multiply takes them
    bool live[4][MAXT];
    uint32_t minc;  // fewest taps of the four
};

template <int MAXT>
static __device__ __forceinline__ void resize_load_cols(ResizeCols<MAXT> &C, const TapsDev &H, uint32_t ox, uint32_t x1,
                                                        uint32_t c0)
{
    C.minc = 0xFFFFFFFFu;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t x = min(ox + e, x1 - 1);
        C.hl[e] = H.left[x] - c0;
        const uint32_t hn = H.count[x];
        C.minc = min(C.minc, hn);
        const float *wh = H.w + (size_t)x * H.stride;
#pragma unroll
        for (int j = 0; j < MAXT; ++j) {
            (e < 2 ? C.w01[j] : C.w23[j])[e & 1] = wh[j];  // rows of the table are zero-padded to `stride` entries
            C.live[e][j] = (uint32_t)j < hn;
        }
    }
}

// Phase 1 for the workgroup's tile; ends with the barrier that publishes `tmp`.
// `src` rows are 16-byte aligned (plane pitch is a multiple of 16 bytes), so the window starts at
// c0 = first source column rounded down to a multiple of 4; the last group may run past the
// source width into the row's pitch padding -- those intermediates are never read by phase 2.
// Work items are (tile row, 4-column group) pairs dealt out to all 256 lanes; a lane walks its
// item's window VU source rows at a time (VU independent 16-byte loads in flight), its taps read
// from the LDS copy of the tile rows' tap table.  Everything is per lane: no scalar-unit work
// beyond the loop counters (the scalar unit is shared by the CU's four SIMDs).
// Taps every row of the tile has (j < vmin) are summed unconditionally; the remaining ones are
// per-lane predicated: a tap past a lane's window repeats its last row and adds -0.0.
// SWZ: the intermediate row is stored with one float of padding after every 32 (index i lives at i + (i >> 5)), the
// layout resize_wide_kernel's horizontal pass reads without bank conflicts; `ncp4` is then unused and `ncp_swz` is the
// row pitch in floats.
template <int VU, bool SWZ = false>
static __device__ __forceinline__ void resize_vpass_items(const f4 *__restrict__ src4, uint32_t sp4, f4 *tmp4, uint32_t ncp4,
                                                          uint32_t th, uint32_t nq, const uint32_t *vl, const uint32_t *vn,
                                                          const float *vw, uint32_t vstride, uint32_t vmin, uint32_t ncp_swz = 0)
{
    auto add = [](f4 &a, const f4 &px, float wt) {
        a.x += px.x * wt;
        a.y += px.y * wt;
        a.z += px.z * wt;
        a.w += px.w * wt;
    };
    const uint32_t items = th * nq;
    // i / nq by multiply-high: exact here because i < th * nq <= 4096 (16 bytes of LDS per item, 64 KiB)
    const uint32_t nq_magic = nq > 1 ? 0xFFFFFFFFu / nq + 1u : 0u;
    for (uint32_t i = threadIdx.x; i < items; i += 256u) {
        const uint32_t ty = nq > 1 ? __umulhi(i, nq_magic) : i;
        const uint32_t q = i - ty * nq;
        const uint32_t n = vn[ty];
        const f4 *col = src4 + (size_t)vl[ty] * sp4 + q;
        const float *w = vw + ty * vstride;
        f4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
        uint32_t j0 = 0;
        for (; j0 + VU <= vmin; j0 += VU) {
            f4 p[VU];
            float wt[VU];
#pragma unroll
            for (int u = 0; u < VU; ++u) {
                p[u] = col[(size_t)(j0 + u) * sp4];
                wt[u] = w[j0 + u];
            }
#pragma unroll
            for (int u = 0; u < VU; ++u) add(acc, p[u], wt[u]);
        }
        if constexpr (VU > 4) {
            // (windows of 5 .. 7 taps everywhere in the tile -- up-sampling with CatmullRom, Lanczos3, Gaussian: four of them need
            // no predicate either)
            for (; j0 + 4u <= vmin; j0 += 4u) {
                f4 p[4];
                float wt[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    p[u] = col[(size_t)(j0 + u) * sp4];
                    wt[u] = w[j0 + u];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) add(acc, p[u], wt[u]);
            }
        }
        for (; j0 < vstride; j0 += 4u) {
            f4 p[4];
            float wt[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                p[u] = col[(size_t)min(j0 + u, n - 1u) * sp4];
                wt[u] = w[min(j0 + u, vstride - 1u)];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool live = j0 + u < n;
                acc.x += live ? p[u].x * wt[u] : -0.0f;
                acc.y += live ? p[u].y * wt[u] : -0.0f;
                acc.z += live ? p[u].z * wt[u] : -0.0f;
                acc.w += live ? p[u].w * wt[u] : -0.0f;
            }
        }
        if constexpr (SWZ) {
            float *o = reinterpret_cast<float *>(tmp4) + ty * ncp_swz + 4u * q + (q >> 3);  // a quad never straddles a multiple of 32
            o[0] = acc.x;
            o[1] = acc.y;
            o[2] = acc.z;
            o[3] = acc.w;
        } else {
            tmp4[ty * ncp4 + q] = acc;
        }
    }
}

// SWZ (resize_wide_kernel): rows of `tmp` are ncp + ncp / 32 + 1 floats apart and swizzled, see resize_vpass_items.
template <bool SWZ = false>
static __device__ __forceinline__ ResizeTile resize_tile_vpass(float *lds, const float *__restrict__ src,
                                                               uint32_t spitch, uint32_t dw, uint32_t dh,
                                                               const TapsDev &V, const TapsDev &H, uint32_t tile_w,
                                                               uint32_t tile_h, uint32_t ncp)
{
    const uint32_t row_floats = SWZ ? ncp + (ncp >> 5) + 1u : ncp;
    ResizeTile T;
    T.x0 = blockIdx.x * tile_w;
    T.y0 = blockIdx.y * tile_h;
    T.x1 = min(T.x0 + tile_w, dw);
    T.y1 = min(T.y0 + tile_h, dh);
    T.th = T.y1 - T.y0;
    T.c0 = H.left[T.x0] & ~3u;
    T.tmp = lds;
    const uint32_t nq = (H.left[T.x1 - 1] + H.count[T.x1 - 1] - T.c0 + 3u) / 4u;  // <= ncp / 4 (host-checked)

    // the tile rows' vertical taps: one coalesced fetch into LDS
    uint32_t *vl = reinterpret_cast<uint32_t *>(lds + tile_h * row_floats + 8u);
    uint32_t *vn = vl + tile_h;
    float *vw = reinterpret_cast<float *>(vn + tile_h);  // tile_h x V.stride
    for (uint32_t i = threadIdx.x; i < T.th; i += 256u) {
        vl[i] = V.left[T.y0 + i];
        vn[i] = V.count[T.y0 + i];
    }
    for (uint32_t i = threadIdx.x; i < T.th * V.stride; i += 256u) vw[i] = V.w[(size_t)T.y0 * V.stride + i];
    __syncthreads();
    // fewest taps of any row of this tile (tile_h <= 64: one value per lane, butterfly minimum)
    uint32_t vmin = (threadIdx.x & 63u) < T.th ? vn[threadIdx.x & 63u] : 0xFFFFFFFFu;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) vmin = min(vmin, (uint32_t)__shfl_xor((int)vmin, off));
    vmin = (uint32_t)__builtin_amdgcn_readfirstlane((int)vmin);

    const f4 *src4 = reinterpret_cast<const f4 *>(src + T.c0);
    f4 *tmp4 = reinterpret_cast<f4 *>(lds);
    if (V.stride <= 4u)
        resize_vpass_items<4, SWZ>(src4, spitch / 4u, tmp4, ncp / 4u, T.th, nq, vl, vn, vw, V.stride, vmin, row_floats);
    else
        resize_vpass_items<8, SWZ>(src4, spitch / 4u, tmp4, ncp / 4u, T.th, nq, vl, vn, vw, V.stride, vmin, row_floats);
    __syncthreads();
    return T;
}

// Horizontal pass for one tile row and this thread's 4 columns.  Taps j < MINT need no predicate (every lane of the wave has
// them); columns 0, 1 and 2, 3 go through the packed multiply and add as pairs (their weights sit in register pairs for the
// whole tile; as four separate sums the compiler packed products of one column's neighbouring taps and then shuffled them
// apart again for the adds: 35 moves per row and thread).
template <int MINT, int MAXT>
static __device__ __forceinline__ void resize_out_row(const ResizeCols<MAXT> &C, const float *row, float (&res)[4])
{
    typedef float f2 __attribute__((ext_vector_type(2)));
    // Taps are contiguous from hl[e]: one base address per output, constant offsets per tap.  A tap past the window reads the
    // next floats of the LDS block -- always inside the allocation (the vertical tap table follows tmp) -- and is discarded below.
    f2 t01 = { 0.0f, 0.0f }, t23 = { 0.0f, 0.0f };
    const float *pe[4] = { row + C.hl[0], row + C.hl[1], row + C.hl[2], row + C.hl[3] };
#pragma unroll
    for (int j = 0; j < MAXT; ++j) {
        f2 q01 = f2{ pe[0][j], pe[1][j] } * C.w01[j];
        f2 q23 = f2{ pe[2][j], pe[3][j] } * C.w23[j];
        if (j >= MINT) {
            // a tap that does not exist contributes -0.0: t + (-0.0) == t for every t (including +-0, +-inf, NaN), so the sum
            // equals the reference's shorter sum
            q01.x = C.live[0][j] ? q01.x : -0.0f;
            q01.y = C.live[1][j] ? q01.y : -0.0f;
            q23.x = C.live[2][j] ? q23.x : -0.0f;
            q23.y = C.live[3][j] ? q23.y : -0.0f;
        }
        t01 += q01;
        t23 += q23;
    }
    res[0] = clamp01_nan_passthrough(t01.x);
    res[1] = clamp01_nan_passthrough(t01.y);
    res[2] = clamp01_nan_passthrough(t23.x);
    res[3] = clamp01_nan_passthrough(t23.y);
}

// How many taps a wave may sum without a predicate: all of its lanes' columns have MAXT - 2 (windows of 6 or 8 register taps:
// up-sampling by a non-integer ratio has 4 - 5 taps with CatmullRom, 6 - 7 with Lanczos3 / Gaussian) or MAXT - 1 (4 register
// taps), else what the whole image guarantees.
template <int MINT, int MAXT>
struct ResizeUmin {
    static constexpr int value = MAXT >= 6 ? MAXT - 2 : MAXT == 4 ? 3 : MINT;
};

template <int MINT, int MAXT>  // horizontal taps, all in registers: MINT unconditional, up to MAXT
__global__ __launch_bounds__(256) void resize_lds_kernel(const ResizePlanes P, uint32_t dw, uint32_t dh, TapsDev V,
                                                         TapsDev H, uint32_t tile_w, uint32_t tile_h, uint32_t ncp)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const float *__restrict__ src = P.src[blockIdx.z];  // blockIdx.z = plane: up to 4 planes of one image per launch
    float *__restrict__ dst = P.dst[blockIdx.z];
    const uint32_t spitch = P.spitch[blockIdx.z], dpitch = P.dpitch[blockIdx.z];
    const uint32_t col_groups = tile_w / 4;         // threads across one tile row
    const uint32_t row_groups = 256u / col_groups;  // tile rows in flight
    const uint32_t cg = threadIdx.x % col_groups;
    const uint32_t rg = threadIdx.x / col_groups;
    const uint32_t x0 = blockIdx.x * tile_w, x1 = min(x0 + tile_w, dw);
    const uint32_t ox = x0 + 4 * cg;
    // this thread's 4 output columns (fetched first so the loads overlap the staging)
    ResizeCols<MAXT> C;
    resize_load_cols<MAXT>(C, H, ox, x1, H.left[x0] & ~3u);
    const ResizeTile T = resize_tile_vpass(lds, src, spitch, dw, dh, V, H, tile_w, tile_h, ncp);
    constexpr int UMIN = ResizeUmin<MINT, MAXT>::value;
    // (asked of every lane, also those without columns: their minc is that of the tile's last column)
    const bool wave_has_umin = UMIN > MINT && __builtin_amdgcn_ballot_w64(C.minc < (uint32_t)UMIN) == 0ull;
    if (ox >= T.x1) return;
    if (ox + 3 < T.x1) {
        // interior columns: one 16-byte store per row
        if (wave_has_umin) {
            for (uint32_t ty = rg; ty < T.th; ty += row_groups) {
                float res[4];
                resize_out_row<UMIN, MAXT>(C, T.tmp + ty * ncp, res);
                *reinterpret_cast<float4 *>(dst + (size_t)(T.y0 + ty) * dpitch + ox) = make_float4(res[0], res[1], res[2], res[3]);
            }
        } else {
            for (uint32_t ty = rg; ty < T.th; ty += row_groups) {
                float res[4];
                resize_out_row<MINT, MAXT>(C, T.tmp + ty * ncp, res);
                *reinterpret_cast<float4 *>(dst + (size_t)(T.y0 + ty) * dpitch + ox) = make_float4(res[0], res[1], res[2], res[3]);
            }
        }
    } else {
        // the tile's last, partial quad
        for (uint32_t ty = rg; ty < T.th; ty += row_groups) {
            float res[4];
            resize_out_row<MINT, MAXT>(C, T.tmp + ty * ncp, res);
            float *o = dst + (size_t)(T.y0 + ty) * dpitch + ox;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (ox + e < T.x1) o[e] = res[e];
        }
    }
}

// Wide horizontal windows (more than 8 taps: down-sampling).  The tile's horizontal tap table is
// staged in LDS behind the vertical one and every thread produces single outputs, four taps per trip
// (both operands come from LDS; a tap past the window repeats the last one and adds -0.0).
__global__ __launch_bounds__(256) void resize_wide_kernel(const ResizePlanes P, uint32_t dw, uint32_t dh, TapsDev V,
                                                          TapsDev H, uint32_t tile_w, uint32_t tile_h, uint32_t ncp,
                                                          uint32_t h_off)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const float *__restrict__ src = P.src[blockIdx.z];
    float *__restrict__ dst = P.dst[blockIdx.z];
    const uint32_t spitch = P.spitch[blockIdx.z], dpitch = P.dpitch[blockIdx.z];
    const uint32_t x0 = blockIdx.x * tile_w, tw = min(x0 + tile_w, dw) - x0;
    const uint32_t c0 = H.left[x0] & ~3u;
    uint32_t *hl = reinterpret_cast<uint32_t *>(lds + h_off);
    uint32_t *hn = hl + tile_w;
    float *hw = reinterpret_cast<float *>(hn + tile_w);  // tile_w x H.stride
    for (uint32_t i = threadIdx.x; i < tw; i += 256u) {
        hl[i] = H.left[x0 + i] - c0;
        hn[i] = H.count[x0 + i];
    }
    for (uint32_t i = threadIdx.x; i < tw * H.stride; i += 256u) hw[i] = H.w[(size_t)x0 * H.stride + i];
    const ResizeTile T = resize_tile_vpass<true>(lds, src, spitch, dw, dh, V, H, tile_w, tile_h, ncp);  // its barriers publish hl/hn/hw
    const uint32_t row_floats = ncp + (ncp >> 5) + 1u;
    const uint32_t sh = 31u - (uint32_t)__clz((int)tile_w);  // tile_w is a power of two
    for (uint32_t i = threadIdx.x; i < T.th * tile_w; i += 256u) {
        const uint32_t ty = i >> sh, x = i & (tile_w - 1u);
        if (x >= tw) continue;
        const uint32_t n = hn[x];
        // Neighbouring outputs read windows `ratio` floats apart: straight indexing put the 32 lanes of a pass on 8 (ratio 4)
        // or 4 (ratio 8) banks -- PMC: 65 % of this pass's LDS cycles were bank conflicts.  The intermediate row is stored
        // with one float of padding after every 32 (resize_vpass_items<.., true>), which spreads strides 2, 4 and 8 over all banks.
        const float *row = T.tmp + ty * row_floats;
        const uint32_t h0 = hl[x];
        const float *w = hw + x * H.stride;
        float t = 0.0f;
        for (uint32_t j0 = 0; j0 < n; j0 += 4u) {
            float p[4], wt[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t jj = min(j0 + u, n - 1u);
                const uint32_t idx = h0 + jj;
                p[u] = row[idx + (idx >> 5)];
                wt[u] = w[jj];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) t += j0 + u < n ? p[u] * wt[u] : -0.0f;
        }
        dst[(size_t)(T.y0 + ty) * dpitch + x0 + x] = clamp01_nan_passthrough(t);
    }
}

// Fused resample + Mix chain: phase 2's four results are input slot K-1 of the chain program, the
// other K-1 inputs are resident planes read with one 16-byte load each, and only the chain's
// result is stored.  The resampled plane itself never exists in HBM: per output pixel the launch
// moves 4 * (K - 1 + 1) bytes plus the (small) source tile instead of 4 * (1 + K + 1).
// blockIdx.z = channel (each channel resamples its own source plane with the shared tap tables).
template <int K, int MAXT>
__global__ __launch_bounds__(256) void resize_chain_kernel(const ChainProgram P, uint32_t dw, uint32_t dh, TapsDev V,
                                                           TapsDev H, uint32_t tile_w, uint32_t tile_h, uint32_t ncp)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t b = blockIdx.z;
    const uint32_t col_groups = tile_w / 4;
    const uint32_t row_groups = 256u / col_groups;
    const uint32_t cg = threadIdx.x % col_groups;
    const uint32_t rg = threadIdx.x / col_groups;
    const uint32_t x0 = blockIdx.x * tile_w, x1 = min(x0 + tile_w, dw);
    const uint32_t ox = x0 + 4 * cg;
    const uint32_t y0 = blockIdx.y * tile_h;
    const uint32_t th = min(tile_h, dh - y0);
    constexpr int KM = K > 1 ? K - 1 : 1;
    const f4 *inp[KM];
    uint32_t ipitch[KM];
#pragma unroll
    for (int k = 0; k < K - 1; ++k) {
        inp[k] = reinterpret_cast<const f4 *>(P.in[b][k]) + ox / 4;  // the whole quad lies inside the pitch
        ipitch[k] = P.in_pitch[b][k];
    }
    // RU tile rows per trip: the chain program is decoded once for RU float4 (its scalar decode is
    // the expensive part, see chain_run); rows past the tile repeat its last row and are not stored.
    // With one resident input, its quads for trip i + 1 are requested before trip i is computed (the
    // first before the vertical pass): a wave then never waits for loads queued behind its own stores.
    constexpr int RU = 4;  // 2 rows per trip: 89.4 us, 1 row: 95.6 us, 4 rows: 83.5 us on config #2 (profiles/r02_fused_ru_ab.txt)
    constexpr bool AHEAD = K <= 2;  // 16 more registers per resident input: not worth the occupancy beyond one
    f4 nxt[KM][RU];
    auto request = [&](uint32_t ty0) {
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const uint32_t oy = y0 + min(ty0 + u * row_groups, th - 1);
#pragma unroll
            for (int k = 0; k < K - 1; ++k) nxt[k][u] = inp[k][oy * ipitch[k]];
        }
    };
    if (AHEAD && ox < x1) request(rg);
    ResizeCols<MAXT> C;
    resize_load_cols<MAXT>(C, H, ox, x1, H.left[x0] & ~3u);
    const ResizeTile T = resize_tile_vpass(lds, P.samp_src[b], P.samp_pitch[b], dw, dh, V, H, tile_w, tile_h, ncp);
    if (ox >= T.x1) return;
    float *outp = P.out[b];
    const uint32_t opitch = P.out_pitch[b] * 4;  // floats
    const bool full = ox + 3 < T.x1;
    for (uint32_t ty0 = rg; ty0 < T.th; ty0 += RU * row_groups) {
        f4 in[K][RU];
        if (!AHEAD) request(ty0);
#pragma unroll
        for (int u = 0; u < RU; ++u)
#pragma unroll
            for (int k = 0; k < K - 1; ++k) in[k][u] = nxt[k][u];
        if (AHEAD && ty0 + RU * row_groups < T.th) request(ty0 + RU * row_groups);
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const uint32_t ty = min(ty0 + u * row_groups, T.th - 1);
            float res[4];
            resize_out_row<1, MAXT>(C, T.tmp + ty * ncp, res);
            in[K - 1][u] = f4{ res[0], res[1], res[2], res[3] };
        }
        f4 acc[RU];
        chain_run<K, RU, 0>(P, b, in, acc);
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const uint32_t ty = ty0 + u * row_groups;
            if (ty >= T.th) break;
            float *o = outp + (size_t)(T.y0 + ty) * opitch + ox;
            if (full) {
                *reinterpret_cast<f4 *>(o) = acc[u];
            } else {
                const float r4[4] = { acc[u].x, acc[u].y, acc[u].z, acc[u].w };
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (ox + e < T.x1) o[e] = r4[e];
            }
        }
    }
}

template <int MINT>
static void launch_resize_lds_t(dim3 grid, size_t lds, hipStream_t s, uint32_t maxt, const ResizePlanes &p, uint32_t dw,
                                uint32_t dh, TapsDev v, TapsDev h, uint32_t tile_w, uint32_t tile_h, uint32_t ncp)
{
#define KC_RESIZE_LAUNCH(MAXT) \
    resize_lds_kernel<(MINT <= MAXT ? MINT : MAXT), MAXT><<<grid, 256, lds, s>>>(p, dw, dh, v, h, tile_w, tile_h, ncp)
    if (maxt == 1) KC_RESIZE_LAUNCH(1);
    else if (maxt == 2) KC_RESIZE_LAUNCH(2);
    else if (maxt == 3) KC_RESIZE_LAUNCH(3);
    else if (maxt == 4) KC_RESIZE_LAUNCH(4);
    else if (maxt == 6) KC_RESIZE_LAUNCH(6);
    else KC_RESIZE_LAUNCH(8);
#undef KC_RESIZE_LAUNCH
}

hipError_t launch_resize_lds(const ResizePlan &r, const ResizePlanes &p, TapsDev v, TapsDev h, hipStream_t s)
{
    if (r.dw == 0 || r.dh == 0) return hipSuccess;
    if (r.planes < 1 || r.planes > 4) return hipErrorInvalidValue;
    if (r.tile_w % 4 != 0 || r.tile_w > 1024 || 256u % (r.tile_w / 4) != 0 || r.tile_h > 64) return hipErrorInvalidValue;
    if (r.form == ResizeForm::wide)
        resize_wide_kernel<<<r.grid, 256, r.lds, s>>>(p, r.dw, r.dh, v, h, r.tile_w, r.tile_h, r.ncp,
                                                      (uint32_t)(r.lds / sizeof(float) - (2u * r.tile_w + (size_t)r.tile_w * h.stride)));
    else if (r.mint >= 2)
        launch_resize_lds_t<2>(r.grid, r.lds, s, r.maxt, p, r.dw, r.dh, v, h, r.tile_w, r.tile_h, r.ncp);
    else
        launch_resize_lds_t<1>(r.grid, r.lds, s, r.maxt, p, r.dw, r.dh, v, h, r.tile_w, r.tile_h, r.ncp);
    return hipGetLastError();
}

template <int K>
static hipError_t launch_resize_chain_k(const ChainProgram &p, dim3 grid, size_t lds, hipStream_t s, uint32_t dw,
                                        uint32_t dh, TapsDev v, TapsDev h, uint32_t tile_w, uint32_t tile_h, uint32_t ncp)
{
    switch (h.stride) {
    case 1: resize_chain_kernel<K, 1><<<grid, 256, lds, s>>>(p, dw, dh, v, h, tile_w, tile_h, ncp); break;
    case 2: resize_chain_kernel<K, 2><<<grid, 256, lds, s>>>(p, dw, dh, v, h, tile_w, tile_h, ncp); break;
    case 3: resize_chain_kernel<K, 3><<<grid, 256, lds, s>>>(p, dw, dh, v, h, tile_w, tile_h, ncp); break;
    case 4: resize_chain_kernel<K, 4><<<grid, 256, lds, s>>>(p, dw, dh, v, h, tile_w, tile_h, ncp); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_resize_chain(const ResizePlan &r, const ChainProgram &p, TapsDev v, TapsDev h, hipStream_t s)
{
    if (r.dw == 0 || r.dh == 0) return hipSuccess;
    if (r.planes < 1 || r.planes > KC_CHAIN_MAX_BATCH || p.n_ops < 1 || p.n_ops > KC_CHAIN_MAX_OPS) return hipErrorInvalidValue;
    if (r.tile_w % 4 != 0 || r.tile_w > 1024 || 256u % (r.tile_w / 4) != 0 || r.tile_h > 64) return hipErrorInvalidValue;
    switch (p.n_in) {
    case 1: return launch_resize_chain_k<1>(p, r.grid, r.lds, s, r.dw, r.dh, v, h, r.tile_w, r.tile_h, r.ncp);
    case 2: return launch_resize_chain_k<2>(p, r.grid, r.lds, s, r.dw, r.dh, v, h, r.tile_w, r.tile_h, r.ncp);
    case 3: return launch_resize_chain_k<3>(p, r.grid, r.lds, s, r.dw, r.dh, v, h, r.tile_w, r.tile_h, r.ncp);
    case 4: return launch_resize_chain_k<4>(p, r.grid, r.lds, s, r.dw, r.dh, v, h, r.tile_w, r.tile_h, r.ncp);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace kc
