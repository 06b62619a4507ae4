// The wave-uniform down-samplers (more than 8 taps on both axes): resize_down_kernel, any windows; resize_poly_kernel and
// resize_poly2_kernel, integer ratios, whose border rows run as resize_down_kernel's tiles.  They share no helper with the
// tiled resamplers of resize_tile.hip besides the clamp; the wave-private third form is down2.hip.
#include "kc_internal.hpp"

namespace kc {

typedef float f4 __attribute__((ext_vector_type(4)));

#include "resample.inc"  // clamp01_nan_passthrough: shared by resize_tile.hip and resize_down.hip

// Down-sampling (more than 8 taps on BOTH axes), second form.  resize_wide_kernel's vertical pass gathers every output
// row's whole window from global memory (25 16-byte loads per row and column quad for Lanczos3 4:1) with per-lane tap
// look-ups; here the unit of work is wave-uniform instead:
//   vertical pass   a WAVE owns R adjacent tile rows and 64 column quads.  It walks the union of the R windows once,
//                   four source rows per trip (one 16-byte load per lane and row), and feeds each row into every sum
//                   whose window contains it.  Which sums those are depends only on the rows, not on the lane, so the
//                   tests are scalar branches on scalar-loaded window bounds and the weights arrive as scalar loads from
//                   the tap table: (taps + (R - 1) ratio) / R loads per output row instead of taps, no tap staging, no
//                   per-lane control.  Each sum still receives its taps in ascending order: same roundings.
//   horizontal pass a lane owns one output column for four tile rows at a time: one weight read and one swizzled
//                   index per tap serve four sums.
// Rows whose windows are far apart (the wrapped rows of a row band) fall back to one row per walk.
// What bounds it (profiles/r02_down_kernel.md): the windows of neighbouring row groups overlap, the overlap is re-read
// by another wave several trips later and by then has left L2 -- 88 % of this pass's reads miss it -- so the pass runs at
// the fabric's rate on (taps + (R - 1) ratio) / (R ratio) times the plane.
template <int R>
static __device__ __forceinline__ void resize_down_rows(const f4 *__restrict__ src4, uint32_t sp4, float *tmp,
                                                        uint32_t row_floats, uint32_t nq, uint32_t ty0, uint32_t th,
                                                        uint32_t y0, const TapsDev &V, uint32_t lane)
{
    uint32_t left[R], cnt[R];
    const float *w[R];
    uint32_t smin = 0xFFFFFFFFu, smax = 0u;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const bool on = ty0 + k < th;
        const uint32_t y = y0 + (on ? ty0 + k : ty0);
        left[k] = V.left[y];
        cnt[k] = on ? V.count[y] : 0u;
        w[k] = V.w + (size_t)y * V.stride;
        if (on) {
            smin = min(smin, left[k]);
            smax = max(smax, left[k] + cnt[k]);
        }
    }
    for (uint32_t qb = 0; qb < nq; qb += 64u) {
        const uint32_t q = min(qb + lane, nq - 1u);
        const f4 *col = src4 + q;
        f4 acc[R];
#pragma unroll
        for (int k = 0; k < R; ++k) acc[k] = f4{ 0.0f, 0.0f, 0.0f, 0.0f };
        for (uint32_t s0 = smin; s0 < smax; s0 += 4u) {
            f4 p[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) p[u] = col[(size_t)min(s0 + u, smax - 1u) * sp4];
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const uint32_t j0 = s0 - left[k];  // wraps for rows above the window
                if (s0 >= left[k] && j0 + 3u < cnt[k]) {
                    const float w0 = w[k][j0], w1 = w[k][j0 + 1u], w2 = w[k][j0 + 2u], w3 = w[k][j0 + 3u];
                    acc[k] += p[0] * w0;
                    acc[k] += p[1] * w1;
                    acc[k] += p[2] * w2;
                    acc[k] += p[3] * w3;
                } else if (s0 + 3u >= left[k] && s0 < left[k] + cnt[k]) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const uint32_t j = j0 + (uint32_t)u;
                        if (j < cnt[k]) acc[k] += p[u] * w[k][j];  // j wraps to a huge value above the window
                    }
                }
            }
        }
        if (qb + lane < nq) {
#pragma unroll
            for (int k = 0; k < R; ++k)
                if (ty0 + k < th) {
                    float *o = tmp + (ty0 + k) * row_floats + 4u * q + (q >> 3);  // a quad never straddles a multiple of 32
                    o[0] = acc[k].x;
                    o[1] = acc[k].y;
                    o[2] = acc[k].z;
                    o[3] = acc[k].w;
                }
        }
    }
}

// The strip's horizontal taps, staged once per workgroup (every wave of it works on the same output columns).
struct DownStrip {
    uint32_t x0, tw, c0, nq, row_floats, hsp;
    float *tmp;
    uint32_t *hl, *hn;
    float *hw;
};

static __device__ __forceinline__ DownStrip resize_down_stage(float *lds, const TapsDev &H, uint32_t dw, uint32_t tile_w,
                                                              uint32_t tmp_rows, uint32_t ncp, uint32_t bx)
{
    DownStrip S;
    S.x0 = bx * tile_w;
    const uint32_t x1 = min(S.x0 + tile_w, dw);
    S.tw = x1 - S.x0;
    S.c0 = H.left[S.x0] & ~3u;
    S.nq = (H.left[x1 - 1] + H.count[x1 - 1] - S.c0 + 3u) / 4u;  // <= ncp / 4 (host-checked)
    S.row_floats = KC_DOWN_ROW_FLOATS;  // a constant: the horizontal pass addresses its four rows with immediate offsets
    S.hsp = H.stride | 1u;  // odd pitch: the lanes' weight rows start on different banks
    S.tmp = lds;
    S.hl = reinterpret_cast<uint32_t *>(lds + tmp_rows * S.row_floats);
    S.hn = S.hl + tile_w;
    S.hw = reinterpret_cast<float *>(S.hn + tile_w);  // tile_w x hsp
    for (uint32_t i = threadIdx.x; i < S.tw; i += 256u) {
        S.hl[i] = H.left[S.x0 + i] - S.c0;
        S.hn[i] = H.count[S.x0 + i];
    }
    for (uint32_t i = threadIdx.x; i < S.tw * H.stride; i += 256u) {
        const uint32_t x = i / H.stride, j = i - x * H.stride;
        S.hw[x * S.hsp + j] = H.w[(size_t)S.x0 * H.stride + i];
    }
    return S;
}

// The same for ONE wave (resize_poly_kernel's band waves, each with a strip of its own): `lds` is the wave's own area -- four
// intermediate rows, then the taps -- filled by its 64 lanes; the caller orders it with a wave barrier.
static __device__ __forceinline__ DownStrip resize_down_stage_wave(float *lds, const TapsDev &H, uint32_t dw, uint32_t tile_w, uint32_t bx,
                                                                   uint32_t lane)
{
    DownStrip S;
    S.x0 = bx * tile_w;
    const uint32_t x1 = min(S.x0 + tile_w, dw);
    S.tw = x1 - S.x0;
    S.c0 = H.left[S.x0] & ~3u;
    S.nq = (H.left[x1 - 1] + H.count[x1 - 1] - S.c0 + 3u) / 4u;  // <= 64 (host-checked)
    S.row_floats = KC_DOWN_ROW_FLOATS;
    S.hsp = H.stride | 1u;
    S.tmp = lds;
    S.hl = reinterpret_cast<uint32_t *>(lds + 4u * S.row_floats);
    S.hn = S.hl + tile_w;
    S.hw = reinterpret_cast<float *>(S.hn + tile_w);  // tile_w x hsp
    for (uint32_t i = lane; i < S.tw; i += 64u) {
        S.hl[i] = H.left[S.x0 + i] - S.c0;
        S.hn[i] = H.count[S.x0 + i];
    }
    for (uint32_t i = lane; i < S.tw * H.stride; i += 64u) {
        const uint32_t x = i / H.stride, j = i - x * H.stride;
        S.hw[x * S.hsp + j] = H.w[(size_t)S.x0 * H.stride + i];
    }
    return S;
}

// Horizontal pass of four intermediate rows (row, row + row_floats, ...) for this lane's output column.
static __device__ __forceinline__ void resize_down_hrows(const DownStrip &S, const float *row, uint32_t lane, float *dst_row,
                                                         uint32_t dpitch, uint32_t nrows)
{
    const uint32_t n = S.hn[lane], h0 = S.hl[lane];
    const float *w = S.hw + lane * S.hsp;
    // rows 0, 1 and rows 2, 3 as pairs: one packed multiply and add per pair and tap
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 t01 = { 0.0f, 0.0f }, t23 = { 0.0f, 0.0f };
    // Every column of the strip has the same number of taps, a multiple of 4 (the interior of an integer-ratio resample):
    // no tap needs clamping or masking.
    const uint32_t nu = (uint32_t)__builtin_amdgcn_readfirstlane((int)n);
    if ((nu & 3u) == 0u && __builtin_amdgcn_ballot_w64(n != nu) == 0ull) {
        for (uint32_t j0 = 0; j0 < nu; j0 += 4u) {
            f2 p01[4], p23[4];
            float wt[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t idx = h0 + j0 + u;
                const float *v = row + idx + (idx >> 5);
                wt[u] = w[j0 + u];
                p01[u] = f2{ v[0], v[KC_DOWN_ROW_FLOATS] };
                p23[u] = f2{ v[2 * KC_DOWN_ROW_FLOATS], v[3 * KC_DOWN_ROW_FLOATS] };
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                t01 += p01[u] * wt[u];
                t23 += p23[u] * wt[u];
            }
        }
    } else {
        for (uint32_t j0 = 0; j0 < n; j0 += 4u) {
            f2 p01[4], p23[4];
            float wt[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t jj = min(j0 + u, n - 1u);
                const uint32_t idx = h0 + jj;
                const float *v = row + idx + (idx >> 5);
                wt[u] = w[jj];
                p01[u] = f2{ v[0], v[KC_DOWN_ROW_FLOATS] };
                p23[u] = f2{ v[2 * KC_DOWN_ROW_FLOATS], v[3 * KC_DOWN_ROW_FLOATS] };
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                // a tap that does not exist contributes -0.0, which leaves every sum unchanged
                const bool live = j0 + u < n;
                t01 += live ? p01[u] * wt[u] : f2{ -0.0f, -0.0f };
                t23 += live ? p23[u] * wt[u] : f2{ -0.0f, -0.0f };
            }
        }
    }
    const float t[4] = { t01.x, t01.y, t23.x, t23.y };
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if ((uint32_t)r < nrows) dst_row[(size_t)r * dpitch + S.x0 + lane] = clamp01_nan_passthrough(t[r]);
}

// One tile of 4 R rows at y0 (th of them exist): the general form, any windows.  Called by all four waves.
template <int R>
static __device__ __forceinline__ void resize_down_tile(const DownStrip &S, const float *__restrict__ src, uint32_t spitch,
                                                        float *__restrict__ dst, uint32_t dpitch, uint32_t y0, uint32_t th,
                                                        const TapsDev &V, uint32_t wave, uint32_t lane)
{
    const f4 *src4 = reinterpret_cast<const f4 *>(src + S.c0);
    {
        const uint32_t ty0 = wave * R;
        // the union of the wave's windows, against the windows themselves
        uint32_t lo = 0xFFFFFFFFu, hi = 0u, sum = 0u;
        for (uint32_t k = 0; k < R && ty0 + k < th; ++k) {
            const uint32_t l = V.left[y0 + ty0 + k], n = V.count[y0 + ty0 + k];
            lo = min(lo, l);
            hi = max(hi, l + n);
            sum += n;
        }
        if (hi - lo <= sum) {
            resize_down_rows<R>(src4, spitch / 4u, S.tmp, S.row_floats, S.nq, ty0, th, y0, V, lane);
        } else {
            for (uint32_t k = 0; k < R && ty0 + k < th; ++k)
                resize_down_rows<1>(src4, spitch / 4u, S.tmp, S.row_floats, S.nq, ty0 + k, th, y0, V, lane);
        }
    }
    __syncthreads();
    if (lane < S.tw)
        for (uint32_t tb = wave * 4u; tb < th; tb += 16u)
            resize_down_hrows(S, S.tmp + tb * S.row_floats, lane, dst + (size_t)(y0 + tb) * dpitch, dpitch, th - tb);
}

template <int R>  // tile rows per wave: the tile is 4 R rows high
__global__ __launch_bounds__(256) void resize_down_kernel(const ResizePlanes P, uint32_t dw, uint32_t dh, TapsDev V,
                                                          TapsDev H, uint32_t tile_w, uint32_t ncp)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr uint32_t tile_h = 4u * R;
    const DownStrip S = resize_down_stage(lds, H, dw, tile_w, tile_h, ncp, blockIdx.x);
    const uint32_t y0 = blockIdx.y * tile_h, th = min(y0 + tile_h, dh) - y0;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    resize_down_tile<R>(S, P.src[blockIdx.z], P.spitch[blockIdx.z], P.dst[blockIdx.z], P.dpitch[blockIdx.z], y0, th, V, wave,
                        threadIdx.x & 63u);
}

// Integer-ratio down-sampling (4096 -> 1024, -> 512, -> 2048 ...): away from the image border every output row has the
// same n = A * RT weights and its window starts RT source rows below its neighbour's (the host checks this bit for bit,
// TapsHost::reg_*).  A wave then STREAMS a band of 12 such rows: RT source rows per trip; the sum of "age" a (the row
// whose window began a trips ago) receives its taps a RT .. a RT + RT - 1 from them; after the trip the oldest sum is
// complete, goes to a four-row LDS ring and the sums move up one age.  No window test, no weight fetch (the A * RT weights
// sit in scalar registers), every source row of the band is loaded once, and after each four finished rows the wave runs the
// horizontal pass on its ring by itself: no barrier after the tap staging.  Same taps in the same order: same roundings.
// Rows near the border (and what does not fill a band) are tiles of the general form, run by the launch's last workgroups.
// Which band wave sits where (round 4): the four waves of a workgroup are four NEIGHBOURING STRIPS of one band (their windows
// share halo columns: one L1), each with its strip's taps staged in LDS by itself, and workgroup id % 8 -- the XCD -- works
// through the k-th eighth of the bands one whole band after the other (a band and the next one share A - 1 trips of rows: one
// L2; every XCD streams a contiguous eighth of the plane).  The bare access pattern takes 12.9 us like this against 18.8 with
// four bands of one strip per workgroup (profiles/tile_read_bench.hip), the kernels 8 - 20 % less.  (PolyBands: kc_internal.hpp)


template <int A, int RT>
__global__ __launch_bounds__(256) void resize_poly_kernel(const ResizePlanes P, uint32_t dw, uint32_t dh, TapsDev V,
                                                          TapsDev H, uint32_t tile_w, uint32_t ncp, PolyBands B)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const float *__restrict__ src = P.src[blockIdx.z];
    float *__restrict__ dst = P.dst[blockIdx.z];
    const uint32_t spitch = P.spitch[blockIdx.z], dpitch = P.dpitch[blockIdx.z];
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t sp4 = spitch / 4u;
    DownStrip S;
    uint32_t yf;
    f4 pn[RT];
    const f4 *col;
    // ---- four strips of one band per workgroup, the bands dealt to the XCDs in eighths (profiles/r04_poly_weights.md 5a: the
    // halo columns of neighbouring strips meet in one L1, a band and the next one in one L2) ----
    if (blockIdx.x >= 8u * B.xper) {
        const uint32_t g = blockIdx.x - 8u * B.xper, t = g / B.gx;
        S = resize_down_stage(lds, H, dw, tile_w, 16u, ncp, g - t * B.gx);
        resize_down_tile<4>(S, src, spitch, dst, dpitch, B.ty0[t], B.th[t], V, wave, lane);
        return;
    }
    const uint32_t tile = (blockIdx.x & 7u) * B.xper + (blockIdx.x >> 3);
    if (tile >= B.n_band_wgs) return;
    const uint32_t bi = tile / B.n_sq, strip = (tile - bi * B.n_sq) * 4u + wave;
    if (strip >= B.gx) return;  // (no workgroup barrier on this path)
    yf = B.ya + B.rows * bi;
    // the band's first rows are requested before the taps are staged: both are in flight together
    {
        const uint32_t x0 = strip * tile_w, x1 = min(x0 + tile_w, dw), c0 = H.left[x0] & ~3u;
        const uint32_t nq = (H.left[x1 - 1] + H.count[x1 - 1] - c0 + 3u) / 4u;
        col = reinterpret_cast<const f4 *>(src + c0) + min(lane, nq - 1u) + (size_t)V.left[yf] * sp4;
    }
#pragma unroll
    for (int u = 0; u < RT; ++u) pn[u] = col[(size_t)u * sp4];
    S = resize_down_stage_wave(lds + wave * B.wave_floats, H, dw, tile_w, strip, lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t ROWS = min(B.rows, B.yb - yf);
    const bool q_ok = lane < S.nq;
    const uint32_t q = min(lane, S.nq - 1u);
    // The A RT weights, two to a VECTOR register pair (the same values in every lane); either half of a pair is broadcast to both
    // lanes of a packed multiply by op_sel, at no cost.  As scalar registers -- rounds 2 and 3 -- the compiler wanted every
    // weight as an SGPR PAIR (w, w) for v_pk_mul_f32: 96 scalar registers at ratio 8, which do not exist, so it parked them in
    // the lanes of two vector registers and fetched each pair back with two v_readlane and a wait state before its multiply:
    // 112 of the 304 vector instructions of a trip (208 now; Gaussian 8:1 30.4 -> 27.7 us, Lanczos3 4:1 22.2 -> 21.1:
    // profiles/r04_poly_weights.md).
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 Wp[A][RT / 2];
#pragma unroll
    for (int a = 0; a < A; ++a)
#pragma unroll
        for (int u = 0; u < RT; u += 2)
            Wp[a][u / 2] = f2{ V.w[(size_t)B.ya * V.stride + a * RT + u], V.w[(size_t)B.ya * V.stride + a * RT + u + 1] };
    auto mad = [&](f4 &sum, const f4 &p, int a, int u) {
        // (the empty statement keeps the pair where it is and the broadcast inside the loop: hoisted out of it, the 48 splats
        // would be 96 more registers -- tried: 303 VGPRs, slower)
        asm volatile("" : "+v"(Wp[a][u / 2]));
        const f2 wp = Wp[a][u / 2];
        const f2 w2 = (u & 1) ? __builtin_shufflevector(wp, wp, 1, 1) : __builtin_shufflevector(wp, wp, 0, 0);
        const f2 lo = f2{ p.x, p.y } * w2, hi = f2{ p.z, p.w } * w2;
        sum = f4{ sum.x + lo.x, sum.y + lo.y, sum.z + hi.x, sum.w + hi.y };
    };
    float *ring = S.tmp;
    float *ringq = ring + 4u * q + (q >> 3);  // swizzled: a quad never straddles a multiple of 32
    f4 acc[A];
#pragma unroll
    for (int a = 0; a < A; ++a) acc[a] = f4{ 0.0f, 0.0f, 0.0f, 0.0f };
    const uint32_t TRIPS = ROWS + A - 1;
    for (uint32_t c = 0; c < TRIPS; ++c) {
        f4 p[RT];
#pragma unroll
        for (int u = 0; u < RT; ++u) p[u] = pn[u];
        if (c + 1u < TRIPS) {
#pragma unroll
            for (int u = 0; u < RT; ++u) pn[u] = col[(size_t)((c + 1u) * RT + u) * sp4];
        }
        // age a holds row c - a of the band
        if (c >= (uint32_t)(A - 1) && c < ROWS) {
#pragma unroll
            for (int u = 0; u < RT; ++u)
#pragma unroll
                for (int a = 0; a < A; ++a) mad(acc[a], p[u], a, u);
        } else {
#pragma unroll
            for (int a = 0; a < A; ++a)
                if (c >= (uint32_t)a && c - (uint32_t)a < ROWS) {
#pragma unroll
                    for (int u = 0; u < RT; ++u) mad(acc[a], p[u], a, u);
                }
        }
        if (c >= (uint32_t)(A - 1)) {
            const uint32_t k = c - (uint32_t)(A - 1);  // this row of the band is complete
            if (q_ok) {
                float *o = ringq + (k & 3u) * S.row_floats;
                o[0] = acc[A - 1].x;
                o[1] = acc[A - 1].y;
                o[2] = acc[A - 1].z;
                o[3] = acc[A - 1].w;
            }
            if ((k & 3u) == 3u) {
                // the ring is this wave's own: its lanes' writes only have to be ordered before its lanes' reads
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (lane < S.tw) resize_down_hrows(S, ring, lane, dst + (size_t)(yf + k - 3u) * dpitch, dpitch, 4u);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
#pragma unroll
        for (int a = A - 1; a > 0; --a) acc[a] = acc[a - 1];
        acc[0] = f4{ 0.0f, 0.0f, 0.0f, 0.0f };
    }
}

hipError_t launch_resize_down(const ResizePlan &r, const ResizePlanes &p, TapsDev v, TapsDev h, hipStream_t s)
{
    if (r.dw == 0 || r.dh == 0) return hipSuccess;
    if (r.planes < 1 || r.planes > 4) return hipErrorInvalidValue;
    if (r.tile_w == 0 || r.tile_w > 64 || (r.tile_h != 16 && r.tile_h != 32) || r.ncp % 4 != 0 || r.ncp > 256) return hipErrorInvalidValue;
    if (r.tile_h == 16)
        resize_down_kernel<4><<<r.grid, 256, r.lds, s>>>(p, r.dw, r.dh, v, h, r.tile_w, r.ncp);
    else
        resize_down_kernel<8><<<r.grid, 256, r.lds, s>>>(p, r.dw, r.dh, v, h, r.tile_w, r.ncp);
    return hipGetLastError();
}

template <int A>
static void launch_resize_poly_a(dim3 grid, size_t lds, hipStream_t s, uint32_t rt, const ResizePlanes &p, uint32_t dw, uint32_t dh,
                                 TapsDev v, TapsDev h, uint32_t tile_w, uint32_t ncp, const PolyBands &b)
{
    if (rt == 2) resize_poly_kernel<A, 2><<<grid, 256, lds, s>>>(p, dw, dh, v, h, tile_w, ncp, b);
    else if (rt == 4) resize_poly_kernel<A, 4><<<grid, 256, lds, s>>>(p, dw, dh, v, h, tile_w, ncp, b);
    else resize_poly_kernel<A, 8><<<grid, 256, lds, s>>>(p, dw, dh, v, h, tile_w, ncp, b);
}

// resize_poly_kernel: bands of the vertical table's regular rows (`ages` x `ratio` taps each, windows `ratio` apart, equal
// weights), the rows above and below them as border tiles
hipError_t launch_resize_poly(const ResizePlan &r, const ResizePlanes &p, TapsDev v, TapsDev h, hipStream_t s)
{
    const PolyBands &b = r.poly;
    if (r.dw == 0 || r.dh == 0) return hipSuccess;
    if (r.planes < 1 || r.planes > 4) return hipErrorInvalidValue;
    if (r.tile_w == 0 || r.tile_w > 64 || r.ncp % 4 != 0 || r.ncp > 256 || b.ya > b.yb || b.yb > r.dh) return hipErrorInvalidValue;
    if ((r.ages != 2 && r.ages != 4 && r.ages != 6) || (r.ratio != 2 && r.ratio != 4 && r.ratio != 8)) return hipErrorInvalidValue;
    if (r.n_border > 4 || r.lds > 64u * 1024u) return hipErrorInvalidValue;
    if (r.ages == 2) launch_resize_poly_a<2>(r.grid, r.lds, s, r.ratio, p, r.dw, r.dh, v, h, r.tile_w, r.ncp, b);
    else if (r.ages == 4) launch_resize_poly_a<4>(r.grid, r.lds, s, r.ratio, p, r.dw, r.dh, v, h, r.tile_w, r.ncp, b);
    else launch_resize_poly_a<6>(r.grid, r.lds, s, r.ratio, p, r.dw, r.dh, v, h, r.tile_w, r.ncp, b);
    return hipGetLastError();
}

// Integer-ratio down-sampling, two waves to a band's strip (round 4).
//
// resize_poly_kernel's geometry is what the memory system likes -- 256-column windows, one wave-wide row request per source row
// (profiles/tile_read_bench.hip: the bare access pattern of Gaussian 4096^2 -> 512^2 takes 15.6 us) -- but a band wave of its
// lives 27 us: a launch has about one wave per SIMD, and that wave's own instruction stream (the trips' packed arithmetic, then
// the horizontal pass) is the critical path.  Narrower strips give more and lighter waves and lose it all again on the wider
// halo (128-column windows: the bare pattern alone is 22.6 us).  So the strip stays and its work is cut in two along the
// columns: waves 2 p and 2 p + 1 of a workgroup take the left and right 128 columns of pair p's window as 8-byte lanes (half
// the arithmetic per trip each), both write their halves of each finished row into ONE ring in LDS, and after every fourth row
// the two share the horizontal pass -- one output pixel per lane, (row, column) = pair lane / strip width -- behind a single
// s_barrier (the ring holds eight rows, so nobody has to wait for the other's reads before writing on).  The barrier is a bare
// s_waitcnt lgkmcnt(0) + s_barrier: the rows requested for the next trips stay in flight across it.  Both pairs of a workgroup
// work on the same band (same number of trips and barriers).  Same taps in the same order: same roundings.
// Rows outside the regular range run as resize_down_kernel tiles in the launch's last workgroups, as before.  (Poly2Bands and
// KC_POLY2_RING_PITCH: kc_internal.hpp)
#ifndef KC_POLY2_NB
#define KC_POLY2_NB 1  // trips of rows in flight beyond the one in use: 1 / 2 / 3 measure the same or worse (profiles/r04_poly2_sweep.txt)
#endif
// (LDS writes of this wave done, then the workgroup's barrier; global loads stay in flight)
#define KC_POLY2_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

template <int A, int RT>
__global__ __launch_bounds__(256) void resize_poly2_kernel(const ResizePlanes P, uint32_t dw, uint32_t dh, TapsDev V, TapsDev H,
                                                           Poly2Bands B, uint32_t pair_floats, XcdOrder X)
{
    typedef float f2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const float *__restrict__ src = P.src[blockIdx.z];
    float *__restrict__ dst = P.dst[blockIdx.z];
    const uint32_t spitch = P.spitch[blockIdx.z], dpitch = P.dpitch[blockIdx.z];
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t wg = blockIdx.x;
    if (X.per) {
        // Workgroup id % 8 is the XCD.  XCD k takes the k-th eighth of the band workgroups in BAND-major order: whole bands, one
        // after the other -- the strips of a band (which share their halo columns) and the next band (which shares 40 of its 136
        // source rows at ratio 8) meet in one L2 while they are there, and every XCD streams one contiguous eighth of the plane.
        // (profiles/tile_read_bench.hip, the loads and the vertical arithmetic alone: 14.1 us like this, 22.2 in plain order;
        // KC_POLY2_XCD=2: the eighths in strip-major order, a strip pair with all its bands, as resize_poly_kernel has them)
        if (wg < 8u * X.per) {
            const uint32_t tile = (wg & 7u) * X.per + (wg >> 3);
            if (tile >= X.n) return;
            if (X.gy) {
                const uint32_t wx = __umulhi(tile, X.magic);
                wg = (tile - wx * X.gy) * B.n_wgx + wx;
            } else {
                wg = tile;
            }
        } else {
            wg = wg - 8u * X.per + B.n_band_wgs;
        }
    }
    if (wg >= B.n_band_wgs) {
        // rows near the border: the general form, all four waves on one tile
        const uint32_t g = wg - B.n_band_wgs;
        const uint32_t t = g / B.gen_gx, bx = g - t * B.gen_gx;
        const DownStrip S = resize_down_stage(lds, H, dw, B.gen_tw, 16u, B.gen_ncp, bx);
        resize_down_tile<4>(S, src, spitch, dst, dpitch, B.ty0[t], B.th[t], V, wave, lane);
        return;
    }
    // ---- a band workgroup: strips 2 wgx, 2 wgx + 1 of band `band` (an odd strip count: the last strip twice, same values) ----
    const uint32_t band = wg / B.n_wgx, wgx = wg - band * B.n_wgx;
    const uint32_t pair = wave >> 1, half = wave & 1u;
    const uint32_t strip = min(2u * wgx + pair, B.n_strips - 1u);
    const uint32_t x0 = strip * B.tw, x1 = min(x0 + B.tw, dw), tw = x1 - x0;
    const uint32_t c0 = H.left[x0] & ~3u;
    const uint32_t ncols = H.left[x1 - 1] + H.count[x1 - 1] - c0;  // <= 256 (host-checked)
    const uint32_t npairs = (ncols + 1u) / 2u;
    float *ring = lds + pair * pair_floats;                        // 8 rows x KC_POLY2_RING_PITCH
    uint32_t *hl = reinterpret_cast<uint32_t *>(ring + 8u * KC_POLY2_RING_PITCH);
    uint32_t *hn = hl + 128;
    float *hw = reinterpret_cast<float *>(hn + 128);               // tw x hsp
    const uint32_t hsp = H.stride | 1u;  // odd pitch: the lanes' weight rows start on different banks
    const uint32_t yf = B.ya + B.rows * band;
    const uint32_t ROWS = min(B.rows, B.yb - yf);
    const uint32_t sp2 = spitch / 2u;
    const uint32_t pl = half * 64u + lane;  // lane of the pair
    const bool p_ok = pl < npairs;
    const uint32_t pq = min(pl, npairs - 1u);
    // (a column pair's second column may be the first one past the window: inside the row or its padding, never past the pitch)
    const f2 *col = reinterpret_cast<const f2 *>(src + c0 + (size_t)V.left[yf] * spitch) + pq;
    // KC_POLY2_NB trips of rows in flight or in use: buffer b holds trips b, b + NB, ... -- named statically, so that the wait for
    // a trip's rows leaves the younger trips' loads in flight
    constexpr int NB = KC_POLY2_NB;
    const uint32_t TRIPS = ROWS + A - 1;
    f2 pb[NB][RT];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int u = 0; u < RT; ++u) pb[b][u] = col[(size_t)(min((uint32_t)b, TRIPS - 1u) * RT + u) * sp2];
    // the pair's copy of its strip's horizontal taps (in flight together with the first rows)
    for (uint32_t i = pl; i < tw; i += 128u) {
        hl[i] = H.left[x0 + i] - c0;
        hn[i] = H.count[x0 + i];
    }
    for (uint32_t i = pl; i < tw * H.stride; i += 128u) {
        const uint32_t x = i / H.stride, j = i - x * H.stride;
        hw[x * hsp + j] = H.w[(size_t)x0 * H.stride + i];
    }
    // the A RT weights, two to a vector register pair, broadcast by op_sel inside the loop (as in resize_poly_kernel)
    f2 Wp[A][RT / 2];
#pragma unroll
    for (int a = 0; a < A; ++a)
#pragma unroll
        for (int u = 0; u < RT; u += 2)
            Wp[a][u / 2] = f2{ V.w[(size_t)B.ya * V.stride + a * RT + u], V.w[(size_t)B.ya * V.stride + a * RT + u + 1] };
    auto mad = [&](f2 &sum, const f2 &p, int a, int u) {
        asm volatile("" : "+v"(Wp[a][u / 2]));
        const f2 wp = Wp[a][u / 2];
        sum += p * ((u & 1) ? __builtin_shufflevector(wp, wp, 1, 1) : __builtin_shufflevector(wp, wp, 0, 0));
    };
    const uint32_t rj = 2u * pq + ((2u * pq) >> 5);  // where this lane's pair goes in a ring row (a pair never straddles a pad)
    // which pixel of four finished rows this lane takes in the horizontal pass: all four rows at once for strips of up to 32
    // columns, two for up to 64, one row of up to 128 columns at a time beyond
    const uint32_t rows_per_pass = tw <= 32u ? 4u : tw <= 64u ? 2u : 1u;  // (uniform)
    const uint32_t hx = rows_per_pass == 4u ? (pl & 31u) : rows_per_pass == 2u ? (pl & 63u) : pl;
    const uint32_t hr = rows_per_pass == 4u ? (pl >> 5) : rows_per_pass == 2u ? (pl >> 6) : 0u;
    const bool h_ok = hx < tw;
    const uint32_t hxs = h_ok ? hx : 0u;
    f2 acc[A];
#pragma unroll
    for (int a = 0; a < A; ++a) acc[a] = f2{ 0.0f, 0.0f };
    KC_POLY2_BARRIER();  // the taps are staged
    const uint32_t hcount = hn[hxs], h0 = hl[hxs];
    const float *hwt = hw + hxs * hsp;
    const uint32_t nu = (uint32_t)__builtin_amdgcn_readfirstlane((int)hcount);
    const bool uniform = (nu & 3u) == 0u && __builtin_amdgcn_ballot_w64(hcount != nu) == 0ull;
    for (uint32_t cb = 0; cb < TRIPS; cb += NB) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const uint32_t c = cb + b;  // (up to NB - 1 trips past the last one do nothing: leaving the loop from its middle would join
                                    // paths with different numbers of loads in flight, and the waits would be for all of them)
        f2 (&p)[RT] = pb[b];
        // age a holds row c - a of the band
        if (c >= (uint32_t)(A - 1) && c < ROWS) {
#pragma unroll
            for (int u = 0; u < RT; ++u)
#pragma unroll
                for (int a = 0; a < A; ++a) mad(acc[a], p[u], a, u);
        } else {
#pragma unroll
            for (int a = 0; a < A; ++a)
                if (c >= (uint32_t)a && c - (uint32_t)a < ROWS) {
#pragma unroll
                    for (int u = 0; u < RT; ++u) mad(acc[a], p[u], a, u);
                }
        }
        // the buffer's next trip (past the last one: that one again, so that the number of loads in flight is the same on every path)
        {
            const uint32_t cn = min(c + (uint32_t)NB, TRIPS - 1u);
#pragma unroll
            for (int u = 0; u < RT; ++u) {
                asm volatile("" : "+v"(p[u]));  // (after this trip's last use of the row, not in a register of its own)
                p[u] = col[(size_t)(cn * RT + u) * sp2];
            }
        }
        if (c >= (uint32_t)(A - 1) && c < TRIPS) {
            const uint32_t k = c - (uint32_t)(A - 1);  // this row of the band is complete
            if (p_ok) {
                float *o = ring + (k & 7u) * KC_POLY2_RING_PITCH + rj;
                o[0] = acc[A - 1].x;
                o[1] = acc[A - 1].y;
            }
            if ((k & 3u) == 3u) {
                KC_POLY2_BARRIER();  // both halves of the four rows are in the ring (and everybody is done with the four before)
                const float *rows4 = ring + (k & 4u) * KC_POLY2_RING_PITCH;
                for (uint32_t r0 = 0; r0 < 4u; r0 += rows_per_pass) {
                    const float *row = rows4 + (r0 + hr) * KC_POLY2_RING_PITCH;
                    float t = 0.0f;
                    if (uniform) {
                        for (uint32_t j0 = 0; j0 < nu; j0 += 4u) {
                            float pv[4], wt[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const uint32_t idx = h0 + j0 + u;
                                pv[u] = row[idx + (idx >> 5)];
                                wt[u] = hwt[j0 + u];
                            }
#pragma unroll
                            for (int u = 0; u < 4; ++u) t += pv[u] * wt[u];
                        }
                    } else {
                        for (uint32_t j0 = 0; j0 < hcount; j0 += 4u) {
                            float pv[4], wt[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const uint32_t jj = min(j0 + u, hcount - 1u);
                                const uint32_t idx = h0 + jj;
                                pv[u] = row[idx + (idx >> 5)];
                                wt[u] = hwt[jj];
                            }
#pragma unroll
                            for (int u = 0; u < 4; ++u) t += j0 + u < hcount ? pv[u] * wt[u] : -0.0f;  // -0.0 leaves the sum as it is
                        }
                    }
                    if (h_ok) dst[(size_t)(yf + k - 3u + r0 + hr) * dpitch + x0 + hx] = clamp01_nan_passthrough(t);
                }
            }
        }
#pragma unroll
        for (int a = A - 1; a > 0; --a) acc[a] = acc[a - 1];
        acc[0] = f2{ 0.0f, 0.0f };
      }
    }
}

template <int A>
static void launch_resize_poly2_a(dim3 grid, size_t lds, hipStream_t s, uint32_t rt, const ResizePlanes &p, uint32_t dw, uint32_t dh,
                                  TapsDev v, TapsDev h, const Poly2Bands &b, uint32_t pair_floats, const XcdOrder &x)
{
    if (rt == 2) resize_poly2_kernel<A, 2><<<grid, 256, lds, s>>>(p, dw, dh, v, h, b, pair_floats, x);
    else if (rt == 4) resize_poly2_kernel<A, 4><<<grid, 256, lds, s>>>(p, dw, dh, v, h, b, pair_floats, x);
    else resize_poly2_kernel<A, 8><<<grid, 256, lds, s>>>(p, dw, dh, v, h, b, pair_floats, x);
}

// b.tw: output columns per band strip (host-checked: every strip's source window, from its first column rounded down to a multiple
// of 4, is at most 256 columns); b.gen_tw / b.gen_ncp: resize_down_kernel's tile for the border rows.
hipError_t launch_resize_poly2(const ResizePlan &r, const ResizePlanes &p, TapsDev v, TapsDev h, hipStream_t s)
{
    const Poly2Bands &b = r.poly2;
    if (r.dw == 0 || r.dh == 0) return hipSuccess;
    if (r.planes < 1 || r.planes > 4) return hipErrorInvalidValue;
    if (b.tw == 0 || b.tw > 128 || b.gen_tw == 0 || b.gen_tw > 64 || b.gen_ncp % 4 != 0 || b.gen_ncp > 256 || b.ya >= b.yb || b.yb > r.dh)
        return hipErrorInvalidValue;
    if ((r.ages != 2 && r.ages != 4 && r.ages != 6) || (r.ratio != 2 && r.ratio != 4 && r.ratio != 8)) return hipErrorInvalidValue;
    if (r.n_border > 6 || r.lds > 64u * 1024u) return hipErrorInvalidValue;
    if (r.ages == 2) launch_resize_poly2_a<2>(r.grid, r.lds, s, r.ratio, p, r.dw, r.dh, v, h, b, r.pair_floats, r.xcd);
    else if (r.ages == 4) launch_resize_poly2_a<4>(r.grid, r.lds, s, r.ratio, p, r.dw, r.dh, v, h, b, r.pair_floats, r.xcd);
    else launch_resize_poly2_a<6>(r.grid, r.lds, s, r.ratio, p, r.dw, r.dh, v, h, b, r.pair_floats, r.xcd);
    return hipGetLastError();
}

}  // namespace kc
