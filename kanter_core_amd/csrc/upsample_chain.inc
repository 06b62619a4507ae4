// Device body of the integer-ratio up-sampling kernels (see upsample.h for what the host has checked).
// Included inside namespace kc by upsample.hip (the interpreter-driven and the plain instantiations) and, as text, by
// the run-time specialiser (specialize.cpp: the Mix chain as straight-line code).  Needs f4, ChainProgram, UpAxis /
// UpsampleArgs.  Arithmetic per output sample is the reference's: vertical pass first, unclamped, every sum sequential
// from 0.0 and unfused; horizontal pass clamped to [0, 1] with NaN passing through (image::math::utils::clamp).
//
// Shape (profiles/tilecopy.hip, r03_tilecopy*.txt): on MI355X a 1-in-1-out stream over 4096^2 planes runs at 5.8-6.0 TB/s
// when every workgroup is SHORT-LIVED -- each thread requests its few 16-byte loads at once, computes, stores, exits --
// and at 5.0-5.5 TB/s when workgroups loop over many trips (1024 x 32 tiles: 77-79 us against 69.5 us for 1024 x 4,
// for the same 403 MB), whatever the loop does about prefetching.  So a workgroup here is ONE trip:
//   * a tile is tile_w columns x RU * (1024 / tile_w) rows (1024 x 4 for wide images); every thread owns 4 columns and RU
//     rows, and requests its RU x (K - 1) resident operands first;
//   * vertical pass, HBM (L2) -> LDS: a work item is (source column quad, chunk of rows that share a window): the
//     window's T source quads are loaded once and feed every row of the chunk.  For a wide tile that is one chunk: 34 lanes
//     of wave 0, their 4 x T weights fetched as scalars;
//   * one barrier;
//   * horizontal pass + chain: the thread's 4 columns share one window of T intermediates (T LDS reads per row), their
//     weights are T 16-byte LDS reads, no tap counts, no predication; then the chain on RU float4 and RU stores.  At ratio 2
//     the window of columns 2, 3 starts one sample after that of columns 0, 1 (T + 1 reads).
// Bit-identical to resize_chain_kernel / resize_lds_kernel: same operands, same order, same roundings.

// image::math::utils::clamp(t, 0, 1) for a t that is never -0.0 (a sum that started at +0.0): the IEEE-754-2019
// maximum / minimum (v_maximum3_f32 / v_minimum3_f32) pass a NaN through, which is what the reference's two comparisons do.
static __device__ __forceinline__ f4 up_clamp01(f4 t)
{
    const f4 zero = { 0.0f, 0.0f, 0.0f, 0.0f }, one = { 1.0f, 1.0f, 1.0f, 1.0f };
    return __builtin_elementwise_minimum(__builtin_elementwise_maximum(t, zero), one);
}

// o / ratio for o < 65536
static __device__ __forceinline__ unsigned int up_div(const UpAxis &A, unsigned int o) { return A.ratio == 1u ? o : __umulhi(o, A.magic); }

static __device__ __forceinline__ unsigned int up_class(const UpAxis &A, unsigned int o)
{
    if (o < A.b_lo) return A.ratio + o;
    if (o >= A.n_out - A.b_hi) return A.ratio + A.b_lo + (o - (A.n_out - A.b_hi));
    return o - up_div(A, o) * A.ratio;
}

// Weight tables are immutable while a kernel runs: read through the constant address space they become scalar loads
// wherever the index is wave-uniform.
typedef const float __attribute__((address_space(4))) up_cfloat;
static __device__ __forceinline__ up_cfloat *up_const(const float *p) { return (up_cfloat *)(unsigned long long)p; }

// Vertical pass of one work item = (source quad, rows of the tile that share the window u0 .. u0 + T - 1), in two halves so
// that the caller can put other requests between the loads and their use.
// Loads: unconditional, from clamped addresses (a conditional load costs a branch and a wait per tap), zeroed afterwards
// where the window leaves the source -- columns past its last one included: the row's padding is not data.
template <int T>
static __device__ __forceinline__ void up_vpass_load(const f4 *__restrict__ src4, unsigned int sp4, unsigned int sw, unsigned int sh, int sq,
                                                     int u0, f4 (&s)[T])
{
    const unsigned int sqc = (unsigned int)min(max(sq, 0), (int)((sw - 1u) >> 2));
#pragma unroll
    for (int j = 0; j < T; ++j) s[j] = src4[(size_t)(unsigned int)min(max(u0 + j, 0), (int)sh - 1) * sp4 + sqc];
}

template <int T>
static __device__ __forceinline__ void up_vpass_mask(unsigned int sw, unsigned int sh, int sq, int u0, f4 (&s)[T])
{
    const int c = 4 * sq;
    const bool x_ok = sq >= 0 && c < (int)sw, y_ok = c + 1 < (int)sw, z_ok = c + 2 < (int)sw, w_ok = c + 3 < (int)sw;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const bool row_ok = u0 + j >= 0 && u0 + j < (int)sh;
        s[j].x = row_ok && x_ok ? s[j].x : 0.0f;
        s[j].y = row_ok && x_ok && y_ok ? s[j].y : 0.0f;
        s[j].z = row_ok && x_ok && z_ok ? s[j].z : 0.0f;
        s[j].w = row_ok && x_ok && w_ok ? s[j].w : 0.0f;
    }
}

// K = inputs of the chain program (slot K - 1 is the resampled one), T = taps per axis, RU = rows per thread,
// WIDE = the tile is 1024 columns x RU rows (thread = column quad; row indices are scalars).
// prog(in, acc): the chain on RU float4; in[K - 1] holds the resampled values.
// PT: ChainProgram, or any struct with its plane members (in, in_pitch, samp_src, samp_pitch, out, out_pitch).
// NT = the launch's cache policy, compile-time (ChainProgram::nt_mask: bit k = resident input k is read nontemporal, bit 8 =
// the result is stored nontemporal; a run-time choice between the two forms of one access is merged back into the plain one
// by the compiler).
// HALF: the horizontal ratio is 2 (half quads); compile-time, so that the ratio-4-and-up form keeps its registers (the
// specialised chain kernel: 57, eight waves per SIMD).
template <int K, int T, int RU, bool WIDE, unsigned int NT, bool HALF = false, class PT, class Prog>
static __device__ __forceinline__ void upsample_chain_tile(const PT &P, const UpsampleArgs &U, float *lds, const Prog &prog)
{
    const unsigned int b = blockIdx.z;
    const unsigned int tile_w = WIDE ? 1024u : U.tile_w, ncp = U.ncp;
    const unsigned int dw = U.H.n_out, dh = U.V.n_out;
    const unsigned int col_groups = tile_w / 4u;                      // threads across one tile row
    const unsigned int row_groups = WIDE ? 1u : 256u / col_groups;    // tile rows per "u"
    const unsigned int tile_h = RU * row_groups;
    const unsigned int cg = WIDE ? threadIdx.x : threadIdx.x % col_groups;
    const unsigned int rg = WIDE ? 0u : threadIdx.x / col_groups;
    const unsigned int x0 = blockIdx.x * tile_w, x1 = min(x0 + tile_w, dw);
    const unsigned int y0 = blockIdx.y * tile_h, th = min(tile_h, dh - y0);
    const unsigned int ox = x0 + 4u * cg;  // dw is a multiple of 4 (H.ratio is): every quad is whole
    const bool active = ox < x1;

    float *tmp = lds;                // tile_h x ncp: the vertical pass' result
    float *hq = lds + tile_h * ncp;  // the H quad classes
    const int cq0 = ((int)up_div(U.H, x0) - U.H.off) >> 2;  // first source quad of the tile's window (floor; may be -1)
    const int last = (int)up_div(U.H, x1 - 1u) - U.H.off + (T - 1);  // last source column any window of the tile touches
    const unsigned int nq = (unsigned int)((last >> 2) - cq0) + 1u;  // <= ncp / 4 <= 256 (host-checked)
    const f4 *src4 = reinterpret_cast<const f4 *>(P.samp_src[b]);
    const unsigned int sp4 = P.samp_pitch[b] / 4u;
    const unsigned int sw = U.H.n_in, sh = U.V.n_in;
    up_cfloat *vc = up_const(U.V.cls);

    // R = 2 ("half quads", upsample.h): columns 0, 1 of a quad share one window and columns 2, 3 the window one sample further; one
    // interior quad class
    constexpr bool half = HALF;
    const unsigned int r4 = HALF ? 1u : U.H.ratio >> 2;
    const unsigned int n_hq4 = (r4 + U.H.qb_lo + U.H.qb_hi) * T;  // <= 256 (host-checked)
    const f4 *hq_src = reinterpret_cast<const f4 *>(U.H.qcls);
    // the resident operands of the chain (columns past the image re-read its last quad and are never stored)
    f4 in[K][RU];
    const f4 *inp[K > 1 ? K - 1 : 1];
#pragma unroll
    for (int k = 0; k < K - 1; ++k) inp[k] = reinterpret_cast<const f4 *>(P.in[b][k]) + min(ox, dw - 4u) / 4u;
    auto request = [&]() {
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const unsigned int oy = y0 + min(rg + u * row_groups, th - 1u);
#pragma unroll
            for (int k = 0; k < K - 1; ++k) {
                const f4 *a = &inp[k][(size_t)oy * P.in_pitch[b][k]];
                if ((NT >> k) & 1u) in[k][u] = __builtin_nontemporal_load(a);
                else in[k][u] = *a;
            }
        }
    };

    // ---- requests + vertical pass ----
    // Loads return in order and the compiler waits for ALL of a wave's loads wherever control flow has met, so the waves
    // with prologue work run it as one straight block: small requests (class quads, source window) first, the HBM
    // reads of the resident operands behind them, then the vertical pass waits for the small ones only.
    const bool one_chunk = WIDE && U.chunk == (unsigned int)RU && th == (unsigned int)RU;
    if (one_chunk) {
        const unsigned int wave_base = (unsigned int)__builtin_amdgcn_readfirstlane((int)threadIdx.x) & ~63u;
        if (wave_base < max(nq, n_hq4)) {
            // a wide tile whose rows share one window: one vertical item per lane, weights wave-uniform (scalar loads);
            // lanes past the work load clamped addresses and write nothing
            const int u0 = (int)up_div(U.V, y0) - U.V.off;
            const f4 hq_v = hq_src[min(threadIdx.x, n_hq4 - 1u)];
            f4 s0[T];
            up_vpass_load<T>(src4, sp4, sw, sh, cq0 + (int)threadIdx.x, u0, s0);
            request();
            float w[RU][T];
#pragma unroll
            for (int r = 0; r < RU; ++r) {
                const unsigned int cls = up_class(U.V, y0 + r);
#pragma unroll
                for (int j = 0; j < T; ++j) w[r][j] = vc[cls * T + j];
            }
            up_vpass_mask<T>(sw, sh, cq0 + (int)threadIdx.x, u0, s0);
            f4 acc[RU];
#pragma unroll
            for (int r = 0; r < RU; ++r) {
                acc[r] = f4{ 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
                for (int j = 0; j < T; ++j) acc[r] += s0[j] * w[r][j];
            }
            if (threadIdx.x < n_hq4) reinterpret_cast<f4 *>(hq)[threadIdx.x] = hq_v;
            if (threadIdx.x < nq) {
#pragma unroll
                for (int r = 0; r < RU; ++r) *reinterpret_cast<f4 *>(tmp + r * ncp + 4u * threadIdx.x) = acc[r];
            }
        } else {
            request();
        }
    } else {
        if (threadIdx.x < n_hq4) reinterpret_cast<f4 *>(hq)[threadIdx.x] = hq_src[threadIdx.x];
        request();
        const unsigned int chunk = U.chunk;
        const unsigned int items = nq * ((th + chunk - 1u) / chunk);
        for (unsigned int it = threadIdx.x; it < items; it += 256u) {
            const unsigned int k = it / nq, q = it - k * nq;
            const unsigned int ty0 = k * chunk, n = min(chunk, th - ty0);
            const int u0 = (int)up_div(U.V, y0 + ty0) - U.V.off, sq = cq0 + (int)q;
            f4 s[T];
            up_vpass_load<T>(src4, sp4, sw, sh, sq, u0, s);
            up_vpass_mask<T>(sw, sh, sq, u0, s);
            for (unsigned int r = 0; r < n; ++r) {
                const unsigned int cls = up_class(U.V, y0 + ty0 + r);
                f4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
                for (int j = 0; j < T; ++j) acc += s[j] * vc[cls * T + j];
                *reinterpret_cast<f4 *>(tmp + (ty0 + r) * ncp + 4u * q) = acc;
            }
        }
    }
    __syncthreads();
    if (!active) return;

    // ---- horizontal pass + chain ----
    const unsigned int m = up_div(U.H, ox);
    f4 wq[T];
    {
        const unsigned int qx = ox >> 2, nqx = dw >> 2;
        unsigned int qc = half ? 0u : qx - m * r4;  // qx % r4
        if (qx < U.H.qb_lo) qc = r4 + qx;
        else if (qx >= nqx - U.H.qb_hi) qc = r4 + U.H.qb_lo + (qx - (nqx - U.H.qb_hi));
        const f4 *q4 = reinterpret_cast<const f4 *>(hq) + qc * T;
#pragma unroll
        for (int j = 0; j < T; ++j) wq[j] = q4[j];
    }
    const float *win = tmp + ((int)m - U.H.off - 4 * cq0);  // the thread's window in an intermediate row
#pragma unroll
    for (int u = 0; u < RU; ++u) {
        const unsigned int ty = min(rg + u * row_groups, th - 1u);
        const float *row = win + ty * ncp;
        f4 t = { 0.0f, 0.0f, 0.0f, 0.0f };
        if constexpr (HALF) {
            float v[T + 1];
#pragma unroll
            for (int j = 0; j <= T; ++j) v[j] = row[j];
#pragma unroll
            for (int j = 0; j < T; ++j) t += wq[j] * f4{ v[j], v[j], v[j + 1], v[j + 1] };
        } else {
            float v[T];
#pragma unroll
            for (int j = 0; j < T; ++j) v[j] = row[j];
#pragma unroll
            for (int j = 0; j < T; ++j) t += wq[j] * v[j];
        }
        in[K - 1][u] = up_clamp01(t);
    }
    f4 acc[RU];
    prog(in, acc);
    f4 *outp = reinterpret_cast<f4 *>(P.out[b]) + ox / 4u;
    const unsigned int opitch = P.out_pitch[b];
#pragma unroll
    for (int u = 0; u < RU; ++u) {
        const unsigned int ty = rg + u * row_groups;
        if (ty < th) {
            if (NT & 0x100u) __builtin_nontemporal_store(acc[u], &outp[(size_t)(y0 + ty) * opitch]);
            else outp[(size_t)(y0 + ty) * opitch] = acc[u];
        }
    }
}
