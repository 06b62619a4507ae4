// What the block-compression units share -- bc.hip (BC1, BC3, BC4, BC5), bc7.hip, bc6h.hip, bc_decode.hip and bc_modes.hip: the packed types,
// the kernels' arguments and grid, the walk over the blocks with its edge rule, the row loaders, the 8-bit quantiser, the column
// clamp, the staging of the sRGB table, the decoders' plane-row store, the fold of a workgroup's counts and sums into one
// record, and BC6H's quantiser and endpoint rules.  The encoder and comparison kernels write their grid-stride loops out over these steps: the loop as one shared
// function compiled the sRGB forms to slower code (see DESIGN, "Where the family's code lies").  A thread holds its block's texels as packed 16-bit
// lanes, rb = R | B << 16 and ga = G | A << 16 (BC6H: rg = R | G << 16 and bl = B, in the same two arrays).
// Included inside namespace kc after streaming.h; every definition is static, each unit keeps its own copy.
#pragma once

typedef float bc_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t bc_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t bc_u2 __attribute__((ext_vector_type(2)));
typedef int16_t bc_s2 __attribute__((ext_vector_type(2)));
typedef uint16_t bc_h2 __attribute__((ext_vector_type(2)));

static __device__ __forceinline__ bc_s2 as_s2(uint32_t x) { return __builtin_bit_cast(bc_s2, x); }
static __device__ __forceinline__ bc_h2 as_h2(uint32_t x) { return __builtin_bit_cast(bc_h2, x); }

// Both 16-bit lanes of a word at once: difference, unsigned minimum and maximum, and the signed dot product a.b + c
static __device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, as_s2(a) - as_s2(b)); }
static __device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(as_h2(a), as_h2(b)));
}
static __device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(as_h2(a), as_h2(b)));
}
static __device__ __forceinline__ int32_t dot2(uint32_t a, uint32_t b, int32_t c) { return __builtin_amdgcn_sdot2(as_s2(a), as_s2(b), c, false); }

// n bits of the 128-bit block from bit `at`, LSB first; `at` and n are constants after unrolling
static __device__ __forceinline__ uint32_t bc_bits(const uint32_t (&b)[4], int at, int n)
{
    const int w = at >> 5, s = at & 31;
    uint32_t v = b[w] >> s;
    if (s + n > 32) v |= b[w + 1] << (32 - s);
    return v & ((1u << n) - 1u);
}

// ---------------------------------------------------------------- arguments and grid (host)
struct BcBlockArgs {
    char *dst;           // the blocks: written by the encoders, read by the comparisons
    uint64_t row_pitch;  // bytes between block rows
    uint32_t w, h, bx, by;
};

static inline BcBlockArgs bc_block_args(char *blocks, uint64_t row_pitch, uint32_t w, uint32_t h)
{
    BcBlockArgs a;
    a.dst = blocks;
    a.row_pitch = row_pitch;
    a.w = w;
    a.h = h;
    a.bx = (w + 3) / 4;
    a.by = (h + 3) / 4;
    return a;
}

// Workgroups of 256 threads for `total` blocks: one block a thread up to `cap` workgroups (the tune_cap option overrides it), the
// grid-stride loop takes the rest; at least one
static inline uint32_t bc_grid(uint64_t total, uint32_t cap)
{
    return (uint32_t)std::max<uint64_t>(std::min<uint64_t>((total + 255) / 256, grid_cap(cap)), 1);
}

// ---------------------------------------------------------------- the walk over the blocks
// Edge blocks: the last block column when the width is not a multiple of 4, the last block row likewise
struct BcWalk {
    uint32_t total, bx, edge_i, edge_j;
};

static __device__ __forceinline__ BcWalk bc_walk(uint32_t w, uint32_t h, uint32_t bx, uint32_t by)
{
    return BcWalk{ bx * by, bx, (w & 3u) ? bx - 1 : 0xffffffffu, (h & 3u) ? by - 1 : 0xffffffffu };
}

// Block n in row order: its column i and row j.  Returns whether the wave holds an edge block (n >= total: no block, as the
// lanes that only accompany their workgroup to a barrier): wave-uniform, so a wave without one skips the clamps and the clipping.
static __device__ __forceinline__ bool bc_block_of(const BcWalk &k, uint32_t n, uint32_t &i, uint32_t &j)
{
    j = n / k.bx;
    i = n - j * k.bx;
    return __any(n < k.total && (i == k.edge_i || j == k.edge_j)) != 0;
}

// ---------------------------------------------------------------- rows of the source image
template <bool NT>
static __device__ __forceinline__ bc_f4 bc_load(const Operand &o, uint32_t row, uint32_t q)
{
    if (o.ptr == nullptr) return bc_f4{ o.c, o.c, o.c, o.c };  // a constant plane: no memory read
    return ld_policy<NT>(reinterpret_cast<const bc_f4 *>(o.ptr + (size_t)row * o.pitch + 4 * q));
}

template <bool SRGB>
static __device__ __forceinline__ uint32_t bc_quant(float v, int c, const uint32_t *srgb_tab)
{
    return (SRGB && c < 3) ? quant_u8_srgb(v, srgb_tab) : quant_u8(v);  // alpha stays linear
}

// Row y of a block's texels, raw: a 16-byte load per channel the format reads (CH: bit c = channel c; Gray: the plane once, for
// R; a constant: none)
template <uint32_t CH, bool NT>
static __device__ __forceinline__ void bc_load_row(const Operand (&op)[4], int gray, const BcBlockArgs &a, uint32_t i, uint32_t j, int y,
                                                   bool wave_edge, bc_f4 (&v)[4])
{
    uint32_t row = 4 * j + y;
    if (wave_edge) row = min(row, a.h - 1);  // bottom edge blocks repeat the last row: in bounds
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (!((CH >> c) & 1u)) continue;
        if (gray && c > 0 && c < 3) continue;
        v[c] = bc_load<NT>(op[c], row, i);
    }
}

// ... quantised to 8 bits and packed as rb = R | B << 16, ga = G | A << 16 (Gray: (v, v, v, A))
template <uint32_t CH, bool SRGB>
static __device__ __forceinline__ void bc_quantise_row(const bc_f4 (&v)[4], int gray, int y, const uint32_t *srgb_tab, uint32_t (&rb)[16],
                                                       uint32_t (&ga)[16])
{
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const uint32_t r = bc_quant<SRGB>(v[0][x], 0, srgb_tab);
        uint32_t g = 0u, b = 0u, al = 0u;
        if constexpr ((CH & 2u) != 0) g = gray ? r : bc_quant<SRGB>(v[1][x], 1, srgb_tab);
        if constexpr ((CH & 4u) != 0) b = gray ? r : bc_quant<SRGB>(v[2][x], 2, srgb_tab);
        if constexpr ((CH & 8u) != 0) al = quant_u8(v[3][x]);
        rb[4 * y + x] = r | (b << 16);
        ga[4 * y + x] = g | (al << 16);
    }
}


// Right edge blocks: the columns past the width repeat the last one
static __device__ __forceinline__ void bc_clamp_columns(const BcBlockArgs &a, uint32_t i, uint32_t (&rb)[16], uint32_t (&ga)[16])
{
    const uint32_t last = min(a.w - 1 - 4 * i, 3u);
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int x = 1; x < 4; ++x)
            if ((uint32_t)x > last) {
                rb[4 * y + x] = rb[4 * y + x - 1];
                ga[4 * y + x] = ga[4 * y + x - 1];
            }
}

// The sRGB threshold table into LDS (257 words), by the workgroup's 256 threads: a global read and a barrier that every thread
// takes
static __device__ __forceinline__ void bc_stage_srgb(uint32_t *srgb_t)
{
    srgb_t[threadIdx.x] = kSrgbThresholdBits[threadIdx.x];
    if (threadIdx.x == 0) srgb_t[256] = 0xffffffffu;  // sentinel: nothing is >= it
    __syncthreads();
}

// ---------------------------------------------------------------- BC1's block, for bc.hip, bc1a.hip and bc_decode.hip
static __device__ __forceinline__ uint32_t pack565(uint32_t r, uint32_t g, uint32_t b)
{
    return ((31u * r + 127u) / 255u) << 11 | ((63u * g + 127u) / 255u) << 5 | ((31u * b + 127u) / 255u);
}

// The endpoints of texels held as rb = R | B << 16 and ga = G | A << 16 (alpha ignored), so that the channel ranges are packed
// 16-bit min / max and the sums over channels 16-bit dot products: the colour box inset by 1/16 of each range, on the diagonal the
// covariance signs against the channel of the largest range choose (s_c = 2 sum a p_c - S_c sum a with a = 2 p_k - S_k,
// S = lo + hi); c0 > c1 unless they are equal.
// PT (KC_BC_PUNCH_THROUGH, bc1a.hip): one masked pass for the block classes a wave holds at once.  Bit t of `opq` = texel t is
// opaque; every min, max and sum runs over the opaque texels (the mask word of a texel is all ones or 0: an OR makes it neutral
// to the minimum, an AND to the maximum and to the sums).  `three`, a lane's own: the three-colour block of 1..15 opaque texels,
// inset by 1/8 and ordered c0 <= c1; otherwise -- all 16 opaque -- the masks are all ones and the result is plain BC1's, bit for
// bit.  A lane without an opaque texel gets endpoints nobody reads.
template <bool PT>
static __device__ __forceinline__ void bc1_endpoints(const uint32_t (&rb)[16], const uint32_t (&ga)[16], uint32_t opq, bool three, uint32_t &c0,
                                                     uint32_t &c1)
{
    bc_h2 lrb, hrb, lga, hga;
    if constexpr (PT) {
        lrb = lga = as_h2(0xffffffffu);
        hrb = hga = as_h2(0u);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const uint32_t m = (uint32_t)__builtin_amdgcn_sbfe((int32_t)opq, (uint32_t)t, 1u);
            lrb = __builtin_elementwise_min(lrb, as_h2(rb[t] | ~m));
            hrb = __builtin_elementwise_max(hrb, as_h2(rb[t] & m));
            lga = __builtin_elementwise_min(lga, as_h2(ga[t] | ~m));
            hga = __builtin_elementwise_max(hga, as_h2(ga[t] & m));
        }
    } else {
        lrb = as_h2(rb[0]), hrb = lrb, lga = as_h2(ga[0]), hga = lga;
#pragma unroll
        for (int t = 1; t < 16; ++t) {
            lrb = __builtin_elementwise_min(lrb, as_h2(rb[t]));
            hrb = __builtin_elementwise_max(hrb, as_h2(rb[t]));
            lga = __builtin_elementwise_min(lga, as_h2(ga[t]));
            hga = __builtin_elementwise_max(hga, as_h2(ga[t]));
        }
    }
    const uint32_t lo[3] = { lrb.x, lga.x, lrb.y }, hi[3] = { hrb.x, hga.x, hrb.y };
    const uint32_t rr = hi[0] - lo[0], rg = hi[1] - lo[1], rb_ = hi[2] - lo[2];
    const uint32_t k = (rr >= rg && rr >= rb_) ? 0u : (rg >= rb_ ? 1u : 2u);
    const int32_t sk = (int32_t)(k == 0u ? lo[0] + hi[0] : k == 1u ? lo[1] + hi[1] : lo[2] + hi[2]);
    const uint32_t ksh = k == 2u ? 16u : 0u;
    int32_t sa = 0, sr = 0, sg = 0, sb = 0;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        int32_t a = 2 * (int32_t)__builtin_amdgcn_ubfe(k == 1u ? ga[t] : rb[t], ksh, 16u) - sk;  // -510..510
        if constexpr (PT) a &= __builtin_amdgcn_sbfe((int32_t)opq, (uint32_t)t, 1u);
        sa += a;
        const uint32_t alo = (uint32_t)a & 0xffffu, ahi = (uint32_t)a << 16;
        sr = __builtin_amdgcn_sdot2(as_s2(rb[t]), as_s2(alo), sr, false);
        sb = __builtin_amdgcn_sdot2(as_s2(rb[t]), as_s2(ahi), sb, false);
        sg = __builtin_amdgcn_sdot2(as_s2(ga[t]), as_s2(alo), sg, false);
    }
    const int32_t s[3] = { 2 * sr - (int32_t)(lo[0] + hi[0]) * sa, 2 * sg - (int32_t)(lo[1] + hi[1]) * sa,
                           2 * sb - (int32_t)(lo[2] + hi[2]) * sa };
    uint32_t ea[3], eb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t m = (hi[c] - lo[c]) >> (PT && three ? 3 : 4);
        const uint32_t a = hi[c] - m, b = lo[c] + m;
        ea[c] = s[c] < 0 ? b : a;  // s_k >= 0: the reference channel keeps its direction
        eb[c] = s[c] < 0 ? a : b;
    }
    c0 = pack565(ea[0], ea[1], ea[2]), c1 = pack565(eb[0], eb[1], eb[2]);
    if ((PT && three) ? c0 > c1 : c0 < c1) {
        const uint32_t tmp = c0;
        c0 = c1;
        c1 = tmp;
    }
}

// The index word of the four-colour block (c0 >= c1).  The palette P_j = 3 E0 + k_j D (D = E1 - E0, k = 0, 3, 1, 2 for
// j = 0..3) lies on one line, so |3p - P_j|^2 = |3p - 3E0|^2 - 6 k v + k^2 L with v = (p - E0).D and L = |D|^2, and the nearest k
// is the number of thresholds 6v > L, 6v > 3L, 6v >= 5L that v passes (the last one >= : the tie of k = 2 and 3 goes to j = 1,
// the lower index) -- the contract's arg-min, without computing the four distances.
static __device__ __forceinline__ uint32_t bc1_indices4(const uint32_t (&rb)[16], const uint32_t (&ga)[16], uint32_t c0, uint32_t c1)
{
    uint32_t word = 0u;
    if (c0 != c1) {
        const int32_t r5 = (int32_t)(c0 >> 11), g6 = (int32_t)((c0 >> 5) & 63u), b5 = (int32_t)(c0 & 31u);
        const int32_t s5 = (int32_t)(c1 >> 11), h6 = (int32_t)((c1 >> 5) & 63u), c5 = (int32_t)(c1 & 31u);
        const int32_t E0[3] = { (r5 << 3) | (r5 >> 2), (g6 << 2) | (g6 >> 4), (b5 << 3) | (b5 >> 2) };
        const int32_t E1[3] = { (s5 << 3) | (s5 >> 2), (h6 << 2) | (h6 >> 4), (c5 << 3) | (c5 >> 2) };
        const int32_t D[3] = { E1[0] - E0[0], E1[1] - E0[1], E1[2] - E0[2] };
        const int32_t L = D[0] * D[0] + D[1] * D[1] + D[2] * D[2];
        const int32_t L3 = 3 * L, L5 = 5 * L;
        const int32_t e0d = -(E0[0] * D[0] + E0[1] * D[1] + E0[2] * D[2]);
        const bc_s2 drb = as_s2(((uint32_t)D[0] & 0xffffu) | ((uint32_t)D[2] << 16)), dg = as_s2((uint32_t)D[1] & 0xffffu);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int32_t v = __builtin_amdgcn_sdot2(as_s2(ga[t]), dg, __builtin_amdgcn_sdot2(as_s2(rb[t]), drb, e0d, false), false);
            const int32_t v6 = 6 * v;
            const uint32_t kk = (uint32_t)(v6 > L) + (uint32_t)(v6 > L3) + (uint32_t)(v6 >= L5);
            word |= __builtin_amdgcn_ubfe(0x78u, 2u * kk, 2u) << (2 * t);  // k = 0, 1, 2, 3 -> j = 0, 2, 3, 1
        }
    }
    return word;
}

// BC1 of the 16 texels, alpha ignored: the bytes c0 and c1, then the index word
static __device__ __forceinline__ bc_u2 encode_bc1(const uint32_t (&rb)[16], const uint32_t (&ga)[16])
{
    uint32_t c0, c1;
    bc1_endpoints<false>(rb, ga, 0xffffu, false, c0, c1);
    return bc_u2{ c0 | (c1 << 16), bc1_indices4(rb, ga, c0, c1) };
}

// BC1 into px (R | G << 8 | B << 16 | A << 24).  `four`: BC3's colour block, always in four-colour mode
static __device__ __forceinline__ void decode_bc1(uint32_t w0, uint32_t idx, bool four, uint32_t (&px)[16])
{
    const uint32_t c0 = w0 & 0xffffu, c1 = w0 >> 16;
    four = four || c0 > c1;
    uint32_t pal[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t sh = c == 0 ? 11u : c == 1 ? 5u : 0u, n = c == 1 ? 6u : 5u;
        const uint32_t q0 = (c0 >> sh) & ((1u << n) - 1u), q1 = (c1 >> sh) & ((1u << n) - 1u);
        const uint32_t e0 = (q0 << (8u - n)) | (q0 >> (2u * n - 8u)), e1 = (q1 << (8u - n)) | (q1 >> (2u * n - 8u));
        const uint32_t p2 = four ? (2u * e0 + e1 + 1u) / 3u : (e0 + e1) >> 1;
        const uint32_t p3 = four ? (e0 + 2u * e1 + 1u) / 3u : 0u;
        pal[0] |= e0 << (8 * c);
        pal[1] |= e1 << (8 * c);
        pal[2] |= p2 << (8 * c);
        pal[3] |= p3 << (8 * c);
    }
    pal[0] |= 0xff000000u;
    pal[1] |= 0xff000000u;
    pal[2] |= 0xff000000u;
    if (four) pal[3] |= 0xff000000u;  // otherwise index 3 is transparent black
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const uint32_t i = idx >> (2 * t);
        const uint32_t lo = (i & 1u) ? pal[1] : pal[0], hi = (i & 1u) ? pal[3] : pal[2];
        px[t] = (i & 2u) ? hi : lo;
    }
}

// ---------------------------------------------------------------- the decoders' store
// The four pixel rows of block (i, j) into the first NP planes of a.dst, texel(c, t) the f32 value of channel c at texel t: a
// float4 per plane row in a wave without an edge block (a wave writes 1 KiB of contiguous bytes per plane row), columns and
// rows clipped to the image otherwise
template <int NP, bool NT, class Texel>
static __device__ __forceinline__ void bc_store_planes(const BcDecodeArgs &a, uint32_t i, uint32_t j, bool wave_edge, Texel texel)
{
    const uint32_t cols = wave_edge ? min(a.w - 4u * i, 4u) : 4u, rows = wave_edge ? min(a.h - 4u * j, 4u) : 4u;
#pragma unroll
    for (int y = 0; y < 4; ++y) {
        if (wave_edge && (uint32_t)y >= rows) break;
#pragma unroll
        for (int c = 0; c < NP; ++c) {
            float *row = a.dst[c] + (size_t)(4u * j + y) * a.dst_pitch + 4u * i;
            bc_f4 v;
#pragma unroll
            for (int x = 0; x < 4; ++x) v[x] = texel(c, 4 * y + x);
            if (!wave_edge || cols == 4u) {
                st_policy<NT>(reinterpret_cast<bc_f4 *>(row), v);
            } else {
#pragma unroll
                for (int x = 0; x < 3; ++x)
                    if ((uint32_t)x < cols) st_policy<NT>(row + x, v[x]);
            }
        }
    }
}

// ---------------------------------------------------------------- counts and sums of a workgroup
// Sum / maximum over the wave's 64 lanes, in every lane
static __device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
        v += (unsigned long long)hi << 32 | lo;
    }
    return v;
}
static __device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off));
    return v;
}

// The threads' val[0..WORDS) to one record of the workgroup at out[0..WORDS): the wave (shuffles), then the workgroup's four
// waves through LDS (red).  Words 4..7 are maxima of 32-bit values, the others sums; USED: bit k clear = word k is 0 in every
// thread and skips the wave's fold.  The error records have KC_BC_REC_WORDS words, a decoder's count one.
template <uint32_t WORDS, uint32_t USED>
static __device__ __forceinline__ void bc_fold_record(unsigned long long (&val)[WORDS], unsigned long long (&red)[4][WORDS],
                                                      unsigned long long *out)
{
#pragma unroll
    for (uint32_t k = 0; k < WORDS; ++k) {
        if (!((USED >> k) & 1u)) continue;
        if (k >= 4 && k < 8) val[k] = wave_max((uint32_t)val[k]);
        else val[k] = wave_sum(val[k]);
    }
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < WORDS; ++k) red[threadIdx.x >> 6][k] = val[k];
    }
    __syncthreads();
    if (threadIdx.x < WORDS) {
        const uint32_t k = threadIdx.x;
        const unsigned long long r0 = red[0][k], r1 = red[1][k], r2 = red[2][k], r3 = red[3][k];
        out[k] = k >= 4 && k < 8 ? max(max(r0, r1), max(r2, r3)) : r0 + r1 + r2 + r3;
    }
}

// ---------------------------------------------------------------- BC6H's rules, for bc6h.hip and bc_modes.hip
// h(v): NaN, the negatives, -0 and -inf fail the comparison and give 0; +inf and everything >= 65504 give 0x7BFF.  The
// conversion rounds to nearest even and keeps denormal halves, as devimage.hip's F16 export does.  The compiler makes one
// median of the two clamps, which may hand -0 through: the callers clear the sign bit, and no other result has it set.
static __device__ __forceinline__ uint32_t quant_half(float v)
{
    float x = v > 0.0f ? v : 0.0f;
    x = x < 65504.0f ? x : 65504.0f;
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)x);
}

// Row y of a block's texels as half bit patterns, rg = R | G << 16 and bl = B (Gray: (v, v, v)); alpha is never read
static __device__ __forceinline__ void bc6h_quantise_row(const bc_f4 (&v)[4], int gray, int y, uint32_t (&rg)[16], uint32_t (&bl)[16])
{
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const uint32_t r = quant_half(v[0][x]);
        const uint32_t g = gray ? r : quant_half(v[1][x]);
        const uint32_t b = gray ? r : quant_half(v[2][x]);
        rg[4 * y + x] = (r | (g << 16)) & 0x7fff7fffu;
        bl[4 * y + x] = b & 0x7fffu;
    }
}

// fin(interp(u0, u1, w)): the half bit pattern of a palette entry from two 16-bit endpoints; 31 * 65535 fits with room
static __device__ __forceinline__ uint32_t bc6h_entry(uint32_t u0, uint32_t u1, uint32_t w)
{
    return (31u * (((64u - w) * u0 + w * u1 + 32u) >> 6)) >> 6;
}

// unq_n(x): an n-bit endpoint as 16 bits
static __device__ __forceinline__ uint32_t bc6h_unq(uint32_t x, uint32_t n)
{
    const uint32_t top = (1u << n) - 1u;
    const uint32_t mid = ((x << 16) + 0x8000u) >> n;  // n <= 12 here: x << 16 stays below 2^28
    return n == 16u ? x : x == 0u ? 0u : x == top ? 0xffffu : mid;
}

// the exact f32 value of a half bit pattern
static __device__ __forceinline__ float half_value(uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits); }
