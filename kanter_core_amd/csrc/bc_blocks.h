// What the block encoder kernels share -- bc.hip (BC1, BC3, BC4, BC5) and bc7.hip: the packed types, the row loaders, the
// quantiser, the column clamp and the kernels' arguments.  A thread holds its block's texels as packed 16-bit lanes,
// rb = R | B << 16 and ga = G | A << 16.
// Included inside namespace kc after streaming.h; every definition is static, each unit keeps its own copy.
#pragma once

typedef float bc_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t bc_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t bc_u2 __attribute__((ext_vector_type(2)));
typedef int16_t bc_s2 __attribute__((ext_vector_type(2)));
typedef uint16_t bc_h2 __attribute__((ext_vector_type(2)));

static __device__ __forceinline__ bc_s2 as_s2(uint32_t x) { return __builtin_bit_cast(bc_s2, x); }
static __device__ __forceinline__ bc_h2 as_h2(uint32_t x) { return __builtin_bit_cast(bc_h2, x); }

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

struct BcBlockArgs {
    char *dst;
    uint64_t row_pitch;  // bytes between block rows
    uint32_t w, h, bx, by;
};

// Row y of a block's texels, raw: a 16-byte load per channel the format reads (CH: bit c = channel c; Gray: the plane once, for
// R; a constant: none)
template <uint32_t CH, bool NT>
static __device__ __forceinline__ void bc_load_row(const Operand (&op)[4], int gray, const BcBlockArgs &a, uint32_t i, uint32_t j, int y,
                                                   bool wave_edge, bc_f4 (&v)[4])
{
    uint32_t row = 4 * j + y;
    if (wave_edge) row = min(row, a.h - 1);  // bottom edge blocks repeat the last row
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
