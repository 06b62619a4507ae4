// BC6H, unsigned (KC_BC6H = DXGI_FORMAT_BC6H_UF16; bc.cpp, bc_decode.cpp): the HDR block format, by the integer rules of
// include/kanter_core_amd.h (tests/bc6h_ref.py is the same rules in numpy).  A plane value is quantised to the bit pattern of a
// half float, h(v) = f16_rne(min(max(v, 0), 65504)), an integer in 0..31743; everything after that is integer arithmetic on
// the pattern, so the blocks, the decoded planes and the error record are exact.  The streams are built from bc_blocks.h's steps,
// as bc7.hip's and bc_decode.hip's: one thread per 4x4 block, a grid-stride loop over the blocks in row order, a 16-byte load per
// plane, row and lane through its loaders, one 16-byte store (decode: its plane-row store), nontemporal instantiations, and
// the wave-uniform edge-block test.  A thread holds its texels as rg = R | G << 16 and bl = B: 15-bit values, so a packed 16-bit
// subtract cannot borrow across the lanes and a difference fits a signed 16-bit lane.
//   bc6h_encode_kernel   mode 11 only (one subset, two 10-bit endpoints per channel, sixteen palette entries)
//   bc6h_decode_kernel   the four single-subset modes 11-14; the two-subset modes 1-10 give (0, 0, 0) and are counted
//   bc6h_compare_kernel  the squared differences of the half bit patterns, decoded against h(source)
// The counts and sums leave each workgroup as one record of KC_BC_REC_WORDS u64 words (bc_blocks.h's bc_fold_record), and
// bc_decode.hip's bc_combine_kernel folds the records (launch_bc_combine).
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // grid_cap, ld_policy / st_policy
#include "bc_blocks.h"  // the packed types and lanes, the block walk, the row loaders, the plane-row store, the record fold and BC6H's rules

static __device__ __forceinline__ uint32_t bc6h_w4(uint32_t i) { return (64u * i + 7u) / 15u; }  // 0, 4, 9, 13, ..., 60, 64

// E(q) = fin(unq_10(q)): what a 10-bit endpoint decodes to at weight 0: 0, 46, 77, ..., 31 q + 15, ..., 31697, 31743
// (as arithmetic on the two comparisons: a chain of selects on q becomes a switch, and the switch divergent branches)
static __device__ __forceinline__ uint32_t bc6h_e10(uint32_t q) { return 31u * q + 15u + 15u * (uint32_t)(q == 1023u) - 15u * (uint32_t)(q == 0u); }
// unq_10(q) = 0, 64 q + 32, 0xFFFF likewise
static __device__ __forceinline__ uint32_t bc6h_unq10(uint32_t q) { return 64u * q + 32u + 31u * (uint32_t)(q == 1023u) - 32u * (uint32_t)(q == 0u); }

// The smallest q minimising |E(q) - e|, e in 0..31743: e div 31 is right except next to the two irregular ends of E and on
// some ties, always within one step, so its neighbours are tried in ascending order and a later one must be strictly closer.
static __device__ __forceinline__ uint32_t bc6h_q10(uint32_t e)
{
    const uint32_t qc = e / 31u;  // <= 1023
    const uint32_t qa = qc > 0u ? qc - 1u : 0u, qb = qc < 1023u ? qc + 1u : 1023u;
    auto dist = [e](uint32_t q) {
        const uint32_t v = bc6h_e10(q);
        return v > e ? v - e : e - v;
    };
    const uint32_t da = dist(qa), dc = dist(qc), db = dist(qb);
    const uint32_t q = dc < da ? qc : qa;
    return db < min(da, dc) ? qb : q;
}

// One block in mode 11.  The axis is BC7's: per channel lo and hi, the reference channel k the first of the largest range,
// and the sign of s_c = sum_t a_t (2 p_t,c - lo_c - hi_c), a_t = 2 p_t,k - lo_k - hi_k, picks which corner of the box endpoint
// 0 takes.  A term reaches 2^30 and the sum 2^34: the three sums are 64-bit.
static __device__ __forceinline__ bc_u4 encode_bc6h(const uint32_t (&rg)[16], const uint32_t (&bl)[16])
{
    uint32_t lrg = rg[0], hrg = lrg, lb = bl[0], hb = lb;
#pragma unroll
    for (int t = 1; t < 16; ++t) {
        lrg = pk_min(lrg, rg[t]);
        hrg = pk_max(hrg, rg[t]);
        lb = min(lb, bl[t]);
        hb = max(hb, bl[t]);
    }
    const uint32_t lo[3] = { lrg & 0xffffu, lrg >> 16, lb }, hi[3] = { hrg & 0xffffu, hrg >> 16, hb };
    const uint32_t dr = hi[0] - lo[0], dg = hi[1] - lo[1], dbl = hi[2] - lo[2];
    const bool kr = dr >= dg && dr >= dbl, kg = !kr && dg >= dbl;  // k = R, G, else B: the first channel of the largest range
    const int32_t sr = (int32_t)(lo[0] + hi[0]), sg = (int32_t)(lo[1] + hi[1]), sb = (int32_t)(lo[2] + hi[2]);
    const int32_t sgb = kg ? sg : sb, sk = kr ? sr : sgb;
    const uint32_t ksh = kg ? 16u : 0u;
    long long cr = 0, cg = 0, cb = 0;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int32_t pr = (int32_t)(rg[t] & 0xffffu), pg = (int32_t)(rg[t] >> 16), pb = (int32_t)bl[t];
        const int32_t a = 2 * (int32_t)__builtin_amdgcn_ubfe((kr || kg) ? rg[t] : bl[t], ksh, 16u) - sk;  // -31743..31743
        cr += (long long)a * (2 * pr - sr);
        cg += (long long)a * (2 * pg - sg);
        cb += (long long)a * (2 * pb - sb);
    }
    const bool neg[3] = { cr < 0, cg < 0, cb < 0 };
    uint32_t q0[3], q1[3], u0[3], u1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        q0[c] = bc6h_q10(neg[c] ? hi[c] : lo[c]);
        q1[c] = bc6h_q10(neg[c] ? lo[c] : hi[c]);
        u0[c] = bc6h_unq10(q0[c]);
        u1[c] = bc6h_unq10(q1[c]);
    }
    // The exhaustive search.  A squared distance is below 3 * 31743^2 < 2^32: it does not share a word with the index, as
    // BC7's key does, so the distance and the index are kept apart and a later entry must be strictly closer (the lowest
    // index on a tie).  R and G: one packed subtract and one dot product, 2 * 31743^2 < 2^31; B: a 24-bit multiply-add on top,
    // whose 32-bit sum is taken as unsigned.
    uint32_t best[16], bi[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) best[t] = 0xffffffffu, bi[t] = 0u;
#pragma unroll 1  // rolled: an entry lives only for its sixteen texels
    for (uint32_t i = 0; i < 16u; ++i) {
        const uint32_t w = bc6h_w4(i);
        const uint32_t prg = bc6h_entry(u0[0], u1[0], w) | bc6h_entry(u0[1], u1[1], w) << 16;
        const int32_t pb = (int32_t)bc6h_entry(u0[2], u1[2], w);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const uint32_t d = pk_sub(rg[t], prg);
            const int32_t e = (int32_t)bl[t] - pb;
            const uint32_t s = (uint32_t)dot2(d, d, 0) + (uint32_t)__mul24(e, e);
            const bool closer = s < best[t];
            best[t] = closer ? s : best[t];
            bi[t] = closer ? i : bi[t];
        }
    }
    uint32_t ilo = 0u, ihi = 0u;  // texel t's index at bits 4t..4t+3
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        if (t < 8) ilo |= bi[t] << (4 * t);
        else ihi |= bi[t] << (4 * t - 32);
    }
    if (ilo & 8u) {  // the anchor: texel 0's index keeps its top bit clear
        ilo = ~ilo;
        ihi = ~ihi;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t x = q0[c];
            q0[c] = q1[c];
            q1[c] = x;
        }
    }
    const uint64_t idx = (uint64_t)ilo | (uint64_t)ihi << 32;
    const uint64_t stream = (idx & 7u) | (idx >> 4) << 3;  // texel 0 in 3 bits, then 4 bits each: 63 bits
    const uint64_t lo64 = 3u | (uint64_t)q0[0] << 5 | (uint64_t)q0[1] << 15 | (uint64_t)q0[2] << 25 | (uint64_t)q1[0] << 35 |
                          (uint64_t)q1[1] << 45 | (uint64_t)q1[2] << 55;  // B1's top bit falls off: it opens the high word
    const uint64_t hi64 = (uint64_t)(q1[2] >> 9) | stream << 1;
    return bc_u4{ (uint32_t)lo64, (uint32_t)(lo64 >> 32), (uint32_t)hi64, (uint32_t)(hi64 >> 32) };
}

template <bool NT>  // NT: the planes are read once and do not fit the Infinity Cache (cache_policy_mask)
__global__ __launch_bounds__(256) void bc6h_encode_kernel(Operand r, Operand g, Operand b, int gray, const BcBlockArgs a)
{
    constexpr uint32_t CH = 0x7u;  // R, G, B
    const Operand op[4] = { r, g, b, Operand{ nullptr, 0, 1.0f } };
    const BcWalk k = bc_walk(a.w, a.h, a.bx, a.by);
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < k.total; idx += gridDim.x * 256u) {
        uint32_t i, j;
        const bool wave_edge = bc_block_of(k, idx, i, j);
        uint32_t rg[16], bl[16];
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            bc_f4 v[4];
            bc_load_row<CH, NT>(op, gray, a, i, j, y, wave_edge, v);
            bc6h_quantise_row(v, gray, y, rg, bl);
        }
        if (wave_edge) bc_clamp_columns(a, i, rg, bl);
        *reinterpret_cast<bc_u4 *>(a.dst + (size_t)j * a.row_pitch + (size_t)i * 16) = encode_bc6h(rg, bl);
    }
}

// ---------------------------------------------------------------- decode
// One block into half bit patterns.  The mode field: bit 1 clear, a 2-bit field, modes 1 and 2; otherwise 5 bits, of which
// 3, 7, 11 and 15 are the single-subset modes 11-14 (m = field >> 2), 19, 23, 27 and 31 are reserved and the rest are modes
// 3-10.  Mode 11 stores both endpoints in 10 bits; modes 12-14 store endpoint 0 in n = 11, 12, 16 bits -- its low ten in the
// first group of a channel, the others at the top of the second group in reverse order -- and endpoint 1 as a signed delta of
// 9, 8, 4 bits at the bottom of the second group, added modulo 2^n.  Returns whether the block is of a two-subset mode, which
// is not decoded; such a block and a reserved one keep the endpoints 0 and every texel interpolates to 0.
static __device__ __forceinline__ bool decode_bc6h(const uint32_t (&b)[4], uint32_t (&rg)[16], uint32_t (&bl)[16])
{
    const uint32_t f = b[0] & 31u;
    const bool single = (f & 3u) == 3u && f < 16u;
    const uint32_t m = (f >> 2) & 3u;
    const uint32_t n = m == 3u ? 16u : 10u + m;
    const uint32_t db = m == 3u ? 4u : 10u - m;  // the delta's bits (mode 11: the whole group is endpoint 1)
    uint32_t u0[3], u1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t low = bc_bits(b, 5 + 10 * c, 10), grp = bc_bits(b, 35 + 10 * c, 10);
        const uint32_t rev = __brev(grp) >> 22;  // bit j = the group's bit 9 - j = endpoint 0's bit 10 + j
        const uint32_t e0 = low | (rev & ((1u << (n - 10u)) - 1u)) << 10;
        const int32_t delta = (int32_t)(grp << (32u - db)) >> (32u - db);
        const uint32_t e1 = m == 0u ? grp : (e0 + (uint32_t)delta) & ((1u << n) - 1u);
        u0[c] = single ? bc6h_unq(e0, n) : 0u;
        u1[c] = single ? bc6h_unq(e1, n) : 0u;
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const uint32_t w = bc6h_w4(t == 0 ? bc_bits(b, 65, 3) : bc_bits(b, 68 + 4 * (t - 1), 4));
        rg[t] = bc6h_entry(u0[0], u1[0], w) | bc6h_entry(u0[1], u1[1], w) << 16;
        bl[t] = bc6h_entry(u0[2], u1[2], w);
    }
    return (f & 3u) != 3u;
}

template <bool NT>
static __device__ __forceinline__ bool bc6h_decode_block(const char *p, uint32_t (&rg)[16], uint32_t (&bl)[16])
{
    const bc_u4 v = ld_policy<NT>(reinterpret_cast<const bc_u4 *>(p));
    const uint32_t b[4] = { v.x, v.y, v.z, v.w };
    return decode_bc6h(b, rg, bl);
}

// Writes dst[0..2] = R, G, B.  COUNT: the workgroup's undecoded blocks go to a.partials[blockIdx.x]
template <bool NT, bool COUNT>
__global__ __launch_bounds__(256) void bc6h_decode_kernel(const BcDecodeArgs a)
{
    [[maybe_unused]] __shared__ unsigned long long red[4][1];  // per wave
    const BcWalk k = bc_walk(a.w, a.h, a.bx, a.by);
    unsigned long long undecoded[1] = { 0ull };
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < k.total; idx += gridDim.x * 256u) {
        uint32_t i, j;
        const bool wave_edge = bc_block_of(k, idx, i, j);
        uint32_t rg[16], bl[16];
        const bool skipped = bc6h_decode_block<NT>(a.src + (size_t)j * a.row_pitch + (size_t)i * 16, rg, bl);
        if constexpr (COUNT) undecoded[0] += skipped ? 1u : 0u;
        bc_store_planes<3, NT>(a, i, j, wave_edge, [&](int c, int t) { return half_value(c == 0 ? rg[t] & 0xffffu : c == 1 ? rg[t] >> 16 : bl[t]); });
    }
    if constexpr (COUNT) bc_fold_record<1, 0x1u>(undecoded, red, a.partials + blockIdx.x);
}

// ---------------------------------------------------------------- the error of an encoding
// Record of a workgroup, bc_decode.hip's layout: [0..2] the squared error of R, G, B over the half bit patterns, [4..6] the
// largest absolute difference, [8] undecoded blocks; the other words are 0.
template <bool NT>
__global__ __launch_bounds__(256) void bc6h_compare_kernel(Operand r, Operand g, Operand b, int gray, const BcBlockArgs a,
                                                           unsigned long long *partials)
{
    __shared__ unsigned long long red[4][KC_BC_REC_WORDS];  // per wave
    constexpr uint32_t CH = 0x7u;
    const Operand op[4] = { r, g, b, Operand{ nullptr, 0, 1.0f } };
    const BcWalk k = bc_walk(a.w, a.h, a.bx, a.by);
    unsigned long long sse[3] = { 0ull, 0ull, 0ull };
    uint32_t mx[3] = { 0u, 0u, 0u }, undecoded = 0u;
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < k.total; idx += gridDim.x * 256u) {
        uint32_t i, j;
        const bool wave_edge = bc_block_of(k, idx, i, j);
        uint32_t rg[16], bl[16];
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            bc_f4 v[4];
            bc_load_row<CH, NT>(op, gray, a, i, j, y, wave_edge, v);  // rows past the height repeat the last one: in bounds
            bc6h_quantise_row(v, gray, y, rg, bl);
        }
        uint32_t drg[16], dbl[16];
        undecoded += bc6h_decode_block<NT>(a.dst + (size_t)j * a.row_pitch + (size_t)i * 16, drg, dbl) ? 1u : 0u;
        const uint32_t cols = wave_edge ? min(a.w - 4u * i, 4u) : 4u, rows = wave_edge ? min(a.h - 4u * j, 4u) : 4u;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const bool in = !wave_edge || ((uint32_t)(t & 3) < cols && (uint32_t)(t >> 2) < rows);  // replicated edge texels do not count
            const uint32_t src[3] = { rg[t] & 0xffffu, rg[t] >> 16, bl[t] }, dec[3] = { drg[t] & 0xffffu, drg[t] >> 16, dbl[t] };
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t d = in ? (src[c] > dec[c] ? src[c] - dec[c] : dec[c] - src[c]) : 0u;  // <= 31743: d * d fits 32 bits
                sse[c] += d * d;  // sixteen of them do not: the sum is 64-bit
                mx[c] = max(mx[c], d);
            }
        }
    }
    unsigned long long val[KC_BC_REC_WORDS];
#pragma unroll
    for (uint32_t w = 0; w < KC_BC_REC_WORDS; ++w) val[w] = 0ull;
#pragma unroll
    for (int c = 0; c < 3; ++c) val[c] = sse[c], val[4 + c] = mx[c];
    val[8] = undecoded;
    bc_fold_record<KC_BC_REC_WORDS, 0x177u>(val, red, partials + (size_t)blockIdx.x * KC_BC_REC_WORDS);  // words 0-2, 4-6 and 8
}

// ---------------------------------------------------------------- launchers
hipError_t launch_bc6h_encode(const Operand op[4], int gray, char *dst, uint64_t row_pitch, uint32_t w, uint32_t h, uint32_t nt_mask,
                              hipStream_t s)
{
    const BcBlockArgs a = bc_block_args(dst, row_pitch, w, h);
    const uint64_t total = (uint64_t)a.bx * a.by;
    if (total == 0) return hipSuccess;
    const uint32_t blocks = bc_grid(total, 1u << 30);
    if ((nt_mask & 0xffu) != 0) bc6h_encode_kernel<true><<<dim3(blocks), 256, 0, s>>>(op[0], op[1], op[2], gray, a);
    else bc6h_encode_kernel<false><<<dim3(blocks), 256, 0, s>>>(op[0], op[1], op[2], gray, a);
    return hipGetLastError();
}

hipError_t launch_bc6h_decode(const BcDecodeArgs &a, bool count, uint32_t nt_mask, uint32_t groups, hipStream_t s)
{
    if (groups == 0 || a.bx == 0 || a.by == 0) return hipErrorInvalidValue;
    if (count && (!a.partials || !a.result)) return hipErrorInvalidValue;
    const bool nt = (nt_mask & 0x100u) != 0;  // the planes written are the launch's stream
    if (count) {
        if (nt) bc6h_decode_kernel<true, true><<<dim3(groups), 256, 0, s>>>(a);
        else bc6h_decode_kernel<false, true><<<dim3(groups), 256, 0, s>>>(a);
    } else {
        if (nt) bc6h_decode_kernel<true, false><<<dim3(groups), 256, 0, s>>>(a);
        else bc6h_decode_kernel<false, false><<<dim3(groups), 256, 0, s>>>(a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !count) return e;
    return launch_bc_combine(a.partials, groups, 1u, 0u, a.result, s);
}

hipError_t launch_bc6h_compare(const Operand op[4], int gray, const char *blocks, uint64_t row_pitch, uint32_t w, uint32_t h, uint32_t nt_mask,
                               uint32_t groups, unsigned long long *partials, unsigned long long *result, hipStream_t s)
{
    const BcBlockArgs a = bc_block_args(const_cast<char *>(blocks), row_pitch, w, h);  // read only here
    if (groups == 0 || a.bx == 0 || a.by == 0 || !partials || !result) return hipErrorInvalidValue;
    if ((nt_mask & 0xffu) != 0) bc6h_compare_kernel<true><<<dim3(groups), 256, 0, s>>>(op[0], op[1], op[2], gray, a, partials);
    else bc6h_compare_kernel<false><<<dim3(groups), 256, 0, s>>>(op[0], op[1], op[2], gray, a, partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_bc_combine(partials, groups, KC_BC_REC_WORDS, 0xf0u, result, s);
}

}  // namespace kc
