// BC7 (kc_image_to_bc with KC_BC7, bc.cpp): the image as kc_image_to_u8 writes it -> 16-byte BC7 blocks of the single-subset
// modes 6 and 5, by the integer rules of include/kanter_core_amd.h (tests/bc7_ref.py is the same rules in numpy).  The stream is
// bc_encode_kernel's (bc.hip), built from the same steps of bc_blocks.h: one thread per 4x4 block, a 16-byte load per
// plane, row and lane, texels kept as rb = R | B << 16 and ga = G | A << 16, one 16-byte store.  Both modes are evaluated in the
// thread, on the packed lanes: a packed 16-bit subtract and a 16-bit dot product give the squared distance of two channels at
// once, and the palette entries are made in the outer loop of the exhaustive search, never held.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // grid_cap, ld_policy, quant_u8 / quant_u8_srgb
#include "bc_blocks.h"  // BcBlockArgs, the grid, the block walk, the row loaders and the quantiser: shared by the block-compression units

// interp of both 16-bit lanes: ((64 - w) e0 + w e1 + 32) >> 6; a lane's sum stays below 2^14, so nothing crosses into the other
static __device__ __forceinline__ uint32_t pk_interp(uint32_t e0, uint32_t e1, uint32_t w)
{
    return (((64u - w) * e0 + w * e1 + 0x00200020u) >> 6) & 0x03ff03ffu;
}

// Bit c set where s_c < 0, s_c = sum_t a_t (2 p_t,c - lo_c - hi_c) with a_t = 2 p_t,k - lo_k - hi_k (channels R, G, B, A = lanes
// rb.lo, ga.lo, rb.hi, ga.hi; lo + hi in the same lanes): s_c = 2 sum a p_c - (lo_c + hi_c) sum a, as in BC1.
static __device__ __forceinline__ uint32_t bc7_signs(const uint32_t (&rb)[16], const uint32_t (&ga)[16], uint32_t k, uint32_t srb, uint32_t sga)
{
    const uint32_t ksh = (k & 2u) ? 16u : 0u;
    const int32_t sk = (int32_t)__builtin_amdgcn_ubfe((k & 1u) ? sga : srb, ksh, 16u);
    int32_t sa = 0, sr = 0, sg = 0, sb = 0, sl = 0;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int32_t a = 2 * (int32_t)__builtin_amdgcn_ubfe((k & 1u) ? ga[t] : rb[t], ksh, 16u) - sk;  // -510..510
        sa += a;
        const uint32_t alo = (uint32_t)a & 0xffffu, ahi = (uint32_t)a << 16;
        sr = dot2(rb[t], alo, sr);
        sb = dot2(rb[t], ahi, sb);
        sg = dot2(ga[t], alo, sg);
        sl = dot2(ga[t], ahi, sl);
    }
    const uint32_t nr = 2 * sr - (int32_t)(srb & 0xffffu) * sa < 0, ng = 2 * sg - (int32_t)(sga & 0xffffu) * sa < 0;
    const uint32_t nb = 2 * sb - (int32_t)(srb >> 16) * sa < 0, nl = 2 * sl - (int32_t)(sga >> 16) * sa < 0;
    return nr | ng << 1 | nb << 2 | nl << 3;
}

// Both lanes: hi where the channel's bit of `neg` is set, else lo (bit `c0` the low lane's channel, bit `c1` the high lane's)
static __device__ __forceinline__ uint32_t bc7_pick(uint32_t lo, uint32_t hi, uint32_t neg, uint32_t c0, uint32_t c1)
{
    const uint32_t m = ((neg >> c0) & 1u ? 0xffffu : 0u) | ((neg >> c1) & 1u ? 0xffff0000u : 0u);
    return (hi & m) | (lo & ~m);
}

// Mode 6's endpoint quantiser on the four packed channels e = (erb, ega): with the p-bit 0 a channel decodes to e when e is
// even and one off when it is odd (255 -> 254 by the clamp), with the p-bit 1 the other way round, so the costs are the counts
// of odd and of even channels and the p-bit is 1 iff three or four channels are odd (strictly lower cost).  q is the 7-bit
// field, v = 2 q + p what it decodes to.
static __device__ __forceinline__ void bc7_quant6(uint32_t erb, uint32_t ega, uint32_t &qrb, uint32_t &qga, uint32_t &pb, uint32_t &vrb,
                                                  uint32_t &vga)
{
    const uint32_t odd = __builtin_popcount(erb & 0x00010001u) + __builtin_popcount(ega & 0x00010001u);
    pb = odd >= 3u ? 1u : 0u;
    const uint32_t up = pb ? 0u : 0x00010001u;
    qrb = pk_min(((erb + up) >> 1) & 0x00ff00ffu, 0x007f007fu);
    qga = pk_min(((ega + up) >> 1) & 0x00ff00ffu, 0x007f007fu);
    vrb = 2u * qrb + (pb ? 0x00010001u : 0u);
    vga = 2u * qga + (pb ? 0x00010001u : 0u);
}

static __device__ __forceinline__ uint32_t bc7_quant5(uint32_t e) { return (127u * e + 127u) / 255u; }

// -2 q of both lanes of a palette entry q (lanes <= 255)
static __device__ __forceinline__ uint32_t pk_minus_twice(uint32_t q) { return pk_sub(0u, q << 1); }

// One block.  lo / hi: the packed channel minima and maxima.  The searches do not form |p - q|^2 but e = |q|^2 - 2 p.q, which
// is the squared distance less |p|^2: the same for every palette entry q of a texel, so the arg-min and its ties are the
// contract's, and summed over the texels the same for both modes (mode 5's colour and alpha parts together are all four
// channels), so err5 < err6 is the comparison of the sums of e.  |q|^2 is made once per entry and a texel costs two dot
// products.  Each search keeps per texel the signed key (e << bits) + index, so that the minimum over the palette is the smallest
// distance and, among equal ones, the lowest index; |e| < 2^18.
static __device__ __forceinline__ bc_u4 encode_bc7(const uint32_t (&rb)[16], const uint32_t (&ga)[16])
{
    uint32_t lrb = rb[0], hrb = lrb, lga = ga[0], hga = lga;
#pragma unroll
    for (int t = 1; t < 16; ++t) {
        lrb = pk_min(lrb, rb[t]);
        hrb = pk_max(hrb, rb[t]);
        lga = pk_min(lga, ga[t]);
        hga = pk_max(hga, ga[t]);
    }
    const uint32_t srb = lrb + hrb, sga = lga + hga;  // lo + hi <= 510 a lane
    const uint32_t drb = hrb - lrb, dga = hga - lga;  // hi >= lo a lane: no borrow
    const uint32_t rr = drb & 0xffffu, rg = dga & 0xffffu, rbl = drb >> 16, ral = dga >> 16;
    const uint32_t k3 = (rr >= rg && rr >= rbl) ? 0u : (rg >= rbl ? 1u : 2u);  // the first channel of the largest range
    const uint32_t r3 = k3 == 0u ? rr : k3 == 1u ? rg : rbl;
    const uint32_t k4 = ral > r3 ? 3u : k3;
    const uint32_t neg4 = bc7_signs(rb, ga, k4, srb, sga);
    // with alpha the widest channel the colour axis of mode 5 has a reference channel of its own
    const uint32_t neg3 = k4 == 3u ? bc7_signs(rb, ga, k3, srb, sga) : neg4;

    // ---- mode 6: RGBA endpoints of 7 bits and a p-bit each, sixteen palette entries
    uint64_t lo6, hi6;
    int32_t err6 = 0;  // less sum |p|^2
    {
        const uint32_t e0rb = bc7_pick(lrb, hrb, neg4, 0u, 2u), e0ga = bc7_pick(lga, hga, neg4, 1u, 3u);
        const uint32_t e1rb = srb - e0rb, e1ga = sga - e0ga;  // the other corner
        uint32_t q0rb, q0ga, p0, v0rb, v0ga, q1rb, q1ga, p1, v1rb, v1ga;
        bc7_quant6(e0rb, e0ga, q0rb, q0ga, p0, v0rb, v0ga);
        bc7_quant6(e1rb, e1ga, q1rb, q1ga, p1, v1rb, v1ga);
        int32_t key[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) key[t] = 0x7fffffff;
#pragma unroll 1  // rolled: the entry's -2 q and |q|^2 live only for its sixteen texels
        for (uint32_t i = 0; i < 16u; ++i) {
            const uint32_t w = (64u * i + 7u) / 15u;  // 0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64
            const uint32_t prb = pk_interp(v0rb, v1rb, w), pga = pk_interp(v0ga, v1ga, w);
            const uint32_t mrb = pk_minus_twice(prb), mga = pk_minus_twice(pga);
            const int32_t qq = dot2(prb, prb, dot2(pga, pga, 0));
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int32_t e = dot2(rb[t], mrb, dot2(ga[t], mga, qq));
                key[t] = min(key[t], (int32_t)(((uint32_t)e << 4) + i));
            }
        }
        uint32_t ilo = 0u, ihi = 0u;  // texel t's index at bits 4t..4t+3
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            err6 += key[t] >> 4;
            if (t < 8) ilo |= ((uint32_t)key[t] & 15u) << (4 * t);
            else ihi |= ((uint32_t)key[t] & 15u) << (4 * t - 32);
        }
        if (ilo & 8u) {  // the anchor: texel 0's index keeps its top bit clear
            ilo = ~ilo;
            ihi = ~ihi;
            uint32_t x;
            x = q0rb, q0rb = q1rb, q1rb = x;
            x = q0ga, q0ga = q1ga, q1ga = x;
            x = p0, p0 = p1, p1 = x;
        }
        const uint64_t idx = (uint64_t)ilo | (uint64_t)ihi << 32;
        const uint64_t stream = (idx & 7u) | (idx >> 4) << 3;  // texel 0 in 3 bits, then 4 bits each: 63 bits
        lo6 = 64u | (uint64_t)(q0rb & 0x7fu) << 7 | (uint64_t)(q1rb & 0x7fu) << 14 | (uint64_t)(q0ga & 0x7fu) << 21 |
              (uint64_t)(q1ga & 0x7fu) << 28 | (uint64_t)(q0rb >> 16) << 35 | (uint64_t)(q1rb >> 16) << 42 | (uint64_t)(q0ga >> 16) << 49 |
              (uint64_t)(q1ga >> 16) << 56 | (uint64_t)p0 << 63;
        hi6 = (uint64_t)p1 | stream << 1;
    }

    // ---- mode 5: RGB endpoints of 7 bits, alpha endpoints of 8, four palette entries each
    uint64_t lo5, hi5;
    int32_t err5 = 0;  // less sum |p|^2
    {
        const uint32_t e0rb = bc7_pick(lrb, hrb, neg3, 0u, 2u), e0g = bc7_pick(lga, hga, neg3, 1u, 1u) & 0xffffu;
        const uint32_t e1rb = srb - e0rb, e1g = (sga & 0xffffu) - e0g;
        uint32_t q0[3] = { bc7_quant5(e0rb & 0xffffu), bc7_quant5(e0g), bc7_quant5(e0rb >> 16) };
        uint32_t q1[3] = { bc7_quant5(e1rb & 0xffffu), bc7_quant5(e1g), bc7_quant5(e1rb >> 16) };
        uint32_t a0 = lga >> 16, a1 = hga >> 16;
        auto dec = [](uint32_t q) { return (q << 1) | (q >> 6); };
        const uint32_t v0rb = dec(q0[0]) | dec(q0[2]) << 16, v1rb = dec(q1[0]) | dec(q1[2]) << 16;
        const uint32_t v0ga = dec(q0[1]) | a0 << 16, v1ga = dec(q1[1]) | a1 << 16;
        int32_t kc[16], ka[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) kc[t] = ka[t] = 0x7fffffff;
#pragma unroll 1
        for (uint32_t i = 0; i < 4u; ++i) {
            const uint32_t w = (64u * i + 1u) / 3u;  // 0, 21, 43, 64
            const uint32_t prb = pk_interp(v0rb, v1rb, w), pga = pk_interp(v0ga, v1ga, w);
            const uint32_t pg = pga & 0xffffu, pa = pga & 0xffff0000u;  // the colour's lane and the alpha's
            const uint32_t mrb = pk_minus_twice(prb), mg = pk_minus_twice(pg), ma = pk_minus_twice(pa);
            const int32_t qc = dot2(prb, prb, dot2(pg, pg, 0)), qa = dot2(pa, pa, 0);
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int32_t ec = dot2(rb[t], mrb, dot2(ga[t], mg, qc));
                const int32_t ea = dot2(ga[t], ma, qa);
                kc[t] = min(kc[t], (int32_t)(((uint32_t)ec << 2) + i));
                ka[t] = min(ka[t], (int32_t)(((uint32_t)ea << 2) + i));
            }
        }
        uint32_t ic = 0u, ia = 0u;  // texel t's index at bits 2t, 2t+1
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            err5 += (kc[t] >> 2) + (ka[t] >> 2);
            ic |= ((uint32_t)kc[t] & 3u) << (2 * t);
            ia |= ((uint32_t)ka[t] & 3u) << (2 * t);
        }
        if (ic & 2u) {  // the two index sets are anchored independently
            ic = ~ic;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t x = q0[c];
                q0[c] = q1[c];
                q1[c] = x;
            }
        }
        if (ia & 2u) {
            ia = ~ia;
            const uint32_t x = a0;
            a0 = a1;
            a1 = x;
        }
        const uint64_t sc = (ic & 1u) | (ic >> 2) << 1, sa = (ia & 1u) | (ia >> 2) << 1;  // texel 0 in 1 bit, then 2 bits each: 31 bits
        lo5 = 32u | (uint64_t)q0[0] << 8 | (uint64_t)q1[0] << 15 | (uint64_t)q0[1] << 22 | (uint64_t)q1[1] << 29 | (uint64_t)q0[2] << 36 |
              (uint64_t)q1[2] << 43 | (uint64_t)a0 << 50 | (uint64_t)a1 << 58;  // a1's top two bits fall off: they open hi5
        hi5 = (uint64_t)(a1 >> 6) | sc << 2 | sa << 33;
    }
    const bool m5 = err5 < err6;
    const uint64_t lo = m5 ? lo5 : lo6, hi = m5 ? hi5 : hi6;
    return bc_u4{ (uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32) };
}

template <bool SRGB, bool NT>  // NT: the planes are read once and do not fit the Infinity Cache (cache_policy_mask)
__global__ __launch_bounds__(256) void bc7_encode_kernel(Operand r, Operand g, Operand b, Operand al, int gray, const BcBlockArgs a)
{
    __shared__ uint32_t srgb_t[SRGB ? 257 : 1];
    constexpr uint32_t CH = 0xfu;  // all four channels
    const Operand op[4] = { r, g, b, al };
    const BcWalk k = bc_walk(a.w, a.h, a.bx, a.by);
    uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if constexpr (SRGB) {
        // The first block's first row of loads goes out BEFORE the threshold table is staged (a global read and a barrier that
        // every thread of the workgroup takes, in range or not), as in to_u8_kernel: the table arrives while they are in flight.
        const bool in_range = idx < k.total;
        uint32_t i, j;
        const bool we = bc_block_of(k, idx, i, j);
        bc_f4 v[4];
        if (in_range) bc_load_row<CH, NT>(op, gray, a, i, j, 0, we, v);
        bc_stage_srgb(srgb_t);
        if (!in_range) return;
        uint32_t rb[16], ga[16];
        bc_quantise_row<CH, SRGB>(v, gray, 0, srgb_t, rb, ga);
#pragma unroll
        for (int y = 1; y < 4; ++y) {
            bc_load_row<CH, NT>(op, gray, a, i, j, y, we, v);
            bc_quantise_row<CH, SRGB>(v, gray, y, srgb_t, rb, ga);
        }
        if (we) bc_clamp_columns(a, i, rb, ga);
        *reinterpret_cast<bc_u4 *>(a.dst + (size_t)j * a.row_pitch + (size_t)i * 16) = encode_bc7(rb, ga);
        idx += gridDim.x * 256u;
    }
    for (; idx < k.total; idx += gridDim.x * 256u) {
        uint32_t i, j;
        const bool we = bc_block_of(k, idx, i, j);
        uint32_t rb[16], ga[16];
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            bc_f4 v[4];
            bc_load_row<CH, NT>(op, gray, a, i, j, y, we, v);
            bc_quantise_row<CH, SRGB>(v, gray, y, srgb_t, rb, ga);
        }
        if (we) bc_clamp_columns(a, i, rb, ga);
        *reinterpret_cast<bc_u4 *>(a.dst + (size_t)j * a.row_pitch + (size_t)i * 16) = encode_bc7(rb, ga);
    }
}

hipError_t launch_bc7_encode(int srgb, const Operand op[4], int gray, char *dst, uint64_t row_pitch, uint32_t w, uint32_t h, uint32_t nt_mask,
                             hipStream_t s)
{
    const BcBlockArgs a = bc_block_args(dst, row_pitch, w, h);
    const uint64_t total = (uint64_t)a.bx * a.by;
    if (total == 0) return hipSuccess;
    const uint32_t blocks = bc_grid(total, 1u << 30);
    const bool nt = (nt_mask & 0xffu) != 0;
#define KC_BC7(SR, NTL) bc7_encode_kernel<SR, NTL><<<dim3(blocks), 256, 0, s>>>(op[0], op[1], op[2], op[3], gray, a)
    if (srgb) {
        if (nt) KC_BC7(true, true);
        else KC_BC7(true, false);
    } else {
        if (nt) KC_BC7(false, true);
        else KC_BC7(false, false);
    }
#undef KC_BC7
    return hipGetLastError();
}

}  // namespace kc
