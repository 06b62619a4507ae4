// The u8 boundary: to_u8_kernel (planes or constants -> interleaved RGBA8, linear or sRGB) and from_u8_kernel (interleaved u8 ->
// planes); the quantisers are streaming.h's.  Device-memory images in other element types and layouts: devimage.hip.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // grid_cap, ld_policy / st_policy, quant_u8 / quant_u8_srgb: shared with devimage.hip, stats.hip and bc.hip
#include "chain_apply.inc"  // splat4, f4

template <bool NT>
static __device__ __forceinline__ float4 load_operand4(const Operand &o, uint32_t row, uint32_t q)
{
    if (o.ptr == nullptr) return splat4(o.c);
    const f4 v = ld_policy<NT>(reinterpret_cast<const f4 *>(o.ptr + (size_t)row * o.pitch + 4 * q));
    return make_float4(v.x, v.y, v.z, v.w);
}

template <bool SRGB, bool NT>  // NT: the planes are read once and do not fit the Infinity Cache (cache_policy_mask)
__global__ __launch_bounds__(256) void to_u8_kernel(Operand r, Operand g, Operand b, Operand a, int gray, uint32_t w,
                                                    uint32_t h, uint8_t *__restrict__ dst)
{
    __shared__ uint32_t srgb_t[SRGB ? 257 : 1];
    const uint32_t *pow_tab = srgb_t;
    const uint32_t row_units = (w + 3) / 4;
    const uint32_t total = row_units * h;
    auto load4 = [&](uint32_t y, uint32_t q, float4 &vr, float4 &vg, float4 &vb, float4 &va) {
        vr = load_operand4<NT>(r, y, q);
        if (!gray) {
            vg = load_operand4<NT>(g, y, q);
            vb = load_operand4<NT>(b, y, q);
            va = load_operand4<NT>(a, y, q);
        }
    };
    auto quantise_store = [&](uint32_t y, uint32_t q, const float4 &vr, const float4 &vg, const float4 &vb, const float4 &va) {
        float rr[4] = { vr.x, vr.y, vr.z, vr.w };
        uint32_t px[4];
        if (gray) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t v = SRGB ? quant_u8_srgb(rr[e], pow_tab) : quant_u8(rr[e]);
                px[e] = v | (v << 8) | (v << 16) | (255u << 24);
            }
        } else {
            float gg[4] = { vg.x, vg.y, vg.z, vg.w };
            float bb[4] = { vb.x, vb.y, vb.z, vb.w };
            float aa[4] = { va.x, va.y, va.z, va.w };
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t qr = SRGB ? quant_u8_srgb(rr[e], pow_tab) : quant_u8(rr[e]);
                const uint32_t qg = SRGB ? quant_u8_srgb(gg[e], pow_tab) : quant_u8(gg[e]);
                const uint32_t qb = SRGB ? quant_u8_srgb(bb[e], pow_tab) : quant_u8(bb[e]);
                const uint32_t qa = quant_u8(aa[e]);
                px[e] = qr | (qg << 8) | (qb << 16) | (qa << 24);
            }
        }
        uint32_t *o = reinterpret_cast<uint32_t *>(dst) + (size_t)y * w + 4 * q;
        if (4 * q + 3 < w && (w & 3u) == 0) {
            *reinterpret_cast<uint4 *>(o) = make_uint4(px[0], px[1], px[2], px[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * q + e < w) o[e] = px[e];
        }
    };
    uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if constexpr (SRGB) {
        // The first quad's plane loads go out BEFORE the threshold table is staged (a global read and a barrier that every
        // thread of the workgroup takes, in range or not): the table arrives while they are in flight (60.1 -> 57.2 us).
        const bool in_range = idx < total;
        const uint32_t y = in_range ? idx / row_units : 0u, q = in_range ? idx - y * row_units : 0u;
        float4 vr = make_float4(0, 0, 0, 0), vg = vr, vb = vr, va = vr;
        if (in_range) load4(y, q, vr, vg, vb, va);
        srgb_t[threadIdx.x] = kSrgbThresholdBits[threadIdx.x];  // 256 threads
        if (threadIdx.x == 0) srgb_t[256] = 0xffffffffu;         // sentinel: nothing is >= it
        __syncthreads();
        if (!in_range) return;
        quantise_store(y, q, vr, vg, vb, va);
        idx += gridDim.x * 256u;
    }
    for (; idx < total; idx += gridDim.x * 256u) {
        const uint32_t y = idx / row_units;
        const uint32_t q = idx - y * row_units;
        float4 vr, vg = make_float4(0, 0, 0, 0), vb = vg, va = vg;
        load4(y, q, vr, vg, vb, va);
        quantise_store(y, q, vr, vg, vb, va);
    }
}

hipError_t launch_to_u8(Operand r, Operand g, Operand b, Operand a, int gray, int srgb, uint32_t w, uint32_t h,
                        uint8_t *dst, uint32_t nt_mask, hipStream_t s, bool *launched_nt)
{
    const bool ntl = (nt_mask & 0xffu) != 0;
    const uint64_t total = (uint64_t)((w + 3) / 4) * h;
    if (total == 0) return hipSuccess;
    uint64_t blocks = (total + 255) / 256;
    if (blocks > grid_cap(1u << 30)) blocks = grid_cap(1u << 30);
    if (srgb && ntl)
        to_u8_kernel<true, true><<<dim3((unsigned)blocks), 256, 0, s>>>(r, g, b, a, gray, w, h, dst);
    else if (srgb)
        to_u8_kernel<true, false><<<dim3((unsigned)blocks), 256, 0, s>>>(r, g, b, a, gray, w, h, dst);
    else if (ntl)
        to_u8_kernel<false, true><<<dim3((unsigned)blocks), 256, 0, s>>>(r, g, b, a, gray, w, h, dst);
    else
        to_u8_kernel<false, false><<<dim3((unsigned)blocks), 256, 0, s>>>(r, g, b, a, gray, w, h, dst);
    if (launched_nt) *launched_nt = ntl;
    return hipGetLastError();
}

// deconstruct_image, src/shared.rs:16-56: interleaved u8 (1..4 channels) -> planar f32 / 255.;
// channels the file lacks become constant planes on the host side (R,G,B = 0, A = 1).
template <bool NT>  // NT: the planes written do not fit the Infinity Cache (cache_policy_mask)
__global__ __launch_bounds__(256) void from_u8_kernel(const uint8_t *__restrict__ src, int channels, uint32_t w,
                                                      uint32_t h, float *p0, float *p1, float *p2, float *p3,
                                                      uint32_t pitch)
{
    const uint32_t total = w * h;
    float *planes[4] = { p0, p1, p2, p3 };
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        const uint32_t y = idx / w;
        const uint32_t x = idx - y * w;
        if (channels == 4) {
            const uint32_t v = reinterpret_cast<const uint32_t *>(src)[idx];
            st_policy<NT>(&p0[(size_t)y * pitch + x], (float)(v & 255u) / 255.0f);
            st_policy<NT>(&p1[(size_t)y * pitch + x], (float)((v >> 8) & 255u) / 255.0f);
            st_policy<NT>(&p2[(size_t)y * pitch + x], (float)((v >> 16) & 255u) / 255.0f);
            st_policy<NT>(&p3[(size_t)y * pitch + x], (float)(v >> 24) / 255.0f);
        } else {
            for (int c = 0; c < channels; ++c)
                planes[c][(size_t)y * pitch + x] = (float)src[(size_t)idx * channels + c] / 255.0f;
        }
    }
}

hipError_t launch_from_u8(const uint8_t *src, int channels, uint32_t w, uint32_t h, float *const planes[4],
                          uint32_t pitch, uint32_t nt_mask, hipStream_t s, bool *launched_nt)
{
    const uint64_t total = (uint64_t)w * h;
    if (total == 0) return hipSuccess;
    uint64_t blocks = (total + 255) / 256;
    if (blocks > grid_cap(1u << 30)) blocks = grid_cap(1u << 30);
    const bool nts = (nt_mask & 0x100u) != 0;
    if (nts)
        from_u8_kernel<true><<<dim3((unsigned)blocks), 256, 0, s>>>(src, channels, w, h, planes[0], planes[1], planes[2], planes[3], pitch);
    else
        from_u8_kernel<false><<<dim3((unsigned)blocks), 256, 0, s>>>(src, channels, w, h, planes[0], planes[1], planes[2], planes[3], pitch);
    if (launched_nt) *launched_nt = nts;
    return hipGetLastError();
}

}  // namespace kc
