// Device-memory images (kc_image_from_device / kc_image_to_device, devimage.cpp): caller memory in one of five element types
// and two layouts <-> the library's f32 planes.  HBM-bound streaming kernels in the form of to_u8_kernel / from_u8_kernel: a
// grid-stride loop over pixel quads (four neighbouring pixels of one row per thread), 16-byte plane accesses (the library's
// planes are 256-byte pitched), and on the caller's side the widest access the quad's byte count, the pointer and the
// pitches allow (host-checked, DevImageArgs::vec) -- a scalar path per element otherwise and for a row's last, partial quad.
// The channel count is a run-time argument: one switch per launch picks the loop compiled for it.
#include "kc_internal.hpp"

namespace kc {

#include "streaming.h"  // grid_cap, ld_policy / st_policy, quant_u8 / quant_u8_srgb: shared with u8.hip

typedef float dv_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t dv_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t dv_u2 __attribute__((ext_vector_type(2)));

static constexpr int dt_bytes(int dt) { return dt == KC_DTYPE_U8 ? 1 : dt == KC_DTYPE_F32 ? 4 : 2; }
// HWC: the widest unit (16, 8 or 4 bytes) that divides the B bytes of a quad of C-channel pixels (B = 4 C E is a multiple of 4)
static constexpr int hwc_unit(int bytes) { return bytes % 16 == 0 ? 16 : bytes % 8 == 0 ? 8 : 4; }

// ---- element <-> f32 ----
template <int DT>
static __device__ __forceinline__ float decode(uint32_t bits)
{
    if constexpr (DT == KC_DTYPE_U8) return (float)bits / 255.0f;  // from_u8_kernel's IEEE division
    else if constexpr (DT == KC_DTYPE_U16) return (float)bits / 65535.0f;
    else if constexpr (DT == KC_DTYPE_F16) {
        // exact widening; infinities and NaNs by their bits (the payload kept, as a bit-level conversion does)
        if ((bits & 0x7c00u) == 0x7c00u) return __uint_as_float(((bits & 0x8000u) << 16) | 0x7f800000u | ((bits & 0x3ffu) << 13));
        return (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
    } else if constexpr (DT == KC_DTYPE_BF16) return __uint_as_float(bits << 16);
    else return __uint_as_float(bits);  // F32: the bits as they are
}

// U16: the reference's to_u8 rule at 16 bits, ((v.clamp(0,1) * 65535.).min(65535.)) truncated, NaN -> 65535
static __device__ __forceinline__ uint32_t quant_u16(float v)
{
    float x = v;
    if (x < 0.0f) x = 0.0f;
    if (x > 1.0f) x = 1.0f;  // NaN falls through both
    x = x * 65535.0f;
    if (!(x <= 65535.0f)) x = 65535.0f;
    return (uint32_t)x;
}

template <int DT, bool SRGB>
static __device__ __forceinline__ uint32_t encode(float v, int c, const uint32_t *srgb_tab)
{
    if constexpr (DT == KC_DTYPE_U8) return (SRGB && c < 3) ? quant_u8_srgb(v, srgb_tab) : quant_u8(v);  // alpha stays linear
    else if constexpr (DT == KC_DTYPE_U16) return quant_u16(v);
    else if constexpr (DT == KC_DTYPE_F16) return __builtin_bit_cast(uint16_t, (_Float16)v);  // round to nearest even
    else if constexpr (DT == KC_DTYPE_BF16) return __builtin_bit_cast(uint16_t, (__bf16)v);   // round to nearest even
    else return __float_as_uint(v);
}

// element k of a quad held as 32-bit words
template <int E>
static __device__ __forceinline__ uint32_t word_get(const uint32_t *wd, int k)
{
    if constexpr (E == 1) return (wd[k >> 2] >> (8 * (k & 3))) & 0xffu;
    else if constexpr (E == 2) return (wd[k >> 1] >> (16 * (k & 1))) & 0xffffu;
    else return wd[k];
}
template <int E>
static __device__ __forceinline__ void word_put(uint32_t *wd, int k, uint32_t v)
{
    if constexpr (E == 1) wd[k >> 2] |= v << (8 * (k & 3));
    else if constexpr (E == 2) wd[k >> 1] |= v << (16 * (k & 1));
    else wd[k] = v;
}

// NB bytes (a multiple of UNIT) at p, UNIT-aligned, as 32-bit words
template <int NB, int UNIT, bool NT>
static __device__ __forceinline__ void load_words(const char *p, uint32_t *wd)
{
#pragma unroll
    for (int i = 0; i < NB / UNIT; ++i) {
        if constexpr (UNIT == 16) {
            const dv_u4 v = ld_policy<NT>(reinterpret_cast<const dv_u4 *>(p) + i);
            wd[4 * i] = v.x, wd[4 * i + 1] = v.y, wd[4 * i + 2] = v.z, wd[4 * i + 3] = v.w;
        } else if constexpr (UNIT == 8) {
            const dv_u2 v = ld_policy<NT>(reinterpret_cast<const dv_u2 *>(p) + i);
            wd[2 * i] = v.x, wd[2 * i + 1] = v.y;
        } else {
            wd[i] = ld_policy<NT>(reinterpret_cast<const uint32_t *>(p) + i);
        }
    }
}
template <int NB, int UNIT, bool NT>
static __device__ __forceinline__ void store_words(char *p, const uint32_t *wd)
{
#pragma unroll
    for (int i = 0; i < NB / UNIT; ++i) {
        if constexpr (UNIT == 16) st_policy<NT>(reinterpret_cast<dv_u4 *>(p) + i, dv_u4{ wd[4 * i], wd[4 * i + 1], wd[4 * i + 2], wd[4 * i + 3] });
        else if constexpr (UNIT == 8) st_policy<NT>(reinterpret_cast<dv_u2 *>(p) + i, dv_u2{ wd[2 * i], wd[2 * i + 1] });
        else st_policy<NT>(reinterpret_cast<uint32_t *>(p) + i, wd[i]);
    }
}

template <int E>
static __device__ __forceinline__ uint32_t load_elem(const char *p)
{
    if constexpr (E == 1) return *reinterpret_cast<const uint8_t *>(p);
    else if constexpr (E == 2) return *reinterpret_cast<const uint16_t *>(p);
    else return *reinterpret_cast<const uint32_t *>(p);
}
template <int E>
static __device__ __forceinline__ void store_elem(char *p, uint32_t v)
{
    if constexpr (E == 1) *reinterpret_cast<uint8_t *>(p) = (uint8_t)v;
    else if constexpr (E == 2) *reinterpret_cast<uint16_t *>(p) = (uint16_t)v;
    else *reinterpret_cast<uint32_t *>(p) = v;
}

// ---- import: caller memory -> C planes ----
template <int DT, int LAYOUT, int C, bool NT>  // NT: the planes written do not fit the Infinity Cache (cache_policy_mask)
static __device__ __forceinline__ void import_quads(const DevImageArgs &a, float *const *planes, uint32_t ppitch)
{
    constexpr int E = dt_bytes(DT);
    const uint32_t row_units = (a.w + 3) / 4;
    const uint32_t total = row_units * a.h;
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        const uint32_t y = idx / row_units;
        const uint32_t q = idx - y * row_units;
        const char *row = a.ptr + (size_t)y * a.row_pitch;
        const bool full = a.vec && 4 * q + 3 < a.w;
        float v[C][4];
        if constexpr (LAYOUT == KC_LAYOUT_INTERLEAVED) {
            constexpr int B = 4 * C * E;
            if (full) {
                uint32_t wd[B / 4];
                load_words<B, hwc_unit(B), false>(row + (size_t)q * B, wd);
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int c = 0; c < C; ++c) v[c][p] = decode<DT>(word_get<E>(wd, p * C + c));
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const uint32_t x = 4 * q + p;
#pragma unroll
                    for (int c = 0; c < C; ++c) v[c][p] = x < a.w ? decode<DT>(load_elem<E>(row + ((size_t)x * C + c) * E)) : 0.0f;
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const char *src = row + (size_t)c * a.channel_pitch + (size_t)q * 4 * E;
                if (full) {
                    uint32_t wd[E];
                    load_words<4 * E, 4 * E, false>(src, wd);
#pragma unroll
                    for (int p = 0; p < 4; ++p) v[c][p] = decode<DT>(word_get<E>(wd, p));
                } else {
#pragma unroll
                    for (int p = 0; p < 4; ++p) v[c][p] = 4 * q + p < a.w ? decode<DT>(load_elem<E>(src + p * E)) : 0.0f;
                }
            }
        }
        // the planes' pitch covers whole quads: the last quad of a row is stored whole (its columns past the width are padding)
#pragma unroll
        for (int c = 0; c < C; ++c)
            st_policy<NT>(reinterpret_cast<dv_f4 *>(planes[c] + (size_t)y * ppitch + 4 * q), dv_f4{ v[c][0], v[c][1], v[c][2], v[c][3] });
    }
}

template <int DT, int LAYOUT, bool NT>
__global__ __launch_bounds__(256) void image_import_kernel(const DevImageArgs a, float *p0, float *p1, float *p2, float *p3, uint32_t ppitch)
{
    float *const planes[4] = { p0, p1, p2, p3 };
    switch (a.channels) {
    case 1: import_quads<DT, LAYOUT, 1, NT>(a, planes, ppitch); break;
    case 2: import_quads<DT, LAYOUT, 2, NT>(a, planes, ppitch); break;
    case 3: import_quads<DT, LAYOUT, 3, NT>(a, planes, ppitch); break;
    default: import_quads<DT, LAYOUT, 4, NT>(a, planes, ppitch); break;
    }
}

// ---- export: operands (planes or constants) -> caller memory ----
template <bool NT>
static __device__ __forceinline__ dv_f4 load_operand(const Operand &o, uint32_t row, uint32_t q)
{
    if (o.ptr == nullptr) return dv_f4{ o.c, o.c, o.c, o.c };  // a constant plane: no memory read
    return ld_policy<NT>(reinterpret_cast<const dv_f4 *>(o.ptr + (size_t)row * o.pitch + 4 * q));
}

template <int DT, int LAYOUT, int C, bool SRGB, bool NT>  // NT: the planes are read once and do not fit the Infinity Cache
static __device__ __forceinline__ void export_quads(const Operand (&op)[4], int gray, const DevImageArgs &a, const uint32_t *srgb_tab)
{
    constexpr int E = dt_bytes(DT);
    const uint32_t row_units = (a.w + 3) / 4;
    const uint32_t total = row_units * a.h;
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        const uint32_t y = idx / row_units;
        const uint32_t q = idx - y * row_units;
        dv_f4 v[C];
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = (gray && c > 0 && c < 3) ? v[0] : load_operand<NT>(op[c], y, q);  // Gray: (v, v, v, A)
        char *row = const_cast<char *>(a.ptr) + (size_t)y * a.row_pitch;
        const bool full = a.vec && 4 * q + 3 < a.w;
        if constexpr (LAYOUT == KC_LAYOUT_INTERLEAVED) {
            constexpr int B = 4 * C * E;
            uint32_t wd[B / 4];
#pragma unroll
            for (int i = 0; i < B / 4; ++i) wd[i] = 0u;
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int c = 0; c < C; ++c) word_put<E>(wd, p * C + c, encode<DT, SRGB>(v[c][p], c, srgb_tab));
            if (full) {
                store_words<B, hwc_unit(B), false>(row + (size_t)q * B, wd);
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    if (4 * q + p < a.w)
#pragma unroll
                        for (int c = 0; c < C; ++c) store_elem<E>(row + ((size_t)(4 * q + p) * C + c) * E, word_get<E>(wd, p * C + c));
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                char *dst = row + (size_t)c * a.channel_pitch + (size_t)q * 4 * E;
                uint32_t wd[E];
#pragma unroll
                for (int i = 0; i < E; ++i) wd[i] = 0u;
#pragma unroll
                for (int p = 0; p < 4; ++p) word_put<E>(wd, p, encode<DT, SRGB>(v[c][p], c, srgb_tab));
                if (full) {
                    store_words<4 * E, 4 * E, false>(dst, wd);
                } else {
#pragma unroll
                    for (int p = 0; p < 4; ++p)
                        if (4 * q + p < a.w) store_elem<E>(dst + p * E, word_get<E>(wd, p));
                }
            }
        }
    }
}

template <int DT, int LAYOUT, bool SRGB, bool NT>
__global__ __launch_bounds__(256) void image_export_kernel(Operand r, Operand g, Operand b, Operand al, int gray, const DevImageArgs a)
{
    __shared__ uint32_t srgb_t[SRGB ? 257 : 1];
    if constexpr (SRGB) {
        srgb_t[threadIdx.x] = kSrgbThresholdBits[threadIdx.x];  // 256 threads
        if (threadIdx.x == 0) srgb_t[256] = 0xffffffffu;         // sentinel: nothing is >= it
        __syncthreads();
    }
    const Operand op[4] = { r, g, b, al };
    switch (a.channels) {
    case 1: export_quads<DT, LAYOUT, 1, SRGB, NT>(op, gray, a, srgb_t); break;
    case 2: export_quads<DT, LAYOUT, 2, SRGB, NT>(op, gray, a, srgb_t); break;
    case 3: export_quads<DT, LAYOUT, 3, SRGB, NT>(op, gray, a, srgb_t); break;
    default: export_quads<DT, LAYOUT, 4, SRGB, NT>(op, gray, a, srgb_t); break;
    }
}

static uint64_t devimage_blocks(const DevImageArgs &a)
{
    const uint64_t total = (uint64_t)((a.w + 3) / 4) * a.h;
    uint64_t blocks = (total + 255) / 256;
    if (blocks > grid_cap(1u << 30)) blocks = grid_cap(1u << 30);
    return blocks;
}

hipError_t launch_image_import(int dtype, const DevImageArgs &a, float *const planes[4], uint32_t ppitch, uint32_t nt_mask, hipStream_t s,
                               bool *launched_nt)
{
    const uint64_t blocks = devimage_blocks(a);
    if (blocks == 0) return hipSuccess;
    const bool nt = (nt_mask & 0x100u) != 0;
    const bool hwc = a.layout == KC_LAYOUT_INTERLEAVED;
#define KC_IMPORT(DT, L, NT) image_import_kernel<DT, L, NT><<<dim3((unsigned)blocks), 256, 0, s>>>(a, planes[0], planes[1], planes[2], planes[3], ppitch)
#define KC_IMPORT_L(DT)                                                                    \
    do {                                                                                   \
        if (hwc && nt) KC_IMPORT(DT, KC_LAYOUT_INTERLEAVED, true);                         \
        else if (hwc) KC_IMPORT(DT, KC_LAYOUT_INTERLEAVED, false);                         \
        else if (nt) KC_IMPORT(DT, KC_LAYOUT_PLANAR, true);                                \
        else KC_IMPORT(DT, KC_LAYOUT_PLANAR, false);                                       \
    } while (0)
    switch (dtype) {
    case KC_DTYPE_U8: KC_IMPORT_L(KC_DTYPE_U8); break;
    case KC_DTYPE_U16: KC_IMPORT_L(KC_DTYPE_U16); break;
    case KC_DTYPE_F16: KC_IMPORT_L(KC_DTYPE_F16); break;
    case KC_DTYPE_BF16: KC_IMPORT_L(KC_DTYPE_BF16); break;
    case KC_DTYPE_F32: KC_IMPORT_L(KC_DTYPE_F32); break;
    default: return hipErrorInvalidValue;
    }
#undef KC_IMPORT_L
#undef KC_IMPORT
    if (launched_nt) *launched_nt = nt;
    return hipGetLastError();
}

hipError_t launch_image_export(int dtype, int srgb, const Operand op[4], int gray, const DevImageArgs &a, uint32_t nt_mask, hipStream_t s,
                               bool *launched_nt)
{
    const uint64_t blocks = devimage_blocks(a);
    if (blocks == 0) return hipSuccess;
    const bool nt = (nt_mask & 0xffu) != 0;
    const bool hwc = a.layout == KC_LAYOUT_INTERLEAVED;
    if (srgb && dtype != KC_DTYPE_U8) return hipErrorInvalidValue;
#define KC_EXPORT(DT, L, SR, NT) image_export_kernel<DT, L, SR, NT><<<dim3((unsigned)blocks), 256, 0, s>>>(op[0], op[1], op[2], op[3], gray, a)
#define KC_EXPORT_L(DT, SR)                                                                    \
    do {                                                                                       \
        if (hwc && nt) KC_EXPORT(DT, KC_LAYOUT_INTERLEAVED, SR, true);                         \
        else if (hwc) KC_EXPORT(DT, KC_LAYOUT_INTERLEAVED, SR, false);                         \
        else if (nt) KC_EXPORT(DT, KC_LAYOUT_PLANAR, SR, true);                                \
        else KC_EXPORT(DT, KC_LAYOUT_PLANAR, SR, false);                                       \
    } while (0)
    switch (dtype) {
    case KC_DTYPE_U8:
        if (srgb) KC_EXPORT_L(KC_DTYPE_U8, true);
        else KC_EXPORT_L(KC_DTYPE_U8, false);
        break;
    case KC_DTYPE_U16: KC_EXPORT_L(KC_DTYPE_U16, false); break;
    case KC_DTYPE_F16: KC_EXPORT_L(KC_DTYPE_F16, false); break;
    case KC_DTYPE_BF16: KC_EXPORT_L(KC_DTYPE_BF16, false); break;
    case KC_DTYPE_F32: KC_EXPORT_L(KC_DTYPE_F32, false); break;
    default: return hipErrorInvalidValue;
    }
#undef KC_EXPORT_L
#undef KC_EXPORT
    if (launched_nt) *launched_nt = nt;
    return hipGetLastError();
}

}  // namespace kc
