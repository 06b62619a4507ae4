// The pack pass: an f32 plane into its lossless packed copy of one tier, verified as it is written (chain_pack.h).
#include <hip/hip_runtime.h>

#include "kc_internal.hpp"

namespace kc {

#include "chain_pack.h"

// One float4 per thread.  What was encoded is decoded again with the function the chain kernels use and compared with the
// original bit for bit; any difference raises *flag (every thread that raises it stores the same 1).
template <int TIER>
__global__ __launch_bounds__(256) void pack_plane_kernel(const float *__restrict__ src, void *__restrict__ dst, uint64_t quads, uint32_t *flag)
{
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= quads) return;
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    const pack_f4 x = reinterpret_cast<const pack_f4 *>(src)[q];
    pack_f4 back;
    if (TIER == KC_PACK_FIX24) {
        const pack_u3 v = pack_encode_fix24(x);
        *reinterpret_cast<pack_u3a *>(static_cast<char *>(dst) + q * 12u) = v;
        back = pack_decode_fix24(v);
    } else {
        const unsigned int v = pack_encode_u8(x);
        static_cast<unsigned int *>(dst)[q] = v;
        back = pack_decode_u8(v);
    }
    const u4 a = __builtin_bit_cast(u4, x), b = __builtin_bit_cast(u4, back);
    if (a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w) *flag = 1u;
}

hipError_t launch_pack_plane(uint32_t tier, const float *src, void *dst, uint64_t quads, uint32_t *flag, hipStream_t s)
{
    if (quads == 0 || quads > 0x7fffffffull * 256u || (tier != (uint32_t)KC_PACK_FIX24 && tier != (uint32_t)KC_PACK_U8)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((quads + 255u) / 256u));
    if (tier == (uint32_t)KC_PACK_FIX24)
        hipLaunchKernelGGL(pack_plane_kernel<KC_PACK_FIX24>, grid, dim3(256), 0, s, src, dst, quads, flag);
    else
        hipLaunchKernelGGL(pack_plane_kernel<KC_PACK_U8>, grid, dim3(256), 0, s, src, dst, quads, flag);
    return hipGetLastError();
}

}  // namespace kc
