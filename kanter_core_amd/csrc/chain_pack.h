// Lossless packed copies of chain inputs ("shadows"): the tiers, as the device sees them.
// Shared, as text, by the pack pass (chain_pack.hip) and by the run-time specialiser, which embeds this file in front of every
// kernel that reads a packed input (csrc/specialize.cpp): builtin types only, no includes, meant to be included inside
// namespace kc after chain_program.h.
//
// A source that stays embedded in a graph is read again by every evaluation, as f32, although its values are quantised: a
// plane of k * 2^-24 (what every uniform-float generator produces) needs 3 bytes per sample, a plane of k / 255.0f (what an
// 8-bit file becomes, u8.hip from_u8_kernel) needs 1.  A tier is { code, bytes per quad, encode, decode }; the pack pass
// decodes what it wrote with the function below and compares bit patterns with the original, so a plane is packed only if
// decode(encode(x)) is x for every sample: whatever encode does with -0.0, NaN, infinities, negatives, 1.0 or off-grid
// values, they end as a mismatch and the plane stays f32.
//
//   tier        code  sample        bytes per quad  layout of a quad
//   FIX24       1     k * 2^-24     12              the four 24-bit k, little endian, one after the other in three dwords
//   U8          2     k / 255.0f    4               the four bytes k in one dword, sample 0 lowest
typedef float pack_f4 __attribute__((ext_vector_type(4)));
typedef unsigned int pack_u3 __attribute__((ext_vector_type(3)));
typedef pack_u3 __attribute__((aligned(4))) pack_u3a;  // as it lies in a shadow: 12 bytes apart, dword aligned

static __device__ __forceinline__ pack_u3 pack_encode_fix24(pack_f4 x)
{
    unsigned int k[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)  // (max first: NaN becomes 0)
        k[i] = (unsigned int)__builtin_fminf(__builtin_fmaxf(x[i] * 16777216.0f, 0.0f), 16777215.0f);
    return pack_u3{ k[0] | k[1] << 24, k[1] >> 8 | k[2] << 16, k[2] >> 16 | k[3] << 8 };
}

// 4 mask / align / shift, 4 conversions, 2 packed multiplies; the multiply by 2^-24 is exact
static __device__ __forceinline__ pack_f4 pack_decode_fix24(pack_u3 v)
{
    const unsigned int k0 = v.x & 0xffffffu, k1 = __builtin_amdgcn_alignbit(v.y, v.x, 24) & 0xffffffu,
                       k2 = __builtin_amdgcn_alignbit(v.z, v.y, 16) & 0xffffffu, k3 = v.z >> 8;
    return pack_f4{ (float)k0, (float)k1, (float)k2, (float)k3 } * 0x1p-24f;
}

static __device__ __forceinline__ unsigned int pack_encode_u8(pack_f4 x)
{
    unsigned int k[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) k[i] = (unsigned int)__builtin_fminf(__builtin_fmaxf(__builtin_rintf(x[i] * 255.0f), 0.0f), 255.0f);
    return k[0] | k[1] << 8 | k[2] << 16 | k[3] << 24;
}

// k / 255.0f without the division: one Newton step on the product with the rounded reciprocal gives the correctly rounded
// quotient for every k in 0..255 (the plain product is wrong for 126 of them).  Explicit fma: the build contracts nothing.
static __device__ __forceinline__ pack_f4 pack_decode_u8(unsigned int v)
{
    const float r = 1.0f / 255.0f;
    const pack_f4 x = pack_f4{ (float)(v & 0xffu), (float)(v >> 8 & 0xffu), (float)(v >> 16 & 0xffu), (float)(v >> 24) };
    const pack_f4 q = x * r;
    pack_f4 e, out;
#pragma unroll
    for (int i = 0; i < 4; ++i) e[i] = __builtin_fmaf(-255.0f, q[i], x[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = __builtin_fmaf(e[i], r, q[i]);
    return out;
}
