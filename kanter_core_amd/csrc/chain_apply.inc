// Per-sample operations of a Mix step (src/node/mix.rs:136-192) shared by the step interpreter (chain_interp.inc) and chain1.hip;
// u8.hip and chain.hip's fill_kernel take splat4 from here, and f4.
// Included inside namespace kc (chain1.hip: inside an unnamed namespace as well, pow_positive.inc defines a __constant__ table).
static __device__ __forceinline__ float4 splat4(float v) { return make_float4(v, v, v, v); }

// f32::powf (src/node/mix.rs:189), evaluated in f64 and rounded to f32 once (<= 1 ulp from any libm powf).
// Positive finite base and finite exponent -- every pixel of ordinary image data -- take
// pow_positive() (pow_positive.inc: 2^(b log2 a), ~75 f64 operations; against the f64 pow routine it
// differs for about 1 pair in 10^8, by one ulp: profiles/pow_check.hip).  Everything else (zero,
// negative, infinite or NaN base, infinite or NaN exponent) goes to that routine, whose special-case
// rules are powf's: pow(x, 0) = 1, pow(1, NaN) = 1, negative base with a non-integer exponent = NaN,
// signed zeros and infinities by the exponent's parity ...
#include "pow_positive.inc"

static __device__ __noinline__ float pow_general(float a, float b) { return (float)pow((double)a, (double)b); }

// `tab`: what pow_setup() returned (the LDS copy of kPowTab + coefficients); only the pow codes read it
static __device__ __forceinline__ float kc_powf(float a, float b, const PowCtx *tab)
{
    if (a > 0.0f && a < __builtin_inff() && __builtin_fabsf(b) < __builtin_inff()) return pow_positive(a, b, *tab);
    return pow_general(a, b);
}

template <int CODE>
static __device__ __forceinline__ float apply1(float acc, float x, float c = 0.0f, const PowCtx *tab = nullptr)
{
    if constexpr (CODE == CH_ADD_INV) return c - (acc + x);
    else if constexpr (CODE == CH_SUBL_INV) return c - (acc - x);
    else if constexpr (CODE == CH_SUBR_INV) return c - (x - acc);
    else if constexpr (CODE == CH_MUL_INV) return c - (acc * x);
    else if constexpr (CODE == CH_ADD) return acc + x;
    else if constexpr (CODE == CH_SUB_L) return acc - x;
    else if constexpr (CODE == CH_SUB_R) return x - acc;
    else if constexpr (CODE == CH_MUL) return acc * x;
    else if constexpr (CODE == CH_DIV_L) return acc / x;
    else if constexpr (CODE == CH_DIV_R) return x / acc;
    else if constexpr (CODE == CH_POW_L) return kc_powf(acc, x, tab);
    else if constexpr (CODE == CH_POW_R) return kc_powf(x, acc, tab);
    else if constexpr (CODE == CH_ADD_R) return x + acc;
    else return x * acc;
}

typedef float f4 __attribute__((ext_vector_type(4)));

