// The Mix-chain step interpreter: runs a ChainProgram's step table on the float4 a thread holds.  Used by chain_kernel
// (chain.hip), resize_chain_kernel (resize_tile.hip) and the interpreter-driven up-sampling kernel (upsample.hip).
// Included inside namespace kc, after chain_apply.inc (f4, apply1<CODE>).

// One step on the U float4 a thread owns, written OUT OF PLACE (dst = op(src, x)): the decode
// loop ping-pongs between two register sets, so no switch arm ever has to preserve or merge the
// old accumulator and the step costs exactly one packed VALU instruction per pixel pair.
template <int CODE, int U>
static __device__ __forceinline__ void apply4(f4 (&dst)[U], const f4 (&src)[U], const f4 (&x)[U], float c, const PowCtx *tab)
{
#pragma unroll
    for (int u = 0; u < U; ++u) {
        dst[u].x = apply1<CODE>(src[u].x, x[u].x, c, tab);
        dst[u].y = apply1<CODE>(src[u].y, x[u].y, c, tab);
        dst[u].z = apply1<CODE>(src[u].z, x[u].z, c, tab);
        dst[u].w = apply1<CODE>(src[u].w, x[u].w, c, tab);
    }
}

template <int CODE, int U>
static __device__ __forceinline__ void apply4c(f4 (&dst)[U], const f4 (&src)[U], float c, const PowCtx *tab)
{
#pragma unroll
    for (int u = 0; u < U; ++u) {
        dst[u].x = apply1<CODE>(src[u].x, c, 0.0f, tab);
        dst[u].y = apply1<CODE>(src[u].y, c, 0.0f, tab);
        dst[u].z = apply1<CODE>(src[u].z, c, 0.0f, tab);
        dst[u].w = apply1<CODE>(src[u].w, c, 0.0f, tab);
    }
}

// Decode.  The step record {word, constant} is wave-uniform (kernel argument block, read through
// SMEM one step ahead), so the dispatch is scalar compares and branches and each arm is
// straight-line VALU on the U float4 the thread owns.  PMC shows the kernel is ISSUE-bound for
// long chains (every instruction, scalar or vector, costs the wave ~4 issue cycles), so the
// scalar path is kept short: one 16-byte scalar load per two steps, a 2-level switch (operand
// source, then op), and only the arms the program can contain -- MODE 0 = {+, -, *}, 1 = + divide,
// 2 = + pow (f64 pow call).  x + acc / x * acc are canonicalised to acc + x / acc * x on the host.
#define KC_CODE_SWITCH(APPLY, DST, SRC)                                                   \
    switch (w & 0xffu) {                                                                  \
    case CH_ADD: APPLY(CH_ADD, DST, SRC); break;                                          \
    case CH_SUB_L: APPLY(CH_SUB_L, DST, SRC); break;                                      \
    case CH_SUB_R: APPLY(CH_SUB_R, DST, SRC); break;                                      \
    case CH_MUL: APPLY(CH_MUL, DST, SRC); break;                                          \
    case CH_DIV_L: if constexpr (MODE >= 1) { APPLY(CH_DIV_L, DST, SRC); } else __builtin_unreachable(); break; \
    case CH_DIV_R: if constexpr (MODE >= 1) { APPLY(CH_DIV_R, DST, SRC); } else __builtin_unreachable(); break; \
    case CH_POW_L: if constexpr (MODE >= 2) { APPLY(CH_POW_L, DST, SRC); } else __builtin_unreachable(); break; \
    case CH_POW_R: if constexpr (MODE >= 2) { APPLY(CH_POW_R, DST, SRC); } else __builtin_unreachable(); break; \
    default: __builtin_unreachable();                                                     \
    }

// Plane operands also carry the fused "step, then c - acc" codes.
#define KC_CODE_SWITCH_P(APPLY, DST, SRC)                                                 \
    switch (w & 0xffu) {                                                                  \
    case CH_ADD: APPLY(CH_ADD, DST, SRC); break;                                          \
    case CH_SUB_L: APPLY(CH_SUB_L, DST, SRC); break;                                      \
    case CH_SUB_R: APPLY(CH_SUB_R, DST, SRC); break;                                      \
    case CH_MUL: APPLY(CH_MUL, DST, SRC); break;                                          \
    case CH_ADD_INV: APPLY(CH_ADD_INV, DST, SRC); break;                                  \
    case CH_SUBL_INV: APPLY(CH_SUBL_INV, DST, SRC); break;                                \
    case CH_SUBR_INV: APPLY(CH_SUBR_INV, DST, SRC); break;                                \
    case CH_MUL_INV: APPLY(CH_MUL_INV, DST, SRC); break;                                  \
    case CH_DIV_L: if constexpr (MODE >= 1) { APPLY(CH_DIV_L, DST, SRC); } else __builtin_unreachable(); break; \
    case CH_DIV_R: if constexpr (MODE >= 1) { APPLY(CH_DIV_R, DST, SRC); } else __builtin_unreachable(); break; \
    case CH_POW_L: if constexpr (MODE >= 2) { APPLY(CH_POW_L, DST, SRC); } else __builtin_unreachable(); break; \
    case CH_POW_R: if constexpr (MODE >= 2) { APPLY(CH_POW_R, DST, SRC); } else __builtin_unreachable(); break; \
    default: __builtin_unreachable();                                                     \
    }

// Runs the whole step program on the U float4 a thread holds: acc = start, then every step.
template <int K, int U, int MODE>
static __device__ __forceinline__ void chain_run(const ChainProgram &P, const uint32_t b, const f4 (&in)[K][U], f4 (&acc)[U],
                                                 const PowCtx *tab = nullptr)
{
    if (P.start_src < 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = f4{ P.start_c[b], P.start_c[b], P.start_c[b], P.start_c[b] };
    } else {
        switch (P.start_src) {
        case 0:
#pragma unroll
            for (int u = 0; u < U; ++u) acc[u] = in[0][u];
            break;
        case 1:
            if constexpr (K > 1) {
#pragma unroll
                for (int u = 0; u < U; ++u) acc[u] = in[1][u];
            }
            break;
        case 2:
            if constexpr (K > 2) {
#pragma unroll
                for (int u = 0; u < U; ++u) acc[u] = in[2][u];
            }
            break;
        default:
            if constexpr (K > 3) {
#pragma unroll
                for (int u = 0; u < U; ++u) acc[u] = in[3][u];
            }
            break;
        }
    }

    // Steps alternate acc -> alt -> acc (no arm ever merges register sets); the host validates
    // every record, so unknown words cannot occur.
    const uint32_t n_ops = P.n_ops;
    const ChainStepPair *pp = P.step[b];  // two records per 16-byte scalar load, fetched one pair ahead
    ChainStepPair nxt = pp[0];
    f4 alt[U];
#define KC_APPLY_C(CODE, DST, SRC) apply4c<CODE, U>(DST, SRC, c, tab)
#define KC_APPLY_0(CODE, DST, SRC) apply4<CODE, U>(DST, SRC, in[0], c, tab)
#define KC_APPLY_1(CODE, DST, SRC) apply4<CODE, U>(DST, SRC, in[K > 1 ? 1 : 0], c, tab)
#define KC_APPLY_2(CODE, DST, SRC) apply4<CODE, U>(DST, SRC, in[K > 2 ? 2 : 0], c, tab)
#define KC_APPLY_3(CODE, DST, SRC) apply4<CODE, U>(DST, SRC, in[K > 3 ? 3 : 0], c, tab)
#define KC_STEP(DST, SRC, REC)                                                          \
    {                                                                                   \
        const uint32_t w = (REC).word;                                                  \
        const float c = (REC).c;                                                        \
        switch (w >> 8) {                                                               \
        case 0: KC_CODE_SWITCH(KC_APPLY_C, DST, SRC) break;                             \
        case 1: KC_CODE_SWITCH_P(KC_APPLY_0, DST, SRC) break;                           \
        case 2: if constexpr (K > 1) { KC_CODE_SWITCH_P(KC_APPLY_1, DST, SRC) } else __builtin_unreachable(); break; \
        case 3: if constexpr (K > 2) { KC_CODE_SWITCH_P(KC_APPLY_2, DST, SRC) } else __builtin_unreachable(); break; \
        case 4: if constexpr (K > 3) { KC_CODE_SWITCH_P(KC_APPLY_3, DST, SRC) } else __builtin_unreachable(); break; \
        default: __builtin_unreachable();                                               \
        }                                                                               \
    }
    uint32_t i = 0;
    for (; i + 1 < n_ops; i += 2) {
        const ChainStepPair cur = nxt;
        nxt = pp[i / 2 + 1];
        KC_STEP(alt, acc, cur.a)
        KC_STEP(acc, alt, cur.b)
    }
    if (i < n_ops) {
        KC_STEP(alt, acc, nxt.a)
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = alt[u];
    }
#undef KC_STEP
#undef KC_APPLY_C
#undef KC_APPLY_0
#undef KC_APPLY_1
#undef KC_APPLY_2
#undef KC_APPLY_3
}
