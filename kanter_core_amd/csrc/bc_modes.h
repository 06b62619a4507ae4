// The all-modes block decoders of bc_modes.hip (KC_BC_ALL_MODES, include/kanter_core_amd.h): every BC7 mode 0-7 and every unsigned
// BC6H mode 1-14, table-driven so that the lanes of a wave, whose blocks are of different modes in a foreign file, run one
// instruction stream.  A block is first reduced to a small state -- its endpoints expanded, the partition's subset word, the
// anchors, where the index sets lie -- and then read texel by texel: the subset from the word, the index from a computed bit
// position (base + n t - the anchors below t), the interpolation.  Every field is read by one bit reader with per-lane positions.
// The tables are the formats' own (tests/bc_modes_ref.py holds the same in numpy); a workgroup stages them in LDS once, the way
// bc_stage_srgb stages its table, because they are indexed per lane.
// Plain C++ without device builtins: included inside namespace kc after bc_blocks.h (bc6h_unq and bc6h_entry are its).
#pragma once

// n <= 16 bits of the block from bit `at`, LSB first; both per lane.  A field that a lane's mode does not have may lie past the
// block: it reads words of the registers, never memory, and its value is not used.
static __device__ __forceinline__ uint32_t bcm_bits(const uint32_t (&b)[4], uint32_t at, uint32_t n)
{
    const uint32_t w = at >> 5, s = at & 31u;
    // every word is read first: a conditional between the elements themselves is compiled to a choice of addresses, which keeps
    // the caller's state in scratch
    const uint32_t b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
    const uint32_t lo = w == 0u ? b0 : w == 1u ? b1 : w == 2u ? b2 : b3;
    const uint32_t hi = w == 0u ? b1 : w == 1u ? b2 : w == 2u ? b3 : 0u;
    const uint32_t v = (uint32_t)((((uint64_t)hi << 32) | lo) >> s);
    return v & ((1u << n) - 1u);
}

// ---------------------------------------------------------------- the partition tables
// Two subsets: bit t of entry p = the subset of texel t.  BC6H uses the first 32.
static __device__ const uint16_t kBcPart2[64] = {
    0xCCCC, 0x8888, 0xEEEE, 0xECC8, 0xC880, 0xFEEC, 0xFEC8, 0xEC80, 0xC800, 0xFFEC, 0xFE80, 0xE800, 0xFFE8, 0xFF00, 0xFFF0, 0xF000,
    0xF710, 0x008E, 0x7100, 0x08CE, 0x008C, 0x7310, 0x3100, 0x8CCE, 0x088C, 0x3110, 0x6666, 0x366C, 0x17E8, 0x0FF0, 0x718E, 0x399C,
    0xAAAA, 0xF0F0, 0x5A5A, 0x33CC, 0x3C3C, 0x55AA, 0x9696, 0xA55A, 0x73CE, 0x13C8, 0x324C, 0x3BDC, 0x6996, 0xC33C, 0x9966, 0x0660,
    0x0272, 0x04E4, 0x4E40, 0x2720, 0xC936, 0x936C, 0x39C6, 0x639C, 0x9336, 0x9CC6, 0x817E, 0xE718, 0xCCF0, 0x0FCC, 0x7744, 0xEE22 };
// Three subsets: bits 2t..2t+1 of entry p = the subset of texel t
static __device__ const uint32_t kBcPart3[64] = {
    0xAA685050u, 0x6A5A5040u, 0x5A5A4200u, 0x5450A0A8u, 0xA5A50000u, 0xA0A05050u, 0x5555A0A0u, 0x5A5A5050u,
    0xAA550000u, 0xAA555500u, 0xAAAA5500u, 0x90909090u, 0x94949494u, 0xA4A4A4A4u, 0xA9A59450u, 0x2A0A4250u,
    0xA5945040u, 0x0A425054u, 0xA5A5A500u, 0x55A0A0A0u, 0xA8A85454u, 0x6A6A4040u, 0xA4A45000u, 0x1A1A0500u,
    0x0050A4A4u, 0xAAA59090u, 0x14696914u, 0x69691400u, 0xA08585A0u, 0xAA821414u, 0x50A4A450u, 0x6A5A0200u,
    0xA9A58000u, 0x5090A0A8u, 0xA8A09050u, 0x24242424u, 0x00AA5500u, 0x24924924u, 0x24499224u, 0x50A50A50u,
    0x500AA550u, 0xAAAA4444u, 0x66660000u, 0xA5A0A5A0u, 0x50A050A0u, 0x69286928u, 0x44AAAA44u, 0x66666600u,
    0xAA444444u, 0x54A854A8u, 0x95809580u, 0x96969600u, 0xA85454A8u, 0x80959580u, 0xAA141414u, 0x96960000u,
    0xAAAA1414u, 0xA05050A0u, 0xA0A5A5A0u, 0x96000000u, 0x40804080u, 0xA9A8A9A8u, 0xAAAAAA44u, 0x2A4A5254u };
// The anchor texels, 4 bits each: bits 0-3 of subset 1 with two subsets, bits 4-7 and 8-11 of subsets 1 and 2 with three
#define KC_A(two, three1, three2) ((two) | (three1) << 4 | (three2) << 8)
static __device__ const uint16_t kBcAnchors[64] = {
    KC_A(15, 3, 15),  KC_A(15, 3, 8),   KC_A(15, 15, 8),  KC_A(15, 15, 3),  KC_A(15, 8, 15),  KC_A(15, 3, 15),  KC_A(15, 15, 3),  KC_A(15, 15, 8),
    KC_A(15, 8, 15),  KC_A(15, 8, 15),  KC_A(15, 6, 15),  KC_A(15, 6, 15),  KC_A(15, 6, 15),  KC_A(15, 5, 15),  KC_A(15, 3, 15),  KC_A(15, 3, 8),
    KC_A(15, 3, 15),  KC_A(2, 3, 8),    KC_A(8, 8, 15),   KC_A(2, 15, 3),   KC_A(2, 3, 15),   KC_A(8, 3, 8),    KC_A(8, 6, 15),   KC_A(15, 10, 8),
    KC_A(2, 5, 3),    KC_A(8, 8, 15),   KC_A(2, 8, 6),    KC_A(2, 6, 10),   KC_A(8, 8, 15),   KC_A(8, 5, 15),   KC_A(2, 15, 10),  KC_A(2, 15, 8),
    KC_A(15, 8, 15),  KC_A(15, 15, 3),  KC_A(6, 3, 15),   KC_A(8, 5, 10),   KC_A(2, 6, 10),   KC_A(8, 10, 8),   KC_A(15, 8, 9),   KC_A(15, 15, 10),
    KC_A(2, 15, 6),   KC_A(8, 3, 15),   KC_A(2, 15, 8),   KC_A(2, 5, 15),   KC_A(2, 15, 3),   KC_A(15, 15, 6),  KC_A(15, 15, 6),  KC_A(6, 15, 8),
    KC_A(6, 3, 15),   KC_A(2, 15, 3),   KC_A(6, 5, 15),   KC_A(8, 5, 15),   KC_A(15, 5, 15),  KC_A(15, 8, 15),  KC_A(2, 5, 15),   KC_A(2, 10, 15),
    KC_A(15, 5, 15),  KC_A(15, 10, 15), KC_A(15, 8, 15),  KC_A(15, 13, 15), KC_A(15, 15, 3),  KC_A(2, 12, 15),  KC_A(2, 3, 15),   KC_A(15, 3, 8) };
#undef KC_A

// ---------------------------------------------------------------- BC7
// A mode: subsets | partition bits << 2 | rotation bits << 5 | index selection bits << 7 | colour bits << 8 | alpha bits << 12 |
// p-bits << 16 (0 none, 1 one per endpoint, 2 one per subset) | index bits << 18 | the second index set's bits << 21.  The fields
// follow one another from bit mode + 1: partition, rotation, index selection, every R, every G, every B, every A (endpoint
// 2 subset + k), the p-bits, the index sets.  Entry 8, the reserved block, has one subset and no endpoint bits; its
// 2-bit indices keep every computed position and width in range, and its texels are 0 whatever they say.
#define KC_M(ns, pb, rb, isb, cb, ab, pk, ib, ib2) ((ns) | (pb) << 2 | (rb) << 5 | (isb) << 7 | (cb) << 8 | (ab) << 12 | (pk) << 16 | (ib) << 18 | (ib2) << 21)
static __device__ const uint32_t kBc7Modes[9] = { KC_M(3u, 4u, 0u, 0u, 4u, 0u, 1u, 3u, 0u), KC_M(2u, 6u, 0u, 0u, 6u, 0u, 2u, 3u, 0u),
                                                  KC_M(3u, 6u, 0u, 0u, 5u, 0u, 0u, 2u, 0u), KC_M(2u, 6u, 0u, 0u, 7u, 0u, 1u, 2u, 0u),
                                                  KC_M(1u, 0u, 2u, 1u, 5u, 6u, 0u, 2u, 3u), KC_M(1u, 0u, 2u, 0u, 7u, 8u, 0u, 2u, 2u),
                                                  KC_M(1u, 0u, 0u, 0u, 7u, 7u, 1u, 4u, 0u), KC_M(2u, 6u, 0u, 0u, 5u, 5u, 1u, 2u, 0u),
                                                  KC_M(1u, 0u, 0u, 0u, 0u, 0u, 0u, 2u, 0u) };
#undef KC_M
// The weights of an n-bit index i at byte (1 << n) - 4 + i: W2, W3, W4
static __device__ const uint8_t kBcWeights[28] = { 0, 21, 43, 64, 0, 9, 18, 27, 37, 46, 55, 64, 0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64 };

// The staged table, in 32-bit words: the two-subset partitions spread to 2 bits a texel like the three-subset ones, the anchor
// words, the modes, the weights
constexpr uint32_t BC7_TAB_P2 = 0, BC7_TAB_P3 = 64, BC7_TAB_ANCHORS = 128, BC7_TAB_MODES = 192, BC7_TAB_WEIGHTS = 201, BC7_TAB_WORDS = 208;

// Word i of the table (i < BC7_TAB_WORDS)
static __device__ __forceinline__ uint32_t bc7_table_word(uint32_t i)
{
    if (i < BC7_TAB_P3) {
        const uint32_t m = kBcPart2[i];
        uint32_t v = 0u;
        for (uint32_t t = 0; t < 16u; ++t) v |= ((m >> t) & 1u) << (2u * t);
        return v;
    }
    if (i < BC7_TAB_ANCHORS) return kBcPart3[i - BC7_TAB_P3];
    if (i < BC7_TAB_MODES) return kBcAnchors[i - BC7_TAB_ANCHORS];
    if (i < BC7_TAB_WEIGHTS) return kBc7Modes[i - BC7_TAB_MODES];
    const uint32_t k = 4u * (i - BC7_TAB_WEIGHTS);
    return (uint32_t)kBcWeights[k] | (uint32_t)kBcWeights[k + 1] << 8 | (uint32_t)kBcWeights[k + 2] << 16 | (uint32_t)kBcWeights[k + 3] << 24;
}

// What is left of a block once its header is read
struct Bc7Block {
    uint32_t b[4];
    uint32_t e0, e1, e2, e3, e4, e5;  // endpoint 2 subset + k as R | G << 8 | B << 16 | A << 24, expanded to 8 bits 
    uint32_t subsets; // 2 bits a texel
    uint32_t a1, a2;  // the anchors of subsets 1 and 2 (16: no such subset); texel 0 is subset 0's
    uint32_t i1, n1;  // the first index set: its first bit and the bits of an index
    uint32_t i2, n2;  // the second one (modes 4 and 5; n2 = 0: none)
    uint32_t sel, rot;
    uint32_t mode;    // 0..7, 8 for the reserved block
};

static __device__ __forceinline__ void bc7_read_header(const uint32_t *tab, Bc7Block &k)
{
    const uint32_t byte0 = k.b[0] & 0xffu;
    const uint32_t m = byte0 ? (uint32_t)__builtin_ctz(byte0) : 8u;
    const uint32_t d = tab[BC7_TAB_MODES + m];
    const uint32_t ns = d & 3u, pb = (d >> 2) & 7u, rb = (d >> 5) & 3u, isb = (d >> 7) & 1u, cb = (d >> 8) & 15u, ab = (d >> 12) & 15u;
    const uint32_t pk = (d >> 16) & 3u, ne = 2u * ns;
    k.mode = m;
    k.n1 = (d >> 18) & 7u;
    k.n2 = (d >> 21) & 3u;
    uint32_t at = m + 1u;
    const uint32_t part = bcm_bits(k.b, at, pb);
    at += pb;
    k.rot = bcm_bits(k.b, at, rb);
    at += rb;
    k.sel = bcm_bits(k.b, at, isb);
    at += isb;
    const uint32_t cbase = at, abase = cbase + 3u * ne * cb, pbase = abase + ne * ab;
    k.i1 = pbase + (pk == 1u ? ne : pk == 2u ? ns : 0u);
    k.i2 = k.i1 + 16u * k.n1 - ns;
    const uint32_t nc = cb + (pk ? 1u : 0u), na = ab + (pk ? 1u : 0u);  // the bits of an endpoint with its p-bit
    auto endpoint = [&](uint32_t e) {  // endpoints past 2 ns read bits that mean something else and are never used
        const uint32_t p = bcm_bits(k.b, pbase + (pk == 2u ? e >> 1 : e), pk ? 1u : 0u);
        uint32_t word = 0u;
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c) {
            const uint32_t n = c < 3u ? cb : ab, nn = c < 3u ? nc : na;
            const uint32_t q = bcm_bits(k.b, c < 3u ? cbase + (c * ne + e) * cb : abase + e * ab, n);
            const uint32_t x = pk ? (q << 1) | p : q;
            uint32_t v = x << (8u - nn);  // nn in 5..8 (alpha: or 0): one repeat of the top bits fills the byte
            v |= v >> nn;
            if (c == 3u) v = ab ? v : 255u;
            word |= (v & 0xffu) << (8u * c);
        }
        return word;
    };
    k.e0 = endpoint(0u), k.e1 = endpoint(1u), k.e2 = endpoint(2u), k.e3 = endpoint(3u), k.e4 = endpoint(4u), k.e5 = endpoint(5u);
    const uint32_t aw = tab[BC7_TAB_ANCHORS + part];
    k.subsets = ns == 2u ? tab[BC7_TAB_P2 + part] : ns == 3u ? tab[BC7_TAB_P3 + part] : 0u;
    k.a1 = ns == 2u ? aw & 15u : ns == 3u ? (aw >> 4) & 15u : 16u;
    k.a2 = ns == 3u ? (aw >> 8) & 15u : 16u;
}

// Texel t (a constant after unrolling) as R | G << 8 | B << 16 | A << 24
static __device__ __forceinline__ uint32_t bc7_texel(const Bc7Block &k, const uint32_t *tab, uint32_t t)
{
    const uint8_t *wt = reinterpret_cast<const uint8_t *>(tab + BC7_TAB_WEIGHTS);
    const uint32_t s = (k.subsets >> (2u * t)) & 3u;
    const uint32_t below = (t > 0u ? 1u : 0u) + (t > k.a1 ? 1u : 0u) + (t > k.a2 ? 1u : 0u);
    const uint32_t anchor = (t == 0u || t == k.a1 || t == k.a2) ? 1u : 0u;
    const uint32_t x1 = bcm_bits(k.b, k.i1 + k.n1 * t - below, k.n1 - anchor);
    const uint32_t n2 = k.n2 ? k.n2 : 2u;  // without a second set its weight is not used
    const uint32_t x2 = bcm_bits(k.b, k.i2 + n2 * t - (t > 0u ? 1u : 0u), n2 - (t == 0u ? 1u : 0u));
    const uint32_t w1 = wt[(1u << k.n1) - 4u + x1], w2 = k.n2 ? wt[(1u << n2) - 4u + x2] : w1;
    const uint32_t wc = k.sel ? w2 : w1, wa = k.sel ? w1 : w2;
        const uint32_t k0 = k.e0, k1 = k.e1, k2 = k.e2, k3 = k.e3, k4 = k.e4, k5 = k.e5;  // read first, as in bcm_bits
    const uint32_t e0 = s == 0u ? k0 : s == 1u ? k2 : k4, e1 = s == 0u ? k1 : s == 1u ? k3 : k5;
    uint32_t v[4];
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c) {
        const uint32_t w = c < 3u ? wc : wa;
        v[c] = ((64u - w) * ((e0 >> (8u * c)) & 0xffu) + w * ((e1 >> (8u * c)) & 0xffu) + 32u) >> 6;
    }
    // rotation r: alpha and channel r - 1 change places
    const uint32_t rot = k.rot;
    const uint32_t al = rot == 0u ? v[3] : rot == 1u ? v[0] : rot == 2u ? v[1] : v[2];
    const uint32_t r = rot == 1u ? v[3] : v[0], g = rot == 2u ? v[3] : v[1], bl = rot == 3u ? v[3] : v[2];
    const uint32_t px = r | (g << 8) | (bl << 16) | (al << 24);
    return k.mode == 8u ? 0u : px;
}

// ---------------------------------------------------------------- BC6H
// A two-subset mode (1-10): bits of endpoint 0 | the stored bits of the other endpoints of R << 4, G << 8, B << 12 | whether
// these are signed deltas << 16.  Every mode keeps the same places for the bulk of its header: the low (up to 10) bits of R0,
// G0, B0 at bits 5, 15, 25; R1, R2, R3 at 35, 65, 71; G1 at 45, the low 4 bits of G2 and G3 at 41 and 51; B1 at 55, the low 4
// bits of B2 at 61; the partition at 77.  What differs from mode to mode is a handful of single bits.
#define KC_H(nb, lr, lg, lb, tr) ((nb) | (lr) << 4 | (lg) << 8 | (lb) << 12 | (tr) << 16)
static __device__ const uint32_t kBc6hModes[10] = { KC_H(10u, 5u, 5u, 5u, 1u), KC_H(7u, 6u, 6u, 6u, 1u), KC_H(11u, 5u, 4u, 4u, 1u), KC_H(11u, 4u, 5u, 4u, 1u),
                                                    KC_H(11u, 4u, 4u, 5u, 1u), KC_H(9u, 5u, 5u, 5u, 1u), KC_H(8u, 6u, 5u, 5u, 1u),  KC_H(8u, 5u, 6u, 5u, 1u),
                                                    KC_H(8u, 5u, 5u, 6u, 1u),  KC_H(6u, 6u, 6u, 6u, 0u) };
#undef KC_H
// The single bits of a mode, up to 12: block bit | destination << 7.  The destinations are bits of one word: G2[4], G2[5],
// G3[4], G3[5], B2[4], B2[5], B3[0..5], R0[10], G0[10], B0[10]; 15: no bit
enum { H_G2_4, H_G2_5, H_G3_4, H_G3_5, H_B2_4, H_B2_5, H_B3_0, H_B3_1, H_B3_2, H_B3_3, H_B3_4, H_B3_5, H_R0_10, H_G0_10, H_B0_10, H_NONE };
#define KC_X(at, dst) (uint16_t)((at) | (dst) << 7)
#define KC_N KC_X(0, H_NONE)
static __device__ const uint16_t kBc6hBits[10][12] = {
    { KC_X(2, H_G2_4), KC_X(3, H_B2_4), KC_X(4, H_B3_4), KC_X(40, H_G3_4), KC_X(50, H_B3_0), KC_X(60, H_B3_1), KC_X(70, H_B3_2), KC_X(76, H_B3_3), KC_N, KC_N,
      KC_N, KC_N },
    { KC_X(2, H_G2_5), KC_X(3, H_G3_4), KC_X(4, H_G3_5), KC_X(12, H_B3_0), KC_X(13, H_B3_1), KC_X(14, H_B2_4), KC_X(22, H_B2_5), KC_X(23, H_B3_2),
      KC_X(24, H_G2_4), KC_X(32, H_B3_3), KC_X(33, H_B3_5), KC_X(34, H_B3_4) },
    { KC_X(40, H_R0_10), KC_X(49, H_G0_10), KC_X(50, H_B3_0), KC_X(59, H_B0_10), KC_X(60, H_B3_1), KC_X(70, H_B3_2), KC_X(76, H_B3_3), KC_N, KC_N, KC_N, KC_N,
      KC_N },
    { KC_X(39, H_R0_10), KC_X(40, H_G3_4), KC_X(50, H_G0_10), KC_X(59, H_B0_10), KC_X(60, H_B3_1), KC_X(69, H_B3_0), KC_X(70, H_B3_2), KC_X(75, H_G2_4),
      KC_X(76, H_B3_3), KC_N, KC_N, KC_N },
    { KC_X(39, H_R0_10), KC_X(40, H_B2_4), KC_X(49, H_G0_10), KC_X(50, H_B3_0), KC_X(60, H_B0_10), KC_X(69, H_B3_1), KC_X(70, H_B3_2), KC_X(75, H_B3_4),
      KC_X(76, H_B3_3), KC_N, KC_N, KC_N },
    { KC_X(14, H_B2_4), KC_X(24, H_G2_4), KC_X(34, H_B3_4), KC_X(40, H_G3_4), KC_X(50, H_B3_0), KC_X(60, H_B3_1), KC_X(70, H_B3_2), KC_X(76, H_B3_3), KC_N,
      KC_N, KC_N, KC_N },
    { KC_X(13, H_G3_4), KC_X(14, H_B2_4), KC_X(23, H_B3_2), KC_X(24, H_G2_4), KC_X(33, H_B3_3), KC_X(34, H_B3_4), KC_X(50, H_B3_0), KC_X(60, H_B3_1), KC_N,
      KC_N, KC_N, KC_N },
    { KC_X(13, H_B3_0), KC_X(14, H_B2_4), KC_X(23, H_G2_5), KC_X(24, H_G2_4), KC_X(33, H_G3_5), KC_X(34, H_B3_4), KC_X(40, H_G3_4), KC_X(60, H_B3_1),
      KC_X(70, H_B3_2), KC_X(76, H_B3_3), KC_N, KC_N },
    { KC_X(13, H_B3_1), KC_X(14, H_B2_4), KC_X(23, H_B2_5), KC_X(24, H_G2_4), KC_X(33, H_B3_5), KC_X(34, H_B3_4), KC_X(40, H_G3_4), KC_X(50, H_B3_0),
      KC_X(70, H_B3_2), KC_X(76, H_B3_3), KC_N, KC_N },
    { KC_X(11, H_G3_4), KC_X(12, H_B3_0), KC_X(13, H_B3_1), KC_X(14, H_B2_4), KC_X(21, H_G2_5), KC_X(22, H_B2_5), KC_X(23, H_B3_2), KC_X(24, H_G2_4),
      KC_X(31, H_G3_5), KC_X(32, H_B3_3), KC_X(33, H_B3_5), KC_X(34, H_B3_4) },
};
#undef KC_N
#undef KC_X

// The staged table, in 32-bit words: the 32 partitions (16-bit masks), their anchors, the modes, the modes' single bits in pairs
constexpr uint32_t BC6H_TAB_P2 = 0, BC6H_TAB_ANCHORS = 32, BC6H_TAB_MODES = 64, BC6H_TAB_BITS = 74, BC6H_TAB_WORDS = 134;

static __device__ __forceinline__ uint32_t bc6h_table_word(uint32_t i)
{
    if (i < BC6H_TAB_ANCHORS) return kBcPart2[i];
    if (i < BC6H_TAB_MODES) return kBcAnchors[i - BC6H_TAB_ANCHORS] & 15u;
    if (i < BC6H_TAB_BITS) return kBc6hModes[i - BC6H_TAB_MODES];
    const uint32_t k = i - BC6H_TAB_BITS;
    return (uint32_t)kBc6hBits[k / 6u][2u * (k % 6u)] | (uint32_t)kBc6hBits[k / 6u][2u * (k % 6u) + 1u] << 16;
}

struct Bc6hBlock {
    uint32_t b[4];
    uint32_t u01[3], u23[3];  // per channel the 16-bit endpoints 0 | 1 << 16 of subset 0 and 2 | 3 << 16 of subset 1
    uint32_t subsets;         // bit t: the subset of texel t (0 in the single-subset modes)
    uint32_t a1;              // subset 1's anchor (16: none)
    uint32_t i1, n1;          // the index set
};

static __device__ __forceinline__ uint32_t bc6h_sext(uint32_t x, uint32_t n) { return (uint32_t)((int32_t)(x << (32u - n)) >> (32u - n)); }

static __device__ __forceinline__ void bc6h_read_header(const uint32_t *tab, Bc6hBlock &k)
{
    const uint32_t f = k.b[0] & 31u;
    const bool two = (f & 3u) != 3u, single = !two && f < 16u;
    const uint32_t mi = (f & 2u) == 0u ? f & 1u : two ? 2u + (f >> 2) : 0u;  // modes 1-10 as 0-9; the others read mode 1's table in vain
    const uint32_t d = tab[BC6H_TAB_MODES + mi];
    // the single bits of the mode, gathered into one word
    uint32_t x = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 12u; ++j) {
        const uint32_t ent = (tab[BC6H_TAB_BITS + 6u * mi + (j >> 1)] >> (16u * (j & 1u))) & 0xffffu;
        x |= bcm_bits(k.b, ent & 127u, 1u) << (ent >> 7);
    }
    const uint32_t nb2 = d & 15u, tr = (d >> 16) & 1u, mask2 = (1u << nb2) - 1u;
    const uint32_t part = bcm_bits(k.b, 77u, 5u);
    // the single-subset modes 11-14: endpoint 0 in n = 10, 11, 12, 16 bits, its bits above the tenth at the top of the second
    // group in reverse order, and endpoint 1 whole (mode 11) or as a signed delta of 9, 8, 4 bits at the bottom of that group
    const uint32_t m1 = (f >> 2) & 3u;
    const uint32_t nb1 = m1 == 3u ? 16u : 10u + m1, db1 = m1 == 3u ? 4u : 10u - m1;
    const uint32_t nb = two ? nb2 : nb1;
#pragma unroll
    for (uint32_t c = 0; c < 3u; ++c) {
        const uint32_t low = bcm_bits(k.b, 5u + 10u * c, 10u);
        // two subsets
        const uint32_t len = (d >> (4u + 4u * c)) & 15u;
        uint32_t e0 = (low & mask2) | ((x >> (H_R0_10 + c)) & 1u) << 10;
        uint32_t e1, e2, e3;
        if (c == 0u) {
            e1 = bcm_bits(k.b, 35u, len);
            e2 = bcm_bits(k.b, 65u, len);
            e3 = bcm_bits(k.b, 71u, len);
        } else if (c == 1u) {
            e1 = bcm_bits(k.b, 45u, len);
            e2 = (bcm_bits(k.b, 41u, 4u) | ((x >> H_G2_4) & 3u) << 4) & ((1u << len) - 1u);
            e3 = (bcm_bits(k.b, 51u, 4u) | ((x >> H_G3_4) & 3u) << 4) & ((1u << len) - 1u);
        } else {
            e1 = bcm_bits(k.b, 55u, len);
            e2 = (bcm_bits(k.b, 61u, 4u) | ((x >> H_B2_4) & 3u) << 4) & ((1u << len) - 1u);
            e3 = (x >> H_B3_0) & ((1u << len) - 1u);
        }
        if (tr) {
            e1 = (e0 + bc6h_sext(e1, len)) & mask2;
            e2 = (e0 + bc6h_sext(e2, len)) & mask2;
            e3 = (e0 + bc6h_sext(e3, len)) & mask2;
        }
        // one subset
        const uint32_t grp = bcm_bits(k.b, 35u + 10u * c, 10u);
        uint32_t rev = 0u;  // bit j = the group's bit 9 - j = endpoint 0's bit 10 + j
#pragma unroll
        for (uint32_t j = 0; j < 6u; ++j) rev |= ((grp >> (9u - j)) & 1u) << j;
        const uint32_t s0 = low | (rev & ((1u << (nb1 - 10u)) - 1u)) << 10;
        const uint32_t s1 = m1 == 0u ? grp : (s0 + bc6h_sext(grp & ((1u << db1) - 1u), db1)) & ((1u << nb1) - 1u);
        if (!two) {
            e0 = s0;
            e1 = s1;
        }
        const bool live = two || single;  // a reserved mode field: the endpoints stay 0 and every texel interpolates to 0
        k.u01[c] = live ? bc6h_unq(e0, nb) | bc6h_unq(e1, nb) << 16 : 0u;
        k.u23[c] = two ? bc6h_unq(e2, nb) | bc6h_unq(e3, nb) << 16 : 0u;
    }
    k.subsets = two ? tab[BC6H_TAB_P2 + part] : 0u;
    k.a1 = two ? tab[BC6H_TAB_ANCHORS + part] : 16u;
    k.i1 = two ? 82u : 65u;
    k.n1 = two ? 3u : 4u;
}

// Texel t (a constant after unrolling): *rg = R | G << 16 and *bl = B as half bit patterns
static __device__ __forceinline__ void bc6h_texel(const Bc6hBlock &k, uint32_t t, uint32_t *rg, uint32_t *bl)
{
    const uint32_t s = (k.subsets >> t) & 1u;
    const uint32_t below = (t > 0u ? 1u : 0u) + (t > k.a1 ? 1u : 0u);
    const uint32_t anchor = (t == 0u || t == k.a1) ? 1u : 0u;
    const uint32_t i = bcm_bits(k.b, k.i1 + k.n1 * t - below, k.n1 - anchor);
    const uint32_t w = k.n1 == 4u ? (64u * i + 7u) / 15u : (64u * i + 3u) / 7u;  // W4, W3
    uint32_t v[3];
#pragma unroll
    for (uint32_t c = 0; c < 3u; ++c) {
        const uint32_t ua = k.u01[c], ub = k.u23[c];  // read first, as in bcm_bits
        const uint32_t u = s ? ub : ua;
        v[c] = bc6h_entry(u & 0xffffu, u >> 16, w);
    }
    *rg = v[0] | v[1] << 16;
    *bl = v[2];
}
