// Stand-alone host program for tests/test_specialize_inflight.py: csrc/chain_codegen.cpp is compiled together with this file
// under AddressSanitizer + UndefinedBehaviorSanitizer and its generator is run over a few hundred random signatures, every
// cache-policy mask, flat and pitched, under every chain_quads setting; then over flat programs with packed inputs and over
// up-sampling signatures.  No device, no compiler run: text only.  Checks on the way: a text comes back for every valid program;
// a setting of 1 gives the one-quad text; a program that is not eligible (pitched, a divide or pow step, more than 16 records,
// no plain input beside a nontemporal stream) gives the one-quad text under every setting.
// Output: the "ok:" line, then per group of texts its name, the number of texts and an FNV-1a 64 over them in sweep order
// (each text with its terminating zero).  tests/golden/chain_kernel_texts.txt pins it: the embedded headers are placeholders
// here, so the digests depend on the generator alone.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

#include "kc_runtime.hpp"

namespace kc {
// what the generator takes from other units: the embedded device headers (their text does not matter here)
extern const char kJitChainProgramH[] = "/* chain_program.h */\n";
extern const char kJitPowPositiveInc[] = "/* pow_positive.inc */\n";
extern const char kJitUpsampleH[] = "/* upsample.h */\n";
extern const char kJitUpsampleChainInc[] = "/* upsample_chain.inc */\n";
extern const char kJitChainPackH[] = "/* chain_pack.h */\n";
}  // namespace kc

using namespace kc;

static int fail(const char *what, int i)
{
    std::fprintf(stderr, "signature %d: %s\n", i, what);
    return 1;
}

struct Group {
    const char *name;
    unsigned count = 0;
    uint64_t h = 1469598103934665603ull;
    void add(const std::string &text)
    {
        count++;
        for (size_t i = 0; i <= text.size(); ++i) h = (h ^ (unsigned char)text.c_str()[i]) * 1099511628211ull;
    }
    void print() const { std::printf("%s %u %016llx\n", name, count, (unsigned long long)h); }
};

static const uint32_t plain_codes[] = { CH_ADD, CH_SUB_L, CH_SUB_R, CH_MUL, CH_ADD_INV, CH_SUBL_INV, CH_SUBR_INV, CH_MUL_INV };
constexpr unsigned kSeed = 20240611u;

static void set_word(ChainProgram &P, uint32_t k, uint32_t word) { ((k & 1u) ? P.step[0][k / 2].b : P.step[0][k / 2].a).word = word; }

int main()
{
    Group flat_one{ "one_quad_flat" }, pitched{ "pitched" }, quads_rule{ "quads_rule" }, quads_2{ "quads_2" }, quads_4{ "quads_4" },
        packed{ "packed" }, upsampling{ "upsampling" };
    std::mt19937 rng(kSeed);
    auto pick = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    const uint32_t other_codes[] = { CH_DIV_L, CH_DIV_R, CH_POW_L, CH_POW_R };
    int multi = 0;
    for (int i = 0; i < 400; ++i) {
        ChainProgram P;
        std::memset(&P, 0, sizeof P);
        P.n_in = 1 + pick(i % 7 == 0 ? KC_CHAIN_MAX_IN : 4);
        P.n_ops = 1 + pick(i % 5 == 0 ? KC_CHAIN_MAX_OPS : 20);
        P.start_src = (int)pick(P.n_in + 1) - 1;
        const bool flat = pick(4) != 0;
        P.rows = flat ? 1u : 1u + pick(4096) + 1u;
        P.row_units = 1u + pick(1u << 20);
        bool plain_only = true, saved = false;
        for (uint32_t k = 0; k < P.n_ops; ++k) {
            uint32_t code = plain_codes[pick(8)];
            if (pick(40) == 0) code = other_codes[pick(4)];
            uint32_t from = pick(P.n_in + 1), level = 0;  // 0: the constant
            if (saved && pick(6) == 0) {
                from = KC_CHAIN_SRC_SAVED;
                level = pick(KC_CHAIN_MAX_SAVED);
            } else if (from && pick(12) == 0) {
                code = CH_SAVE_LOAD;
                level = pick(KC_CHAIN_MAX_SAVED);
                saved = true;
            }
            plain_only &= code != CH_DIV_L && code != CH_DIV_R && code != CH_POW_L && code != CH_POW_R;
            set_word(P, k, code | from << 8 | level << 16);
        }
        uint32_t inputs = 0;
        for (uint32_t k = 0; k < P.n_in; ++k) inputs |= KC_CHAIN_NT_BIT(k);
        const uint32_t one_input = pick(P.n_in);  // (KC_CHAIN_NT_BIT evaluates its argument more than once)
        const uint32_t masks[] = { 0u, 0x100u, inputs, inputs | 0x100u, (uint32_t)rng() & (inputs | 0x100u), KC_CHAIN_NT_BIT(one_input) };
        for (uint32_t mask : masks) {
            P.nt_mask = mask;
            const bool eligible = flat && plain_only && P.n_ops <= 16 && mask != 0 && (mask & inputs) != inputs;
            if (specialize_set_chain_quads(1) != KC_OK) return fail("chain_quads = 1 refused", i);
            const std::string one = specialize_source(P);
            if (one.empty()) return fail("no text", i);
            (flat ? flat_one : pitched).add(one);
            for (int q : { 0, 2, 4 }) {
                if (specialize_set_chain_quads(q) != KC_OK) return fail("chain_quads refused", i);
                const std::string text = specialize_source(P);
                if (text.empty()) return fail("no text", i);
                if (!eligible && text != one) return fail("a program that is not eligible left the one-quad text", i);
                if (eligible && text == one) return fail("an eligible program kept the one-quad text", i);
                multi += eligible;
                if (eligible) (q == 0 ? quads_rule : q == 2 ? quads_2 : quads_4).add(text);
            }
        }
    }
    if (specialize_set_chain_quads(3) == KC_OK || specialize_set_chain_quads(-1) == KC_OK) return fail("chain_quads = 3 or -1 accepted", -1);
    specialize_set_chain_quads(0);

    // flat programs that read some inputs from their packed copies, every tier per input, under the rule's own quads
    rng.seed(kSeed);
    for (int i = 0; i < 200; ++i) {
        ChainProgram P;
        std::memset(&P, 0, sizeof P);
        P.n_in = 1 + pick(i % 7 == 0 ? KC_CHAIN_MAX_IN : 4);
        P.n_ops = 1 + pick(16);
        P.start_src = (int)pick(P.n_in + 1) - 1;
        P.rows = 1;
        P.row_units = 1u + pick(1u << 20);
        for (uint32_t k = 0; k < P.n_ops; ++k) set_word(P, k, plain_codes[pick(8)] | pick(P.n_in + 1) << 8);
        uint32_t inputs = 0, tiers = 0;
        for (uint32_t k = 0; k < P.n_in; ++k) {
            inputs |= KC_CHAIN_NT_BIT(k);
            if (k < 16) tiers |= pick(3) << (2 * k);
        }
        if (!tiers) tiers = 1u + pick(2);
        P.in_tiers = tiers;
        for (uint32_t mask : { 0u, inputs | 0x100u, (uint32_t)rng() & (inputs | 0x100u) }) {
            P.nt_mask = mask;
            const std::string text = specialize_source(P);
            if (text.empty()) return fail("no text for a packed program", i);
            if (text.find("pack_decode_") == std::string::npos) return fail("a packed program decodes nothing", i);
            packed.add(text);
        }
    }

    // programs inside the up-sampling kernel: taps 1 and 3, the 256- and the 1024-column tile
    rng.seed(kSeed);
    for (int i = 0; i < 200; ++i) {
        ChainProgram P;
        std::memset(&P, 0, sizeof P);
        P.n_in = 1 + (uint32_t)i % KC_CHAIN_INTERP_IN;
        P.n_ops = 1 + pick(i % 5 == 0 ? KC_CHAIN_MAX_OPS : 20);
        P.start_src = (int)pick(P.n_in + 1) - 1;
        for (uint32_t k = 0; k < P.n_ops; ++k) set_word(P, k, plain_codes[pick(8)] | pick(P.n_in + 1) << 8);
        P.nt_mask = (uint32_t)rng() & 0x1ffu;  // bits of the resampled operand and of absent inputs drop out of the signature
        for (uint32_t taps : { 1u, 3u })
            for (uint32_t tile_w : { 256u, 1024u }) {
                UpsampleArgs U{};
                U.H.taps = U.V.taps = taps;
                U.tile_w = tile_w;
                const std::string text = specialize_source(P, &U);
                if (text.empty()) return fail("no text for an up-sampling program", i);
                upsampling.add(text);
            }
    }

    std::printf("ok: 400 programs x 6 masks, %d texts with more than one quad per lane\n", multi);
    for (const Group *g : { &flat_one, &pitched, &quads_rule, &quads_2, &quads_4, &packed, &upsampling }) g->print();
    return 0;
}
