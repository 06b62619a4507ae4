// Compiled chain kernels, the pure part (chain_codegen.cpp): what identifies a kernel, and its source text.  No HIP runtime call,
// no context, no file, no thread; the embedded device headers (kJit*, build.py) are its only externals.
#pragma once
#include <string>

#include "kc_runtime.hpp"

namespace kc {

// Everything the generated code depends on (constants and pointers do not).  Built by make_signature / signature_of only, which
// normalise it: two launches that run the same kernel have equal signatures.
struct Signature {
    uint32_t n_in = 0, n_ops = 0;
    int32_t start_src = 0;
    bool flat = false;
    // up_taps > 0: the program runs inside the integer-ratio up-sampling kernel (upsample_chain.inc), input slot
    // n_in - 1 being the resampled operand; up_wide = its 1024-column tile form
    uint32_t up_taps = 0;
    bool up_wide = false;
    uint32_t nt_mask = 0;  // ChainProgram::nt_mask: which loads / stores carry the nontemporal hint (plain chain kernels)
    uint32_t quads = 1;    // float4 per lane (chain_quads_for); the grid of a launch follows from it
    uint32_t in_tiers = 0; // ChainProgram::in_tiers: which inputs are read from their packed copies (plain flat chain kernels)
    uint32_t word[KC_CHAIN_MAX_OPS] = {};

    bool operator==(const Signature &o) const;  // over the fields above, n_ops words
    // The serialised form: what the kernel name and the cache file name are hashed from, and what a cache file stores.
    std::string key() const;
};
struct SignatureHash {
    size_t operator()(const Signature &s) const;
};

// The signature of a program given by value.  total_units: rows * row_units of the launch where there is one.
Signature make_signature(const uint32_t *words, uint32_t n_ops, uint32_t n_in, int32_t start_src, bool flat, uint32_t nt_mask, uint32_t in_tiers,
                         uint32_t up_taps, bool up_wide, uint64_t total_units = 0);
Signature signature_of(const ChainProgram &P, const UpsampleArgs *U = nullptr);
bool has_div_or_pow(const uint32_t *words, uint32_t n_ops);

int spec_wg();  // workgroup size of the plain generated kernels
std::string kernel_name(const Signature &s);
std::string generate(const Signature &s);  // empty: a step code the form does not know

}  // namespace kc
