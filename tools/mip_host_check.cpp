// Stand-alone check of the mip chain's host arithmetic under AddressSanitizer and UndefinedBehaviorSanitizer: the level counts,
// the BC chain layout, the DDS header, the constant fold and the plan of a chain's launches, at ordinary and extreme sizes, with exact-size output arrays so
// that a write past them is seen.  No device is needed.  Build the library first (python -m kanter_core_amd.build), compile the
// host sources of kanter_core_amd/build.py's SOURCES and this file with
//     clang++ -x c++ -O1 -g -std=c++17 -fno-fast-math -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//             -D__HIP_PLATFORM_AMD__ -I<rocm>/include -Iinclude -Ikanter_core_amd/csrc -c ...
// link them with the regular build's device objects (kanter_core_amd/csrc/build/*.o of the .hip units, jit_texts.o) and
// -lamdhip64 -lz -ldl into a program, and run it: it prints "mip host check: ok" and exits 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/kanter_core_amd.h"
#include "kc_runtime.hpp"  // kc::mip_const_fold, kc::mip_plan

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

static uint32_t bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static uint64_t level_texels(uint32_t w, uint32_t h, uint32_t k) { return (uint64_t)std::max(1u, w >> k) * std::max(1u, h >> k); }

// The plan of a chain's launches (kc::mip_plan) for four planes read and written, by what a plan must be rather than by the
// code that makes it: the first step reads level 0, every step reads the level the step before it ended on, the last ends on
// level L - 1 and every level below 0 is written once; a step fuses levels only while both extents still halve, six at the
// most, and none under per_level; where the first step's bytes fit the cache budget no step is nontemporal.
static void check_plan(uint32_t w, uint32_t h, uint32_t L, bool per_level)
{
    const std::vector<kc::MipStep> plan = kc::mip_plan(w, h, L, per_level, 4, 4, 4);
    std::vector<uint32_t> written(L, 0);  // exactly L entries
    uint32_t next = 0;
    for (const kc::MipStep &s : plan) {
        CHECK(s.k == next && s.k + 1 < L);
        CHECK(s.sw == std::max(1u, w >> s.k) && s.sh == std::max(1u, h >> s.k));
        const uint32_t small = std::min(s.sw, s.sh);
        CHECK(s.fused <= 6 && (1u << s.fused) <= small);
        CHECK((s.fused == 0) == (per_level || small < 2));
        CHECK(s.last() == s.k + std::max(s.fused, 1u) && s.last() < L);
        for (uint32_t k = s.k + 1; k <= s.last(); ++k) written[k]++;
        next = s.last();
    }
    CHECK(next == L - 1 && written[0] == 0);
    for (uint32_t k = 1; k < L; ++k) CHECK(written[k] == 1);
    const uint64_t budget = (uint64_t)kc::options().cache_budget_mb << 20;
    if (L > 1 && 16 * (level_texels(w, h, 0) + level_texels(w, h, 1)) < budget)
        for (const kc::MipStep &s : plan) CHECK(!s.nt);
}

// the fused walks the device tests pin: (k, fused) of every step
static void check_walk(uint32_t w, uint32_t h, std::vector<std::pair<uint32_t, uint32_t>> want)
{
    uint32_t L = 0;
    CHECK(kc_mip_level_count(w, h, &L) == KC_OK);
    const std::vector<kc::MipStep> plan = kc::mip_plan(w, h, L, false, 4, 4, 4);
    CHECK(plan.size() == want.size());
    for (size_t i = 0; i < plan.size(); ++i) CHECK(plan[i].k == want[i].first && plan[i].fused == want[i].second);
}

int main()
{
    const uint32_t sizes[] = { 1, 2, 3, 4, 5, 63, 64, 65, 70, 130, 4096, 65535, 65536, 1u << 20, 0x7fffffffu, 0x80000000u, 0xffffffffu };
    const int formats[] = { KC_BC1, KC_BC3, KC_BC4, KC_BC5, KC_BC7 };
    for (uint32_t w : sizes)
        for (uint32_t h : sizes) {
            uint32_t L = 0;
            CHECK(kc_mip_level_count(w, h, &L) == KC_OK);
            const uint32_t m = w > h ? w : h;
            CHECK(L >= 1 && L <= 32 && (m >> (L - 1)) == 1);
            if (h <= 65536) {
                check_plan(w, h, L, false);
                check_plan(w, h, L, true);
            }
            for (int f : formats) {
                uint32_t n = 0;
                size_t total = 0;
                std::vector<size_t> offs(L);  // exactly L entries
                const int s = kc_bc_mip_layout(w, h, f, &n, offs.data(), L, &total);
                const bool fits = (((uint64_t)w + 3) / 4) * (((uint64_t)h + 3) / 4) <= (1ull << 31);
                CHECK(s == (fits ? KC_OK : KC_ERR_INVALID_ARG));
                CHECK(n == L);
                if (fits) {
                    CHECK(offs[0] == 0);
                    for (uint32_t k = 1; k < L; ++k) CHECK(offs[k] > offs[k - 1]);
                    CHECK(total - offs[L - 1] == (f == KC_BC1 || f == KC_BC4 ? 8u : 16u));
                }
                if (L > 1) CHECK(kc_bc_mip_layout(w, h, f, &n, offs.data(), L - 1, &total) == KC_ERR_INVALID_ARG);
                std::vector<uint8_t> hdr(148);  // exactly 148 bytes
                size_t hb = 0;
                const int hs = kc_dds_header(w, h, f, f == KC_BC1 || f == KC_BC3 || f == KC_BC7 ? KC_BC_SRGB : 0u, L, hdr.data(), &hb);
                const bool says = (((uint64_t)w + 3) / 4) * (((uint64_t)h + 3) / 4) * (f == KC_BC1 || f == KC_BC4 ? 8 : 16) <= 0xffffffffull;
                CHECK(hs == (says ? KC_OK : KC_ERR_INVALID_ARG));
                if (says) CHECK(hb == 148 && std::memcmp(hdr.data(), "DDS ", 4) == 0);
                CHECK(kc_dds_header(w, h, f, 0, L + 1, hdr.data(), &hb) == KC_ERR_INVALID_ARG);
            }
        }
    CHECK(kc_mip_level_count(0, 0, nullptr) == KC_ERR_INVALID_ARG);
    CHECK(kc_bc_mip_layout(0, 0, 0, nullptr, nullptr, 0, nullptr) == KC_ERR_INVALID_ARG);
    CHECK(kc_dds_header(0, 0, 0, 0, 0, nullptr, nullptr) == KC_ERR_INVALID_ARG);
    // the pixel entries: argument checks, then the device that was never initialised
    CHECK(kc_image_build_mips(nullptr, 0, nullptr, 0, nullptr) == KC_ERR_INVALID_ARG);
    CHECK(kc_image_to_bc_mips(nullptr, KC_BC1, 0, nullptr, 0) == KC_ERR_INVALID_ARG);
    CHECK(kc_image_to_bc_mips_device(nullptr, KC_BC1, 0, nullptr, 0, nullptr) == KC_ERR_INVALID_ARG);
    CHECK(kc_image_write_dds(nullptr, nullptr, KC_BC1, 0, 1) == KC_ERR_INVALID_ARG);
    CHECK(kc_live_graph_buffer_bc_mips(nullptr, 0, 0, KC_BC1, 0, nullptr, 0, nullptr) == KC_ERR_INVALID_ARG);
    // the constant fold: ((c + c) + (c + c)) * 0.25f in f32, no flush, no shortcut
    CHECK(bits(kc::mip_const_fold(0.6f)) == bits(0.6f));
    CHECK(std::isinf(kc::mip_const_fold(3e38f)) && kc::mip_const_fold(-3e38f) < 0);
    CHECK(bits(kc::mip_const_fold(-0.0f)) == 0x80000000u);
    float tiny, three;
    const uint32_t one = 1, thr = 3;
    std::memcpy(&tiny, &one, 4);
    std::memcpy(&three, &thr, 4);
    CHECK(bits(kc::mip_const_fold(tiny)) == 1u && bits(kc::mip_const_fold(three)) == 3u);
    CHECK(std::isnan(kc::mip_const_fold(NAN)));
    check_walk(64, 64, { { 0, 6 } });
    check_walk(256, 256, { { 0, 6 }, { 6, 2 } });
    check_walk(130, 70, { { 0, 6 }, { 6, 0 } });
    check_walk(1, 5, { { 0, 0 }, { 1, 0 } });
    check_walk(1024, 512, { { 0, 6 }, { 6, 3 }, { 9, 0 } });
    // four planes of 4096 x 4096: the first launch is nontemporal exactly when what it reads and writes exceeds the cache budget
    const uint64_t budget = (uint64_t)kc::options().cache_budget_mb << 20;
    CHECK(kc::mip_plan(4096, 4096, 13, false, 4, 4, 4)[0].nt == (16 * (level_texels(4096, 4096, 0) + level_texels(4096, 4096, 1)) > budget));
    std::puts("mip host check: ok");
    return 0;
}
