// Stand-alone check of the mip chain's host arithmetic under AddressSanitizer and UndefinedBehaviorSanitizer: the level counts,
// the BC chain layout, the DDS header and the constant fold, at ordinary and extreme sizes, with exact-size output arrays so
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

namespace kc {
float mip_const_fold(float c);
}

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
    std::puts("mip host check: ok");
    return 0;
}
