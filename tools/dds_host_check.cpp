// Stand-alone check of kc_dds_parse under AddressSanitizer and UndefinedBehaviorSanitizer: the parser is arithmetic on a
// caller's bytes, so every buffer here is a heap block of exactly the size passed in and a read past it is seen.  Headers of
// kc_dds_header parse back at ordinary and extreme sizes, truncated at every length; then headers with random words in every
// field, which must come back with one of the three documented codes and, on KC_OK, fields that fit the buffer.  No device is
// needed.  Build and link as tools/mip_host_check.cpp says; the program prints "dds host check: ok" and exits 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/kanter_core_amd.h"

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

// kc_dds_parse of a copy of the first n bytes in a heap block of exactly n bytes
static int parse_exact(const std::vector<uint8_t> &file, size_t n, kc_dds_info *info)
{
    uint8_t *p = (uint8_t *)std::malloc(n ? n : 1);
    std::memcpy(p, file.data(), n);
    const int s = kc_dds_parse(p, n, info);
    std::free(p);
    return s;
}

static uint32_t rnd(uint64_t &state)
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 32);
}

int main()
{
    const uint32_t sizes[] = { 1, 2, 3, 4, 5, 63, 64, 65, 130, 4096 };
    const int formats[] = { KC_BC1, KC_BC3, KC_BC4, KC_BC5, KC_BC7 };
    for (uint32_t w : sizes)
        for (uint32_t h : sizes)
            for (int f : formats)
                for (uint32_t flags = 0; flags < 2; ++flags) {
                    if (flags && (f == KC_BC4 || f == KC_BC5)) continue;
                    uint32_t L = 0;
                    CHECK(kc_mip_level_count(w, h, &L) == KC_OK);
                    std::vector<size_t> offs(L);
                    size_t total = 0;
                    CHECK(kc_bc_mip_layout(w, h, f, nullptr, offs.data(), L, &total) == KC_OK);
                    for (uint32_t levels : { 1u, L }) {
                        std::vector<uint8_t> file(148 + (levels == L ? total : offs[levels]), 0);
                        CHECK(kc_dds_header(w, h, f, flags, levels, file.data(), nullptr) == KC_OK);
                        kc_dds_info info;
                        CHECK(parse_exact(file, file.size(), &info) == KC_OK);
                        CHECK(info.width == w && info.height == h && info.format == f && info.flags == flags && info.levels == levels);
                        CHECK(info.data_offset == 148 && info.data_offset + info.data_bytes == file.size());
                        if (w <= 5 && h <= 5)  // every shorter buffer is refused, none is read past
                            for (size_t n = 0; n < file.size(); ++n) CHECK(parse_exact(file, n, &info) == KC_ERR_INVALID_ARG);
                    }
                }
    // extents whose chain does not fit any buffer: refused by arithmetic, nothing is allocated for them
    {
        std::vector<uint8_t> file(148, 0);
        CHECK(kc_dds_header(16, 16, KC_BC7, 0, 1, file.data(), nullptr) == KC_OK);
        const uint32_t big[] = { 0x7fffffffu, 0x80000000u, 0xffffffffu };
        for (uint32_t w : big)
            for (uint32_t h : big) {
                std::memcpy(file.data() + 12, &h, 4);
                std::memcpy(file.data() + 16, &w, 4);
                kc_dds_info info;
                CHECK(parse_exact(file, file.size(), &info) == KC_ERR_INVALID_ARG);
            }
    }
    // random words in a header of either form
    uint64_t state = 0x9e3779b97f4a7c15ull;
    for (int it = 0; it < 200000; ++it) {
        std::vector<uint8_t> file(148 + rnd(state) % 600, 0);
        CHECK(kc_dds_header(1 + rnd(state) % 40, 1 + rnd(state) % 40, formats[rnd(state) % 5], 0, 1, file.data(), nullptr) == KC_OK);
        const int edits = 1 + (int)(rnd(state) % 3);
        for (int e = 0; e < edits; ++e) {
            const uint32_t word = rnd(state) % 37, kind = rnd(state) % 4;
            uint32_t v = rnd(state);
            if (kind == 0) v &= 0xffu;
            else if (kind == 1) v = 1u << (v & 31u);
            else if (kind == 2) {
                const char *cc[] = { "DXT1", "DXT3", "DXT5", "ATI1", "ATI2", "BC4U", "BC5U", "DX10" };
                std::memcpy(&v, cc[v % 8], 4);
            }
            std::memcpy(file.data() + 4 * word, &v, 4);
        }
        kc_dds_info info;
        const int s = parse_exact(file, file.size(), &info);
        CHECK(s == KC_OK || s == KC_ERR_INVALID_ARG || s == KC_ERR_UNSUPPORTED);
        if (s == KC_OK) {
            CHECK(info.data_offset == 128 || info.data_offset == 148);
            CHECK(info.data_offset + info.data_bytes <= file.size() && info.levels >= 1 && info.width && info.height);
        }
    }
    std::puts("dds host check: ok");
    return 0;
}
