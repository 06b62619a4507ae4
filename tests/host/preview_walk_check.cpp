// The walk of kc_image_previews on the CPU: every workgroup and thread of every pass of a sweep of image sizes, levels and rects,
// with the planner (pw_plan) and the index functions (preview_walk.h) the library and its kernel use.  Each thread does the loads
// and stores it would do on the device -- real reads and writes on planes, scratch and destination allocated at their exact
// sizes -- so an address sanitizer sees every address the device would form.  The reduction is done twice: lane by lane as the
// kernel does it (in lane, exchanges inside a wave, 16 floats behind a barrier) and on the tile as a whole; the value a thread holds
// must be the tile's value at the texel pw_out_texel names.  Checked besides: every byte inside a rect is
// written exactly once with the reference value (the level-by-level chain, quantised), every scratch texel of a footprint
// exactly once, and no other byte changes (sentinel fill).
// Built and run by tests/test_preview_walk_sanitized.py: clang++ -fsanitize=address,undefined -ffp-contract=off.  Exit status
// 0: clean.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "preview_walk.h"

using namespace kc;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (failures++ < 20) {                        \
                std::fprintf(stderr, "FAIL %s: ", #cond); \
                std::fprintf(stderr, __VA_ARGS__);        \
                std::fprintf(stderr, "\n");               \
            }                                             \
        }                                                 \
    } while (0)

static float box(float a, float b, float c, float d) { return ((a + b) + (c + d)) * 0.25f; }
static uint32_t quant(float v)  // streaming.h's quant_u8
{
    float x = v;
    if (x < 0.0f) x = 0.0f;
    if (x > 1.0f) x = 1.0f;
    x = x * 255.0f;
    if (!(x <= 255.0f)) x = 255.0f;
    return (uint32_t)x;
}
static uint32_t rng_state = 12345u;
static float rnd()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(rng_state >> 8) / 16777216.0f * 1.4f - 0.2f;
}

// A plane at its exact size: rows `pitch` floats apart, the last one ending with its last whole quad
struct Plane {
    float *p = nullptr;
    uint32_t w = 0, h = 0, pitch = 0;
    void alloc(uint32_t w_, uint32_t h_, uint32_t pitch_)
    {
        w = w_;
        h = h_;
        pitch = pitch_;
        const size_t floats = (size_t)(h - 1) * pitch + 4 * (((size_t)w + 3) / 4);
        p = (float *)std::malloc(floats * sizeof(float));
        for (size_t i = 0; i < floats; ++i) p[i] = -7.0f;  // what a row's tail and the padding hold never reaches a texel
    }
    void release() { std::free(p); p = nullptr; }
    float at(uint32_t x, uint32_t y) const { return p[(size_t)y * pitch + x]; }
};

// the chain of a plane, level by level, with the header's clamps (tests/mip_ref.py in C++)
static std::vector<Plane> chain_of(const Plane &src)
{
    std::vector<Plane> lv;
    Plane l0;
    l0.alloc(src.w, src.h, 4 * ((src.w + 3) / 4));
    for (uint32_t y = 0; y < src.h; ++y)
        for (uint32_t x = 0; x < src.w; ++x) l0.p[(size_t)y * l0.pitch + x] = src.at(x, y);
    lv.push_back(l0);
    while (lv.back().w > 1 || lv.back().h > 1) {
        const Plane &s = lv.back();
        Plane d;
        d.alloc(s.w > 1 ? s.w >> 1 : 1, s.h > 1 ? s.h >> 1 : 1, 4 * (((s.w > 1 ? s.w >> 1 : 1) + 3) / 4));
        for (uint32_t y = 0; y < d.h; ++y)
            for (uint32_t x = 0; x < d.w; ++x) {
                const uint32_t x0 = 2 * x, x1 = 2 * x + 1 < s.w ? 2 * x + 1 : s.w - 1, y0 = 2 * y, y1 = 2 * y + 1 < s.h ? 2 * y + 1 : s.h - 1;
                d.p[(size_t)y * d.pitch + x] = box(s.at(x0, y0), s.at(x1, y0), s.at(x0, y1), s.at(x1, y1));
            }
        lv.push_back(d);
    }
    return lv;
}

struct ImageCfg {
    uint32_t n_ch, n_planes;
    uint8_t slot_of[4];
    float cval[4];
};
static const ImageCfg kGray = { 1, 1, { 0, PW_CONST, PW_CONST, PW_CONST }, { 0, 0, 0, 0 } };
static const ImageCfg kRgbConstAlpha = { 4, 3, { 0, 1, 2, PW_CONST }, { 0, 0, 0, 0.75f } };
static const ImageCfg kAlias = { 4, 1, { 0, 0, 0, PW_CONST }, { 0, 0, 0, 1.0f } };
static const ImageCfg kRgba = { 4, 4, { 0, 1, 2, 3 }, { 0, 0, 0, 0 } };
static const ImageCfg kConst = { 4, 0, { PW_CONST, PW_CONST, PW_CONST, PW_CONST }, { 0.25f, 3e38f, 1e-45f, 0.75f } };

struct Rect { uint32_t x, y, w, h; };

static uint32_t pack(const ImageCfg &I, const float v[4], const float cv[4])
{
    float ch[4];
    PreviewJob m{};
    m.slot_map = pw_slot_map(I.slot_of);
    for (uint32_t c = 0; c < 4; ++c) ch[c] = pw_slot_of(m, c) == PW_CONST ? cv[c] : v[pw_slot_of(m, c)];
    const uint32_t r = quant(ch[0]);
    if (I.n_ch == 1) return r | r << 8 | r << 16 | 255u << 24;
    return r | quant(ch[1]) << 8 | quant(ch[2]) << 16 | quant(ch[3]) << 24;
}

// One destination of 4-byte elements with a per-element write count and a sentinel fill
struct Dest {
    uint32_t *p = nullptr;
    std::vector<uint8_t> writes;
    size_t elems = 0;
    void alloc(size_t n)
    {
        elems = n;
        p = (uint32_t *)std::malloc(n * 4);
        std::memset(p, 0xA5, n * 4);
        writes.assign(n, 0);
    }
    void store(size_t off, uint32_t v)
    {
        p[off] = v;  // the sanitizer checks the address
        if (off < elems && writes[off] < 255) ++writes[off];
    }
    void release() { std::free(p); p = nullptr; }
};

static uint32_t as_bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// preview.hip's reduction by lane (mip_steps.h's mip_tile_reduce and mip_tile_tail, written out here a second time on purpose: the
// host's oracle does not share the device's header), all 256 threads of a workgroup in lockstep: raw[t] =
// the 4 x 4 texels thread t loaded; out[t][e] = the level-n values thread t holds afterwards, where pw_out_texel says it holds
// one.  A wave is 64 consecutive threads; an exchange with mask m reads lane ^ m of the same wave.
static void lanes_reduce(const float (*raw)[4][4], uint32_t n, float (*out)[4])
{
    static float v1[256][2][2], a[256], hs[256], l4[16];
    auto other = [](uint32_t t, uint32_t m) { return (t & ~63u) | ((t & 63u) ^ m); };
    for (uint32_t t = 0; t < 256; ++t) {
        for (int r = 0; r < 2; ++r) {
            v1[t][r][0] = box(raw[t][2 * r][0], raw[t][2 * r][1], raw[t][2 * r + 1][0], raw[t][2 * r + 1][1]);
            v1[t][r][1] = box(raw[t][2 * r][2], raw[t][2 * r][3], raw[t][2 * r + 1][2], raw[t][2 * r + 1][3]);
        }
        out[t][0] = v1[t][0][0];
        out[t][1] = v1[t][0][1];
        out[t][2] = v1[t][1][0];
        out[t][3] = v1[t][1][1];
    }
    if (n == 1) return;
    for (uint32_t t = 0; t < 256; ++t) out[t][0] = a[t] = box(v1[t][0][0], v1[t][0][1], v1[t][1][0], v1[t][1][1]);
    if (n == 2) return;
    for (uint32_t step = 0; step < 2; ++step) {  // levels 3 and 4: lanes ^ 1, ^ 16, then ^ 2, ^ 32
        const uint32_t mx = 1u << step, my = 16u << step;
        for (uint32_t t = 0; t < 256; ++t) hs[t] = a[t] + a[other(t, mx)];
        for (uint32_t t = 0; t < 256; ++t) out[t][0] = (hs[t] + hs[other(t, my)]) * 0.25f;
        for (uint32_t t = 0; t < 256; ++t) a[t] = out[t][0];
        if (n == 3 + step) return;
    }
    for (uint32_t t = 0; t < 256; ++t) {
        const uint32_t tx = t & 15u, ty = t >> 4;
        if (!(tx & 3u) && !(ty & 3u)) l4[(ty >> 2) * 4u + (tx >> 2)] = a[t];
    }
    float v5[4];
    for (uint32_t k = 0; k < 4; ++k) {
        const float *q = l4 + 8 * (k >> 1) + 2 * (k & 1);
        v5[k] = box(q[0], q[1], q[4], q[5]);
        if (n == 5) out[k][0] = v5[k];  // threads 0 .. 3
    }
    if (n == 6) out[0][0] = box(v5[0], v5[1], v5[2], v5[3]);  // thread 0
}

// All rects of one level of one image as one batch: the jobs of each pass share a launch and a prefix table
static void run_batch(uint32_t w, uint32_t h, const ImageCfg &I, uint32_t pad, uint32_t level, const std::vector<Rect> &rects, uint32_t dst_extra)
{
    std::vector<Plane> src(I.n_planes);
    std::vector<std::vector<Plane>> chain(I.n_planes);
    for (uint32_t s = 0; s < I.n_planes; ++s) {
        src[s].alloc(w, h, 4 * ((w + 3) / 4) + pad);
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) src[s].p[(size_t)y * src[s].pitch + x] = rnd();
        chain[s] = chain_of(src[s]);
    }
    float cv[4];
    for (int c = 0; c < 4; ++c) {
        cv[c] = I.cval[c];
        for (uint32_t k = 0; k < level; ++k) cv[c] = box(cv[c], cv[c], cv[c], cv[c]);
    }
    const size_t R = rects.size();
    std::vector<PwPlan> plan(R);
    uint32_t passes = 0;
    for (size_t i = 0; i < R; ++i) {
        const int s = pw_plan(w, h, level, rects[i].x, rects[i].y, rects[i].w, rects[i].h, &plan[i]);
        CHECK(s == 0, "pw_plan %ux%u level %u rect %u %u %u %u -> %d", w, h, level, rects[i].x, rects[i].y, rects[i].w, rects[i].h, s);
        if (s != 0) return;
        // an image without resident planes: one level-0 pass from the folded constants, as the library plans it
        if (I.n_planes == 0) CHECK(pw_plan_constant(rects[i].x, rects[i].y, rects[i].w, rects[i].h, &plan[i]), "pw_plan_constant");
        if (plan[i].passes > passes) passes = plan[i].passes;
    }
    // destinations and scratch, exact sizes
    std::vector<Dest> dst(R);
    std::vector<uint64_t> dst_pitch(R);
    std::vector<std::vector<std::vector<Dest>>> scratch(R);  // [request][pass][slot]
    for (size_t i = 0; i < R; ++i) {
        dst_pitch[i] = rects[i].w + dst_extra;
        dst[i].alloc((size_t)(rects[i].h - 1) * dst_pitch[i] + rects[i].w);
        scratch[i].resize(plan[i].passes);
        for (uint32_t p = 0; p + 1 < plan[i].passes; ++p) {
            const PwPass &G = plan[i].pass[p];
            scratch[i][p].resize(I.n_planes);
            for (uint32_t s = 0; s < I.n_planes; ++s) scratch[i][p][s].alloc((size_t)(G.rh - 1) * G.scratch_pitch + 4 * (((size_t)G.rw + 3) / 4));
        }
    }
    for (uint32_t p = 0; p < passes; ++p) {
        std::vector<PreviewJob> jobs;
        std::vector<uint32_t> prefix, owner;
        uint32_t wgs = 0;
        for (size_t i = 0; i < R; ++i) {
            if (plan[i].passes <= p) continue;
            const PwPass &G = plan[i].pass[p];
            const bool last = p + 1 == plan[i].passes;
            PreviewJob J{};
            pw_job_geometry(G, last, &J);
            J.n_planes = I.n_planes;
            J.gray = I.n_ch == 1;
            for (uint32_t s = 0; s < I.n_planes; ++s) {
                if (p == 0) {
                    // the fallback reads levels[level] of the chain, as the library does after kc_image_build_mips
                    const Plane &P0 = plan[i].fallback ? chain[s][level] : src[s];
                    J.src[s] = P0.p;
                    J.src_pitch[s] = P0.pitch;
                } else {
                    J.src[s] = (const float *)scratch[i][p - 1][s].p;
                    J.src_pitch[s] = plan[i].pass[p - 1].scratch_pitch;
                }
            }
            J.slot_map = pw_slot_map(I.slot_of);
            for (int c = 0; c < 4; ++c) J.cval[c] = cv[c];
            J.dst_pitch = last ? dst_pitch[i] : G.scratch_pitch;
            prefix.push_back(wgs);
            wgs += G.workgroups;
            jobs.push_back(J);
            owner.push_back((uint32_t)i);
        }
        prefix.push_back(wgs);
        static float tile[4][64][64], raw[4][256][4][4], lane[4][256][4];
        for (uint32_t wg = 0; wg < wgs; ++wg) {
            const uint32_t ji = pw_find_job(prefix.data(), (uint32_t)jobs.size(), wg);
            CHECK(ji < jobs.size() && prefix[ji] <= wg && wg < prefix[ji + 1], "job of workgroup %u", wg);
            const PreviewJob &J = jobs[ji];
            const uint32_t i = owner[ji], local = wg - prefix[ji], n = J.n;
            auto store = [&](size_t off, uint32_t e, const float v[4]) {
                (void)e;
                if (J.last) dst[i].store(off, pack(I, v, cv));
                else
                    for (uint32_t s = 0; s < J.n_planes; ++s) scratch[i][p][s].store(off, as_bits(v[s]));
            };
            if (n == 0) {
                CHECK(J.last, "a level-0 job that is not the last pass: the kernel stores RGBA8 there");
                for (uint32_t t = 0; t < 256; ++t) {
                    uint32_t X, Y, cnt;
                    if (!pw_n0_quad(J, local, t, &X, &Y, &cnt)) continue;
                    float v[4][4] = {};
                    for (uint32_t s = 0; s < J.n_planes; ++s) {
                        const float *q = J.src[s] + pw_n0_src_offset(J.src_pitch[s], X, Y);
                        const uint32_t take = pw_n0_wide(X) ? 4u : cnt;
                        for (uint32_t e = 0; e < take; ++e) v[s][e] = q[e];
                    }
                    size_t off;
                    if (!pw_dst_offset(J, X, Y, &off)) continue;
                    for (uint32_t e = 0; e < cnt; ++e) {
                        const float ve[4] = { v[0][e], v[1][e], v[2][e], v[3][e] };
                        store(off + e, e, ve);
                    }
                }
                continue;
            }
            uint32_t tX, tY;
            pw_tile(J, local, &tX, &tY);
            for (uint32_t s = 0; s < J.n_planes; ++s) {
                for (uint32_t t = 0; t < 256; ++t)
                    for (uint32_t r = 0; r < 4; ++r) {
                        const float *q = J.src[s] + pw_src_offset(J, J.src_pitch[s], tX, tY, t & 15u, t >> 4, r);
                        for (uint32_t e = 0; e < 4; ++e) tile[s][4 * (t >> 4) + r][4 * (t & 15u) + e] = raw[s][t][r][e] = q[e];
                    }
                lanes_reduce(raw[s], n, lane[s]);
                for (uint32_t k = 1, side = 32; k <= n; ++k, side >>= 1)
                    for (uint32_t y = 0; y < side; ++y)
                        for (uint32_t x = 0; x < side; ++x)
                            tile[s][y][x] = box(tile[s][2 * y][2 * x], tile[s][2 * y][2 * x + 1], tile[s][2 * y + 1][2 * x], tile[s][2 * y + 1][2 * x + 1]);
            }
            const uint32_t span = 64u >> n;
            for (uint32_t t = 0; t < 256; ++t)
                for (uint32_t e = 0; e < 4; ++e) {
                    uint32_t X, Y;
                    size_t off;
                    if (!pw_out_texel(n, tX, tY, t, e, &X, &Y)) continue;
                    CHECK(X / span == tX && Y / span == tY, "texel (%u, %u) of tile (%u, %u) at n = %u", X, Y, tX, tY, n);
                    if (!pw_dst_offset(J, X, Y, &off)) continue;
                    float v[4] = { 0, 0, 0, 0 };
                    for (uint32_t s = 0; s < J.n_planes; ++s) {
                        v[s] = lane[s][t][e];  // what the thread holds, against the tile's own reduction at the texel it names
                        CHECK(as_bits(v[s]) == as_bits(tile[s][Y % span][X % span]), "thread %u value %u at n = %u is not texel (%u, %u)", t, e, n, X, Y);
                    }
                    store(off, e, v);
                }
        }
    }
    // every texel of every rect once, with the reference value; nothing else touched
    for (size_t i = 0; i < R; ++i) {
        const Rect &rc = rects[i];
        for (uint32_t y = 0; y < rc.h; ++y)
            for (uint32_t x = 0; x < dst_pitch[i] && (size_t)y * dst_pitch[i] + x < dst[i].elems; ++x) {
                const size_t off = (size_t)y * dst_pitch[i] + x;
                if (x < rc.w) {
                    float v[4] = { 0, 0, 0, 0 };
                    for (uint32_t s = 0; s < I.n_planes; ++s) v[s] = chain[s][level].at(rc.x + x, rc.y + y);
                    const uint32_t want = pack(I, v, cv);
                    CHECK(dst[i].writes[off] == 1, "%ux%u level %u rect (%u %u %u %u): texel (%u, %u) written %u times", w, h, level, rc.x, rc.y, rc.w, rc.h, x,
                          y, dst[i].writes[off]);
                    CHECK(dst[i].p[off] == want, "%ux%u level %u rect (%u %u %u %u): texel (%u, %u) is %08x, reference %08x", w, h, level, rc.x, rc.y, rc.w,
                          rc.h, x, y, dst[i].p[off], want);
                } else {
                    CHECK(dst[i].writes[off] == 0 && dst[i].p[off] == 0xA5A5A5A5u, "%ux%u level %u: a byte between the rows changed", w, h, level);
                }
            }
        for (uint32_t p = 0; p + 1 < plan[i].passes; ++p) {
            const PwPass &G = plan[i].pass[p];
            for (uint32_t s = 0; s < I.n_planes; ++s) {
                const Dest &D = scratch[i][p][s];
                for (size_t off = 0; off < D.elems; ++off) {
                    const bool inside = off % G.scratch_pitch < G.rw;
                    CHECK(D.writes[off] == (inside ? 1 : 0), "%ux%u level %u pass %u: scratch element %zu written %u times", w, h, level, p, off, D.writes[off]);
                }
            }
        }
        dst[i].release();
        for (auto &ps : scratch[i])
            for (Dest &D : ps) D.release();
    }
    for (uint32_t s = 0; s < I.n_planes; ++s) {
        src[s].release();
        for (Plane &P : chain[s]) P.release();
    }
}

static std::vector<Rect> rects_of(uint32_t lw, uint32_t lh)
{
    std::vector<Rect> r;
    r.push_back({ 0, 0, lw, lh });
    const uint32_t widths[] = { 1, 2, 3, 5 };
    for (uint32_t x = 0; x < 4; ++x)        // every x % 4, an odd y
        for (uint32_t wd : widths)
            if ((uint64_t)x + wd <= lw && lh >= 2) r.push_back({ x, 1, wd, lh - 1 < 3 ? lh - 1 : 3 });
    for (uint32_t wd : widths)              // ends on the level's last column and row
        if (wd <= lw) r.push_back({ lw - wd, lh - (lh < 3 ? lh : 3), wd, lh < 3 ? lh : 3 });
    if (lw > 70 && lh > 40) r.push_back({ 61, 33, lw - 66, lh - 38 });  // several tiles, off the origin
    if (lw > 9 && lh > 4) r.push_back({ 5, 3, lw - 7, 1 });
    return r;
}

int main()
{
    // the job search on a table with empty entries
    {
        const uint32_t prefix[] = { 0, 3, 3, 4, 10 };
        const uint32_t want[] = { 0, 0, 0, 2, 3, 3, 3, 3, 3, 3 };
        for (uint32_t wg = 0; wg < 10; ++wg) CHECK(pw_find_job(prefix, 4, wg) == want[wg], "pw_find_job(%u)", wg);
    }
    struct Size { uint32_t w, h; };
    const Size sizes[] = { { 1, 1 }, { 1, 5 }, { 5, 1 }, { 2, 2 }, { 3, 7 }, { 64, 2 }, { 64, 64 }, { 65, 63 }, { 130, 70 }, { 67, 131 },
                           { 256, 256 }, { 300, 260 }, { 1024, 512 }, { 8192, 128 } };
    unsigned batches = 0;
    for (const Size &sz : sizes) {
        const bool small = (uint64_t)sz.w * sz.h <= 100000;
        uint32_t L = 1 + pw_floor_log2(sz.w > sz.h ? sz.w : sz.h);
        for (uint32_t level = 0; level < L && level <= 8; ++level) {
            const std::vector<Rect> rects = rects_of(pw_level_extent(sz.w, level), pw_level_extent(sz.h, level));
            run_batch(sz.w, sz.h, kGray, (level & 1) * 4, level, rects, (level % 3) * 2);
            ++batches;
            if (small) {
                run_batch(sz.w, sz.h, level & 1 ? kRgbConstAlpha : kRgba, 4, level, rects, 0);
                run_batch(sz.w, sz.h, kAlias, 0, level, rects, 1);
                run_batch(sz.w, sz.h, kConst, 0, level, rects, 2);
                batches += 3;
            }
        }
    }
    std::printf("preview_walk_check: %u batches, %d failures\n", batches, failures);
    return failures ? 1 : 0;
}
