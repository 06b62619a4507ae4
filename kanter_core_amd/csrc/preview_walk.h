// Previews (kc_image_previews, preview.cpp / preview.hip): every piece of index arithmetic of the planner and of preview_kernel,
// as plain inline functions that compile for the host as well.  The kernel calls these and does not restate them, so
// tests/host/preview_walk_check.cpp walks every workgroup and thread of every pass on the CPU, under an address sanitizer, with
// the addresses the device would form.
// Two rules hold throughout:
//   1. A destination offset is derived from the OUTPUT texel.  A thread computes its texel (X, Y) in coordinates of the level it
//      stores, tests rx <= X < rx + rw (and y likewise) and only then forms X - rx (pw_dst_offset).
//   2. No subtraction whose result may be negative is done in unsigned arithmetic; where one is formed, the line says why it
//      cannot be.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PW_HD __host__ __device__
#else
#define PW_HD
#endif

namespace kc {

constexpr uint32_t PW_MAX_PASSES = 6;   // ceil(31 / 6): a 32-bit extent halves at most 31 times
constexpr uint32_t PW_CONST = 0xffu;    // a slot of PreviewJob::slot_map: the channel is a constant

// One request in one pass.  n >= 1: the workgroups are the 64 x 64 source tiles (tx0 + i, ty0 + j), i < tnx, that touch the rect's
// footprint; each reduces its tile n levels and stores the level-n texels inside the rect.  n == 0: a thread owns four texels of a
// rect row, tnx = the quads per rect row.  The rect is in texels of level n of the source.
struct PreviewJob {
    const float *src[4];    // the distinct resident planes ("slots")
    void *dst[4];           // last: dst[0] = the rect's RGBA8 rows; otherwise one f32 scratch plane per slot, the rect at its origin
    uint64_t dst_pitch;     // 4-byte elements between rows of the destination (dwords of RGBA8 / floats)
    uint32_t src_pitch[4];  // floats
    float cval[4];          // last: the constant channels' values at the stored level
    uint32_t slot_map;      // last: channel c's slot in bits 8 c .. 8 c + 7, PW_CONST for a constant (pw_slot_of)
    uint32_t n_planes, gray, last;
    uint32_t sw, sh, n;
    uint32_t rx, ry, rw, rh;
    uint32_t tx0, ty0, tnx;
};

// The geometry of one pass of one request, and the plan of a request: what kc_preview_plan reports and the entry points run
struct PwPass {
    uint32_t sw, sh, n;                // the source this pass reads and the levels it reduces
    uint32_t rx, ry, rw, rh;           // the rect it stores, in texels of level n of that source
    uint32_t tx0, ty0, tnx, tny;       // n >= 1: the tiles; n == 0: tnx = quads per rect row, tny = rh
    uint32_t workgroups;
    uint32_t scratch_pitch;            // floats between the rows of the scratch this pass writes (0: the last pass)
};
struct PwPlan {
    uint32_t passes, fallback;
    uint32_t level_w, level_h;         // the extent of the requested level
    PwPass pass[PW_MAX_PASSES];
};

PW_HD inline uint32_t pw_slot_of(const PreviewJob &j, uint32_t ch) { return (j.slot_map >> (8u * ch)) & 0xffu; }  // ch < 4
PW_HD inline uint32_t pw_slot_map(const uint8_t slot_of[4])
{
    return (uint32_t)slot_of[0] | (uint32_t)slot_of[1] << 8 | (uint32_t)slot_of[2] << 16 | (uint32_t)slot_of[3] << 24;
}
PW_HD inline uint32_t pw_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
PW_HD inline uint32_t pw_floor_log2(uint32_t v)  // v > 0
{
    uint32_t k = 0;
    while (v >> (k + 1u)) ++k;  // ends: v >> 32 is never formed, k + 1 <= 31
    return k;
}
PW_HD inline uint32_t pw_level_extent(uint32_t v, uint32_t k) { return k < 32u && (v >> k) ? v >> k : 1u; }

// The workgroups of a pass; false when they (or a thread index) leave 32 bits
PW_HD inline bool pw_pass_finish(PwPass *p)
{
    uint64_t wgs;
    if (p->n == 0u) {
        p->tx0 = 0u;
        p->ty0 = 0u;
        p->tnx = (uint32_t)(((uint64_t)p->rw + 3u) / 4u);
        p->tny = p->rh;
        const uint64_t quads = (uint64_t)p->tnx * p->rh;
        if (quads > (1ull << 31)) return false;  // the thread's quad index is 32-bit
        wgs = (quads + 255u) / 256u;
    } else {
        const uint32_t span = 64u >> p->n;  // level-n texels per tile side, 1 <= n <= 6
        p->tx0 = p->rx / span;
        p->ty0 = p->ry / span;
        // rw, rh >= 1, so rx + rw - 1 >= rx: the last tile is not before the first
        const uint32_t tx1 = (uint32_t)(((uint64_t)p->rx + p->rw - 1u) / span), ty1 = (uint32_t)(((uint64_t)p->ry + p->rh - 1u) / span);
        p->tnx = tx1 - p->tx0 + 1u;
        p->tny = ty1 - p->ty0 + 1u;
        wgs = (uint64_t)p->tnx * p->tny;
        if (wgs > 0x7fffffffull) return false;
    }
    p->workgroups = (uint32_t)wgs;
    return true;
}

// The plan of texels [x, x + rw) x [y, y + rh) of level `level` of a w x h image.  0: planned; 1: a zero size, a level at or above
// the level count, an empty rect or one that leaves the level; 2: too many workgroups for one launch.
PW_HD inline int pw_plan(uint32_t w, uint32_t h, uint32_t level, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh, PwPlan *out)
{
    if (w == 0u || h == 0u || rw == 0u || rh == 0u) return 1;
    const uint32_t L = 1u + pw_floor_log2(w > h ? w : h), H = pw_floor_log2(w < h ? w : h);
    if (level >= L) return 1;
    const uint32_t lw = pw_level_extent(w, level), lh = pw_level_extent(h, level);
    if ((uint64_t)x + rw > lw || (uint64_t)y + rh > lh) return 1;
    PwPlan P{};
    P.level_w = lw;
    P.level_h = lh;
    if (level > H) {  // one extent has reached 1: the chain is built and the request runs at relative level 0 on levels[level]
        P.fallback = 1u;
        P.passes = 1u;
        PwPass &p = P.pass[0];
        p.sw = lw;
        p.sh = lh;
        p.n = 0u;
        p.rx = x;
        p.ry = y;
        p.rw = rw;
        p.rh = rh;
        if (!pw_pass_finish(&p)) return 2;
        *out = P;
        return 0;
    }
    uint32_t sw = w, sh = h, left = level, px = x, py = y;
    for (;;) {
        PwPass &p = P.pass[P.passes++];
        p.sw = sw;
        p.sh = sh;
        if (left > 6u) {
            // the footprint of the rect at level 6 of this source: the rect scaled by 2^(left - 6).  It lies inside that level
            // (px + rw <= sw >> left), so the shifts stay below 2^32
            const uint32_t up = left - 6u;  // left > 6
            p.n = 6u;
            p.rx = px << up;
            p.ry = py << up;
            p.rw = rw << up;
            p.rh = rh << up;
            p.scratch_pitch = (uint32_t)((((uint64_t)p.rw + 63u) / 64u) * 64u);
            if (!pw_pass_finish(&p)) return 2;
            // the next pass reads the scratch as an image of its own, the rect at its origin
            sw = p.rw;
            sh = p.rh;
            px = 0u;
            py = 0u;
            left = up;
        } else {
            p.n = left;
            p.rx = px;
            p.ry = py;
            p.rw = rw;
            p.rh = rh;
            if (!pw_pass_finish(&p)) return 2;
            break;
        }
    }
    *out = P;
    return 0;
}

// The plan of a rect of an image without resident planes (all channels constant): one level-0 pass that reads nothing and fills
// the rect from the job's constants, whatever the level.  The rect has passed pw_plan.  false: too many workgroups for one launch.
PW_HD inline bool pw_plan_constant(uint32_t x, uint32_t y, uint32_t rw, uint32_t rh, PwPlan *plan)
{
    PwPlan Q{};
    Q.passes = 1u;
    Q.level_w = plan->level_w;
    Q.level_h = plan->level_h;
    PwPass &p = Q.pass[0];
    p.sw = plan->level_w;
    p.sh = plan->level_h;
    p.n = 0u;
    p.rx = x;
    p.ry = y;
    p.rw = rw;
    p.rh = rh;
    if (!pw_pass_finish(&p)) return false;
    *plan = Q;
    return true;
}

// The geometry of a pass into a job; the caller fills the pointers, pitches, channel map and constants
PW_HD inline void pw_job_geometry(const PwPass &p, bool last, PreviewJob *j)
{
    j->last = last ? 1u : 0u;
    j->sw = p.sw;
    j->sh = p.sh;
    j->n = p.n;
    j->rx = p.rx;
    j->ry = p.ry;
    j->rw = p.rw;
    j->rh = p.rh;
    j->tx0 = p.tx0;
    j->ty0 = p.ty0;
    j->tnx = p.tnx;
}

// ---- the walk of a launch ----
// prefix[j] = the first workgroup of job j, prefix[count] = the grid: the job of workgroup wg < prefix[count], count >= 1
PW_HD inline uint32_t pw_find_job(const uint32_t *prefix, uint32_t count, uint32_t wg)
{
    uint32_t lo = 0u, hi = count;  // prefix[lo] <= wg < prefix[hi]
    while (hi - lo > 1u) {         // hi > lo throughout
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (prefix[mid] <= wg) lo = mid;
        else hi = mid;
    }
    return lo;
}

// n >= 1: the source tile of workgroup `local` (< tnx * tny) of the job
PW_HD inline void pw_tile(const PreviewJob &j, uint32_t local, uint32_t *tX, uint32_t *tY)
{
    const uint32_t row = local / j.tnx;
    *tX = j.tx0 + (local - row * j.tnx);  // row * tnx <= local
    *tY = j.ty0 + row;
}

// n >= 1: where thread (tx, ty) of the 16 x 16 workgroup on tile (tX, tY) loads the i-th of its four 16-byte rows, in floats from
// the plane's first: rows 4 ty .. 4 ty + 3 and columns 4 tx .. 4 tx + 3 of the tile, moved into the image where the tile leaves
// it -- whole quads up to 4 ceil(sw / 4) floats of a row and rows 0 .. sh - 1, nothing else (kc_plane_wrap)
PW_HD inline size_t pw_src_offset(const PreviewJob &j, uint32_t pitch, uint32_t tX, uint32_t tY, uint32_t tx, uint32_t ty, uint32_t i)
{
    const uint32_t q = pw_min(tX * 16u + tx, (uint32_t)(((uint64_t)j.sw + 3u) / 4u) - 1u);  // sw >= 1: at least one quad
    const uint32_t r = pw_min(tY * 64u + 4u * ty + i, j.sh - 1u);                            // sh >= 1
    return (size_t)r * pitch + 4u * (size_t)q;
}

// n >= 1: the e-th (0 .. 3) level-n texel that thread t of the workgroup on tile (tX, tY) holds after the reduction, in texels
// of that level; false: it holds none.  Level 1: a 2 x 2 patch per thread; level 2: one texel; levels 3 and 4: the lanes whose
// tx and ty are multiples of 2 and 4; level 5: threads 0 .. 3; level 6: thread 0.
PW_HD inline bool pw_out_texel(uint32_t n, uint32_t tX, uint32_t tY, uint32_t t, uint32_t e, uint32_t *X, uint32_t *Y)
{
    const uint32_t tx = t & 15u, ty = t >> 4;
    if (n == 1u) {
        *X = tX * 32u + 2u * tx + (e & 1u);
        *Y = tY * 32u + 2u * ty + (e >> 1);
        return e < 4u;
    }
    if (e != 0u) return false;
    if (n == 2u) {
        *X = tX * 16u + tx;
        *Y = tY * 16u + ty;
        return true;
    }
    if (n == 3u || n == 4u) {
        const uint32_t s = n - 2u, low = (1u << s) - 1u;  // n >= 3
        *X = tX * (64u >> n) + (tx >> s);
        *Y = tY * (64u >> n) + (ty >> s);
        return !((tx | ty) & low);
    }
    if (n == 5u) {
        *X = tX * 2u + (t & 1u);
        *Y = tY * 2u + ((t >> 1) & 1u);
        return t < 4u;
    }
    *X = tX;
    *Y = tY;
    return n == 6u && t == 0u;
}

// n == 0: the quad of thread t of workgroup `local`: texels (X .. X + cnt - 1, Y) of the source, 1 <= cnt <= 4; false: none
PW_HD inline bool pw_n0_quad(const PreviewJob &j, uint32_t local, uint32_t t, uint32_t *X, uint32_t *Y, uint32_t *cnt)
{
    const uint32_t idx = local * 256u + t, qpr = j.tnx;  // at most 2^31 quads (pw_pass_finish)
    if (idx >= qpr * j.rh) return false;
    const uint32_t row = idx / qpr, i = idx - row * qpr;  // row * qpr <= idx
    *X = j.rx + 4u * i;
    *Y = j.ry + row;
    *cnt = pw_min(4u, j.rw - 4u * i);  // i < qpr = ceil(rw / 4), so 4 i < rw
    return true;
}
// n == 0: texel (X, Y) of a plane in floats from its first, and whether the whole quad X .. X + 3 may be read with one 16-byte
// load: planes start 16-byte aligned with pitches that are multiples of 16 bytes, so the address is aligned exactly when X is a
// multiple of 4, and then the quad ends at or before 4 ceil(sw / 4)
PW_HD inline size_t pw_n0_src_offset(uint32_t pitch, uint32_t X, uint32_t Y) { return (size_t)Y * pitch + X; }
PW_HD inline bool pw_n0_wide(uint32_t X) { return (X & 3u) == 0u; }

// Where output texel (X, Y) goes, in 4-byte elements from the destination's first: false when it lies outside the rect.  The
// differences are formed after the comparisons that make them non-negative.
PW_HD inline bool pw_dst_offset(const PreviewJob &j, uint32_t X, uint32_t Y, size_t *off)
{
    if (X < j.rx || Y < j.ry) return false;
    const uint32_t dx = X - j.rx, dy = Y - j.ry;  // X >= rx, Y >= ry
    if (dx >= j.rw || dy >= j.rh) return false;
    *off = (size_t)dy * (size_t)j.dst_pitch + dx;
    return true;
}

// The source texels a job reads, per plane: what kc_stats_algorithmic_bytes counts 4 bytes each for
PW_HD inline uint64_t pw_texels_read(const PwPass &p)
{
    if (p.n == 0u) return (uint64_t)p.rw * p.rh;
    // the tiles clipped to the image; a tile that touches the rect starts inside the image
    const uint64_t x0 = (uint64_t)p.tx0 * 64u, x1 = ((uint64_t)p.tx0 + p.tnx) * 64u, y0 = (uint64_t)p.ty0 * 64u, y1 = ((uint64_t)p.ty0 + p.tny) * 64u;
    const uint64_t cx = (x1 < p.sw ? x1 : p.sw) - x0, cy = (y1 < p.sh ? y1 : p.sh) - y0;  // x0 < sw, y0 < sh
    return cx * cy;
}

}  // namespace kc
