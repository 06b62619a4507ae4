// Lossless packed copies of long-lived chain inputs: when a plane is packed, and its shadow's lifetime.
//
// The headline graph reads its two embedded sources again at every evaluation: 24 of the 36 bytes per pixel the launch moves,
// and the launch runs at the rate of a bare stream.  The sources do not change while they are embedded and their values are
// quantised (chain_pack.h), so a copy that holds the same values in 3 bytes or 1, made once, is all a later launch has to
// read.  The f32 plane stays: everything but the compiled flat chain kernels reads it as before.
//
// Which planes: MEM, owned, not a view, dense (pitch == 4 * w, or one row), whole float4 (w % 4 == 0).  Caller-owned planes
// (kc_plane_wrap) never: their owner may write them.
// When (pack_sources = 1): the plane is input of a plain flat chain launch that chain_cache_policy does not leave alone
// (n * stream_bytes + out_bytes > budget: HBM-bound), somebody besides the chain holds it (refs >= 2: it will be read again),
// and this is the second such sighting -- a one-shot evaluation never pays -- for EVERY such plane of the launch: a launch that
// reads a fresh image each time beside a constant source (the u8 pipe's route) stays as it is.  Then the pass runs for the slot's channel planes
// in both tiers, the stream is synchronised once, and the flags decide: U8 if every channel round-trips, else FIX24 if every
// channel does, else the slot stays f32 and its planes are not tried again.  pack_sources = 2 drops the size and sighting
// conditions (tests), 0 switches everything off.  pack_budget_mb caps what the shadows hold; past it nothing more is packed.
// Who writes into an existing owned plane: nobody inside the library -- u8 pipe uploads, communicator receives, band gathers
// and device imports all fill planes they have just created, before any chain reads them -- and two entry points of the C
// API: kc_plane_upload_f32 (drops the shadow; the plane may be packed again) and kc_plane_device_ptr (drops it for good: the
// pointer is the caller's to write through from then on).
#include "kc_runtime.hpp"

namespace kc {

uint32_t pack_bytes_per_quad(uint32_t tier) { return tier == (uint32_t)KC_PACK_FIX24 ? 12u : tier == (uint32_t)KC_PACK_U8 ? 4u : 16u; }

void plane_shadow_drop(kc_plane *p, bool never_again)
{
    if (p->shadow) {
        Context &c = ctx();
        pool_free(p->shadow, p->shadow_bytes);
        c.shadow_bytes -= p->shadow_bytes;
        c.counters["packed_bytes"] = c.shadow_bytes;
        p->shadow = nullptr;
        p->shadow_bytes = 0;
    }
    p->pack_tier = KC_PACK_NONE;
    p->pack_seen = 0;
    p->pack_state = never_again ? kc_plane::PACK_NEVER : kc_plane::PACK_UNTRIED;
}

static bool plane_packable(const kc_plane *p, uint32_t w, uint32_t h)
{
    return p && p->kind == kc_plane::MEM && p->owned && !p->view_of && p->dptr && p->w == w && p->h == h && w % 4 == 0 &&
           (p->pitch == (size_t)w * 4 || h == 1) && p->pack_state != kc_plane::PACK_NEVER;
}

static size_t shadow_block(uint64_t quads, uint32_t tier) { return (size_t)((quads * pack_bytes_per_quad(tier) + 255) / 256 * 256); }

// The pass for the planes of one input slot that have no shadow yet (n <= KC_CHAIN_MAX_BATCH, distinct): both tiers, one
// synchronisation.  Afterwards every plane is PACKED in the slot's tier, or PACK_NEVER.
static void pack_slot(kc_plane *const *planes, int n)
{
    Context &c = ctx();
    const uint64_t quads = (uint64_t)planes[0]->w * planes[0]->h / 4;
    const uint64_t budget = (uint64_t)c.pack_budget_mb << 20;
    if (c.shadow_bytes + (uint64_t)n * shadow_block(quads, KC_PACK_U8) > budget) return;  // (asked again at the next launch: it costs nothing)
    static const uint32_t kTiers[2] = { KC_PACK_U8, KC_PACK_FIX24 };  // in the order they are preferred
    void *blk[KC_CHAIN_MAX_BATCH][2] = {};
    PoolStaging flags;
    uint32_t host[KC_CHAIN_MAX_BATCH][2];
    bool ok = flags.alloc(sizeof host) == KC_OK && hipMemsetAsync(flags.ptr, 0, sizeof host, c.stream) == hipSuccess;
    for (int i = 0; i < n && ok; ++i)
        for (int t = 0; t < 2 && ok; ++t) {
            ok = pool_alloc(shadow_block(quads, kTiers[t]), &blk[i][t]) == KC_OK &&
                 launch_pack_plane(kTiers[t], planes[i]->dptr, blk[i][t], quads, (uint32_t *)flags.ptr + 2 * i + t, c.stream) == hipSuccess;
        }
    ok = ok && hipMemcpyAsync(host, flags.ptr, sizeof host, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = hipStreamSynchronize(c.stream) == hipSuccess && ok;
    c.counters["pack_passes"] += 2 * (uint64_t)n;  // (not in Context::launches: a recording counts the chain launches of its walk by it)
    c.alg_bytes += (uint64_t)n * quads * (16 + 4 + 16 + 12);
    int keep = -1;
    for (int t = 0; t < 2 && ok && keep < 0; ++t) {
        bool all = true;
        for (int i = 0; i < n; ++i) all = all && host[i][t] == 0;
        if (all) keep = t;
    }
    if (!ok) (void)hipGetLastError();
    if (ok && keep < 0) c.counters["pack_rejected"] += (uint64_t)n;
    if (keep >= 0 && c.shadow_bytes + (uint64_t)n * shadow_block(quads, kTiers[keep]) > budget) keep = -1;
    for (int i = 0; i < n; ++i) {
        for (int t = 0; t < 2; ++t)
            if (blk[i][t] && t != keep) pool_free(blk[i][t], shadow_block(quads, kTiers[t]));
        kc_plane *p = planes[i];
        if (keep < 0) {
            p->pack_state = kc_plane::PACK_NEVER;
            continue;
        }
        p->shadow = blk[i][keep];
        p->shadow_bytes = shadow_block(quads, kTiers[keep]);
        p->pack_tier = (uint8_t)kTiers[keep];
        p->pack_state = kc_plane::PACKED;
        c.shadow_bytes += p->shadow_bytes;
        c.counters["packed_planes"]++;
    }
    c.counters["packed_bytes"] = c.shadow_bytes;
}

uint32_t pack_chain_inputs(const ChainProgram &P, int batch, kc_plane *const (*src)[KC_CHAIN_MAX_IN], const uint32_t *refs, uint32_t w, uint32_t h)
{
    Context &c = ctx();
    const int mode = c.pack_sources;
    if (!mode || !src || !refs || batch < 1 || batch > (int)KC_CHAIN_MAX_BATCH) return 0;
    const uint64_t px4 = 4ull * w * h * (uint64_t)batch;
    if (mode == 1 && (uint64_t)P.n_in * px4 + px4 <= ((uint64_t)c.opt.cache_budget_mb << 20)) return 0;
    // first every slot's planes that have no shadow yet, and whether their turn has come.  One plane still at its first sighting
    // keeps the whole launch f32 (pack_sources = 1): a launch that reads a new image every time beside a long-lived source -- the
    // u8 pipe's route -- is no repeat, and measured slower with only its constant source packed (profiles/chain_packed_sources_times.txt)
    struct Slot {
        kc_plane *todo[KC_CHAIN_MAX_BATCH];
        int n_todo = 0;
        bool ok = false;
    } slots[KC_CHAIN_MAX_IN];
    bool due = true;
    for (uint32_t k = 0; k < P.n_in; ++k) {
        Slot &sl = slots[k];
        if (refs[k] < 2) continue;  // nobody else holds it: never read again
        sl.ok = true;
        for (int b = 0; b < batch && sl.ok; ++b) {
            kc_plane *p = src[b][k];
            sl.ok = plane_packable(p, w, h) && (const float *)p->dptr == P.in[b][k];
            if (!sl.ok || p->pack_state == kc_plane::PACKED) continue;
            bool seen = false;
            for (int i = 0; i < sl.n_todo; ++i) seen = seen || sl.todo[i] == p;
            if (seen) continue;
            sl.todo[sl.n_todo++] = p;
            if (p->pack_seen < 255) ++p->pack_seen;
            if (mode == 1 && p->pack_seen < 2) due = false;
        }
    }
    if (!due) return 0;
    uint32_t tiers = 0;
    for (uint32_t k = 0; k < P.n_in; ++k) {
        Slot &sl = slots[k];
        if (!sl.ok) continue;
        if (sl.n_todo) pack_slot(sl.todo, sl.n_todo);
        uint32_t tier = src[0][k]->pack_state == kc_plane::PACKED ? src[0][k]->pack_tier : 0u;
        for (int b = 1; b < batch; ++b)
            if (src[b][k]->pack_state != kc_plane::PACKED || src[b][k]->pack_tier != tier) tier = 0;
        tiers |= tier << (2 * k);
    }
    return tiers;
}

}  // namespace kc
