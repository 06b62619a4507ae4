// Previews (include/kanter_core_amd.h): kc_preview_plan, kc_image_previews, kc_image_previews_device, kc_live_graph_buffer_previews.
// The host side plans every request with preview_walk.h's pw_plan (what kc_preview_plan reports), folds constant planes with
// mip.cpp's expression, gives the passes between two launches their f32 scratch, uploads the job tables of all passes with one
// copy from pinned memory and enqueues one launch of preview.hip's kernel per pass on the library's stream.
#include <algorithm>

#include "kc_runtime.hpp"

namespace kc {

static int pv_refuse(const char *who, const char *what)
{
    set_error(std::string(who) + ": " + what);
    return KC_ERR_INVALID_ARG;
}

int preview_plan(uint32_t w, uint32_t h, uint32_t level, uint32_t x, uint32_t y, uint32_t rect_w, uint32_t rect_h, kc_preview_plan_info *out)
{
    if (!out) return pv_refuse("kc_preview_plan", "NULL output");
    PwPlan P;
    const int s = pw_plan(w, h, level, x, y, rect_w, rect_h, &P);
    if (s == 1) return pv_refuse("kc_preview_plan", "a zero size, a level at or above the level count, an empty rect or one outside the level");
    if (s != 0) return pv_refuse("kc_preview_plan", "more workgroups than one launch holds");
    kc_preview_plan_info o{};
    o.passes = P.passes;
    o.fallback = P.fallback;
    o.level_width = P.level_w;
    o.level_height = P.level_h;
    for (uint32_t p = 0; p < P.passes; ++p) {
        o.levels[p] = P.pass[p].n;
        o.workgroups[p] = P.pass[p].workgroups;
        if (p + 1 < P.passes) {
            o.scratch_width[p] = P.pass[p].rw;
            o.scratch_height[p] = P.pass[p].rh;
            o.scratch_bytes[p] = (uint64_t)P.pass[p].scratch_pitch * P.pass[p].rh * sizeof(float);
        }
    }
    *out = o;
    return KC_OK;
}

// the last byte of request q, + 1; false when it leaves size_t
static bool pv_request_end(const kc_preview_request &q, size_t *end)
{
    const unsigned __int128 e = (unsigned __int128)q.offset_bytes + (unsigned __int128)(q.height - 1u) * q.row_pitch_bytes + (unsigned __int128)q.width * 4u;  // height >= 1
    if (e > (unsigned __int128)SIZE_MAX) return false;
    *end = (size_t)e;
    return true;
}

int preview_check(const kc_preview_request *r, uint32_t count, uint32_t flags, const void *out, size_t out_bytes, bool images_named, const char *who)
{
    if (flags & ~(uint32_t)KC_PREVIEW_SRGB) {
        set_error(std::string(who) + ": flags other than KC_PREVIEW_SRGB");
        return KC_ERR_UNSUPPORTED;
    }
    if (!r || !out) return pv_refuse(who, "NULL requests or output");
    if (count > 4096u) return pv_refuse(who, "more than 4096 requests");
    for (uint32_t i = 0; i < count; ++i) {
        const kc_preview_request &q = r[i];
        if (images_named && !q.image) return pv_refuse(who, "a request with a NULL image");
        if (q.width == 0 || q.height == 0) return pv_refuse(who, "an empty rect");
        if (q.offset_bytes % 4 || q.row_pitch_bytes % 4) return pv_refuse(who, "an offset or a row pitch that is not a multiple of 4");
        if (q.row_pitch_bytes < (size_t)q.width * 4) return pv_refuse(who, "a row pitch below 4 * width");
        size_t end = 0;
        if (!pv_request_end(q, &end) || end > out_bytes) return pv_refuse(who, "a request whose last byte lies past the buffer");
    }
    return KC_OK;
}

void preview_release()
{
    Context::PreviewBuffers &b = ctx().preview;
    if (b.copied) (void)hipEventDestroy(b.copied);
    if (b.host) (void)hipHostFree(b.host);
    b = Context::PreviewBuffers{};
}

namespace {
// What a request reads: the distinct resident planes of its (forced) image, the channel map, the constants at the stored level
struct PvSource {
    const float *src[4] = { nullptr, nullptr, nullptr, nullptr };
    uint32_t pitch[4] = { 0, 0, 0, 0 };
    uint8_t slot_of[4] = { PW_CONST, PW_CONST, PW_CONST, PW_CONST };
    float cval[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    uint32_t n_planes = 0, gray = 0;
};

void pv_source(const kc_image *img, uint32_t folds, PvSource &s)
{
    const kc_plane *seen[4] = { nullptr, nullptr, nullptr, nullptr };
    s.gray = img->is_rgba() ? 0u : 1u;
    for (int ch = 0; ch < img->n; ++ch) {
        const kc_plane *p = img->planes[ch];
        if (p->kind == kc_plane::CONST) {
            float c = p->cval;
            for (uint32_t k = 0; k < folds; ++k) c = mip_const_fold(c);  // once per level, as kc_image_build_mips folds it
            s.cval[ch] = c;
            continue;
        }
        uint32_t k = 0;
        while (k < s.n_planes && !(seen[k] == p || (seen[k]->dptr == p->dptr && seen[k]->pitch == p->pitch))) ++k;
        if (k == s.n_planes) {
            seen[k] = p;
            s.src[k] = p->dptr;
            s.pitch[k] = (uint32_t)(p->pitch / sizeof(float));
            ++s.n_planes;
        }
        s.slot_of[ch] = (uint8_t)k;
    }
}

struct PvHeld {  // the chains the fallback requests read, by image, until their launch has been enqueued
    std::vector<std::pair<const kc_image *, std::vector<kc_image *>>> chains;
    ~PvHeld()
    {
        for (auto &ch : chains)
            for (kc_image *i : ch.second) image_release(i);
    }
};
}  // namespace

// Every pass of the batch on the library's stream: request i stores its rect at dst[i], rows pitch[i] bytes apart (device memory).
// The requests have passed preview_check; the level and the rect are checked here, before anything is launched for the batch.
static int previews_enqueue(const kc_preview_request *r, kc_image *const *imgs, uint32_t count, bool srgb, uint8_t *const *dst, const size_t *pitch,
                            const char *who)
{
    Context &c = ctx();
    std::vector<PwPlan> plans(count);
    auto image_of = [&](uint32_t i) { return imgs ? imgs[i] : r[i].image; };
    for (uint32_t i = 0; i < count; ++i) {
        const kc_image *img = image_of(i);
        const int s = pw_plan(img->w(), img->h(), r[i].level, r[i].x, r[i].y, r[i].width, r[i].height, &plans[i]);
        if (s == 1) return pv_refuse(who, "a level at or above the level count, or a rect that reaches outside the level");
        if (s != 0) return pv_refuse(who, "a request of more workgroups than one launch holds");
    }
    for (uint32_t i = 0; i < count; ++i) KC_TRY(image_force(image_of(i)));  // pending chains and deferred resizes run first
    PvHeld held;
    uint64_t fallbacks = 0;  // counted once the batch has been launched
    std::vector<PvSource> source(count);
    for (uint32_t i = 0; i < count; ++i) {
        kc_image *img = image_of(i);
        PwPlan &P = plans[i];
        bool resident = false;
        for (int ch = 0; ch < img->n; ++ch) resident = resident || img->planes[ch]->kind != kc_plane::CONST;
        if (!resident) {  // nothing to read: the folded constants fill the rect in one level-0 pass, fallback or not
            if (!pw_plan_constant(r[i].x, r[i].y, r[i].width, r[i].height, &P)) return pv_refuse(who, "a request of more workgroups than one launch holds");
            pv_source(img, r[i].level, source[i]);
        } else if (P.fallback) {
            // one chain per distinct image of the batch, held until the launches have been enqueued
            size_t at = 0;
            while (at < held.chains.size() && held.chains[at].first != img) ++at;
            if (at == held.chains.size()) {
                uint32_t L = 0, made = 0;
                KC_TRY(mip_level_count(img->w(), img->h(), &L));
                std::vector<kc_image *> lv(L, nullptr);
                KC_TRY(image_build_mips(img, 0, lv.data(), L, &made));
                held.chains.emplace_back(img, std::move(lv));
            }
            ++fallbacks;
            pv_source(held.chains[at].second[r[i].level], 0, source[i]);  // the chain has folded its constants
        } else {
            pv_source(img, r[i].level, source[i]);
        }
    }
    uint32_t passes = 0;
    for (const PwPlan &P : plans) passes = std::max(passes, P.passes);
    // the scratch between the passes: one pool block, a 256-byte aligned plane per slot, request and pass
    std::vector<size_t> scratch_at((size_t)count * PW_MAX_PASSES, 0);
    size_t scratch_bytes = 0;
    for (uint32_t i = 0; i < count; ++i)
        for (uint32_t p = 0; p + 1 < plans[i].passes; ++p) {
            const size_t plane = ((size_t)plans[i].pass[p].scratch_pitch * plans[i].pass[p].rh * sizeof(float) + 255) / 256 * 256;
            scratch_at[(size_t)i * PW_MAX_PASSES + p] = scratch_bytes;
            scratch_bytes += plane * source[i].n_planes;
        }
    PoolStaging scratch;
    if (scratch_bytes) KC_TRY(scratch.alloc(scratch_bytes));
    auto scratch_plane = [&](uint32_t i, uint32_t p, uint32_t s) {
        const size_t plane = ((size_t)plans[i].pass[p].scratch_pitch * plans[i].pass[p].rh * sizeof(float) + 255) / 256 * 256;
        return (float *)((char *)scratch.ptr + scratch_at[(size_t)i * PW_MAX_PASSES + p] + plane * s);
    };
    // the tables of every pass, one after the other: count_p + 1 prefix words (padded to 16 bytes), then count_p jobs
    struct PassTable {
        size_t prefix_at = 0, jobs_at = 0;
        uint32_t count = 0, workgroups = 0, max_planes = 1;
        uint64_t in_bytes = 0, out_bytes = 0;
    };
    std::vector<PassTable> table(passes);
    size_t table_bytes = 0;
    for (uint32_t p = 0; p < passes; ++p) {
        PassTable &T = table[p];
        for (uint32_t i = 0; i < count; ++i) T.count += plans[i].passes > p;
        T.prefix_at = table_bytes;
        table_bytes += ((size_t)(T.count + 1) * sizeof(uint32_t) + 15) / 16 * 16;
        T.jobs_at = table_bytes;
        table_bytes += (size_t)T.count * sizeof(PreviewJob);
    }
    Context::PreviewBuffers &B = c.preview;
    if (!B.copied) KC_HIP(hipEventCreateWithFlags(&B.copied, hipEventDisableTiming));
    else KC_HIP(hipEventSynchronize(B.copied));  // the previous batch's upload has read the buffer
    if (B.bytes < table_bytes) {
        if (B.host) KC_HIP(hipHostFree(B.host));
        B.host = nullptr;
        B.bytes = 0;
        const size_t want = std::max(table_bytes, (size_t)64 << 10);
        KC_HIP(hipHostMalloc(&B.host, want, hipHostMallocDefault));
        B.bytes = want;
    }
    PoolStaging dev_table;
    KC_TRY(dev_table.alloc(table_bytes));
    std::memset(B.host, 0, table_bytes);
    for (uint32_t p = 0; p < passes; ++p) {
        PassTable &T = table[p];
        uint32_t *prefix = (uint32_t *)((char *)B.host + T.prefix_at);
        PreviewJob *jobs = (PreviewJob *)((char *)B.host + T.jobs_at);
        uint32_t k = 0;
        uint64_t wgs = 0;
        for (uint32_t i = 0; i < count; ++i) {
            const PwPlan &P = plans[i];
            if (P.passes <= p) continue;
            const PwPass &G = P.pass[p];
            const PvSource &S = source[i];
            const bool last = p + 1 == P.passes;
            PreviewJob &J = jobs[k];
            pw_job_geometry(G, last, &J);
            J.n_planes = S.n_planes;
            J.gray = S.gray;
            for (uint32_t s = 0; s < S.n_planes; ++s) {
                J.src[s] = p == 0 ? S.src[s] : scratch_plane(i, p - 1, s);
                J.src_pitch[s] = p == 0 ? S.pitch[s] : P.pass[p - 1].scratch_pitch;
                if (!last) J.dst[s] = scratch_plane(i, p, s);
            }
            J.slot_map = pw_slot_map(S.slot_of);
            for (int ch = 0; ch < 4; ++ch) J.cval[ch] = S.cval[ch];
            if (last) {
                J.dst[0] = dst[i];
                J.dst_pitch = pitch[i] / 4;
            } else {
                J.dst_pitch = G.scratch_pitch;
            }
            prefix[k++] = (uint32_t)wgs;
            wgs += G.workgroups;
            T.max_planes = std::max(T.max_planes, S.n_planes);
            T.in_bytes += 4 * pw_texels_read(G) * S.n_planes;
            T.out_bytes += 4 * (uint64_t)G.rw * G.rh * (last ? 1u : S.n_planes);
        }
        if (wgs > 0x7fffffffull) return pv_refuse(who, "a batch of more workgroups than one launch holds");
        prefix[k] = (uint32_t)wgs;
        T.workgroups = (uint32_t)wgs;
    }
    KC_HIP(hipMemcpyAsync(dev_table.ptr, B.host, table_bytes, hipMemcpyHostToDevice, c.stream));
    KC_HIP(hipEventRecord(B.copied, c.stream));
    for (uint32_t p = 0; p < passes; ++p) {
        const PassTable &T = table[p];
        const bool nt = (cache_policy_mask(T.in_bytes, T.out_bytes, T.max_planes) & 0xffu) != 0;
        hipError_t e = launch_preview((const PreviewJob *)((char *)dev_table.ptr + T.jobs_at), (const uint32_t *)((char *)dev_table.ptr + T.prefix_at),
                                      T.count, T.workgroups, srgb, nt, c.stream);
        if (e != hipSuccess) return hip_fail(e, "launch_preview");
        c.counters["preview_launches"]++;
        if (nt) c.counters["preview_nt"]++;
        c.launches++;
        c.alg_bytes += T.in_bytes + T.out_bytes;
    }
    c.counters["preview_fallback"] += fallbacks;
    // the scratch, the table and the fallback's levels go back to the pool here; the pool hands a block out again only to work
    // enqueued on the same stream
    return KC_OK;
}

int image_previews(const kc_preview_request *r, kc_image *const *imgs, uint32_t count, uint32_t flags, uint8_t *host, size_t host_bytes, const char *who)
{
    KC_TRY(preview_check(r, count, flags, host, host_bytes, imgs == nullptr, who));
    if (count == 0) return KC_OK;
    KC_TRY(need_init());
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    // the rects tightly packed in request order in a staging block; when the caller's layout is that packing, one copy lands
    // them, otherwise the rows are placed from a host copy, so that no byte between or outside the rects is written
    std::vector<size_t> at(count), tight_pitch(count);
    size_t total = 0;
    bool packed = true;
    for (uint32_t i = 0; i < count; ++i) {
        at[i] = total;
        tight_pitch[i] = (size_t)r[i].width * 4;
        packed = packed && r[i].row_pitch_bytes == tight_pitch[i] && r[i].offset_bytes == r[0].offset_bytes + total;
        total += tight_pitch[i] * r[i].height;
    }
    PoolStaging staging;
    KC_TRY(staging.alloc(total));
    std::vector<uint8_t *> dst(count);
    for (uint32_t i = 0; i < count; ++i) dst[i] = (uint8_t *)staging.ptr + at[i];
    KC_TRY(previews_enqueue(r, imgs, count, (flags & KC_PREVIEW_SRGB) != 0, dst.data(), tight_pitch.data(), who));
    std::vector<uint8_t> rows;
    if (!packed) rows.resize(total);
    hipError_t e = hipMemcpyAsync(packed ? host + r[0].offset_bytes : rows.data(), staging.ptr, total, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) return hip_fail(e, "image_previews");
    if (!packed)
        for (uint32_t i = 0; i < count; ++i)
            for (uint32_t y = 0; y < r[i].height; ++y)
                std::memcpy(host + r[i].offset_bytes + (size_t)y * r[i].row_pitch_bytes, rows.data() + at[i] + (size_t)y * tight_pitch[i], tight_pitch[i]);
    return KC_OK;
}

int image_previews_device(const kc_preview_request *r, uint32_t count, uint32_t flags, void *device_ptr, size_t bytes, void *hip_stream)
{
    const char *who = "kc_image_previews_device";
    KC_TRY(preview_check(r, count, flags, device_ptr, bytes, true, who));
    if ((uintptr_t)device_ptr % 4) return pv_refuse(who, "the pointer must be a multiple of 4");
    if (count == 0) return KC_OK;
    KC_TRY(need_init());  // an image exists only after kc_init: it is not looked at before
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    size_t extent = 0;
    std::vector<uint8_t *> dst(count);
    std::vector<size_t> pitch(count);
    for (uint32_t i = 0; i < count; ++i) {
        size_t end = 0;
        pv_request_end(r[i], &end);  // checked
        extent = std::max(extent, end);
        dst[i] = (uint8_t *)device_ptr + r[i].offset_bytes;
        pitch[i] = r[i].row_pitch_bytes;
    }
    KC_TRY(device_extent_check(device_ptr, extent, who));
    return with_stream_edges(hip_stream, [&] { return previews_enqueue(r, nullptr, count, (flags & KC_PREVIEW_SRGB) != 0, dst.data(), pitch.data(), who); });
}

}  // namespace kc
