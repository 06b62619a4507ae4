// Host runtime declarations: context, HBM plane pool, planes / images, node operators, graphs.
#pragma once

#include <cstring>
#include <deque>
#include <set>
#include <tuple>
#include <type_traits>
#include <unordered_map>
#include <unordered_set>

#include "kc_internal.hpp"

// ------------------------------------------------------------------------------------------
// Opaque C-ABI types
// ------------------------------------------------------------------------------------------
namespace kc {
struct Chain;
struct ChainLink;
}

// Fixed-size objects the evaluator creates and drops by the hundred per evaluation (a plane, a chain link and an
// image per node and channel) come from free lists: released together when a chain has run, they overflow
// malloc's small per-thread cache and took its locked fast-bin path -- a third of the host time of a 256 x 256
// evaluation (profiles/r02_host_samples.txt).  The lists are guarded by Context::mu, which every creator and
// releaser of these objects holds (see kc_plane::refs); a list keeps at most kMaxFree blocks.  Sanitizer builds
// use plain new / delete so that they still see every use after free.
namespace kc {
#if defined(__SANITIZE_ADDRESS__) || defined(__SANITIZE_THREAD__)
#define KC_NO_OBJECT_POOL 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer) || __has_feature(thread_sanitizer)
#define KC_NO_OBJECT_POOL 1
#endif
#endif
template <class T> struct Pooled {
#ifndef KC_NO_OBJECT_POOL
    struct FreeList {
        struct Block { Block *next; };
        static constexpr size_t kMaxFree = 1u << 14;
        Block *head = nullptr;
        size_t n = 0;
        bool closed = false;  // the process is exiting: objects released by later exit handlers go straight to the heap
        ~FreeList()
        {
            closed = true;
            while (head) {
                Block *b = head;
                head = b->next;
                ::operator delete(b);
            }
            n = 0;
        }
    };
    static FreeList &list()
    {
        static FreeList fl;
        return fl;
    }
    static void *operator new(size_t bytes)
    {
        FreeList &fl = list();
        if (bytes == sizeof(T) && fl.head) {
            typename FreeList::Block *b = fl.head;
            fl.head = b->next;
            --fl.n;
            return b;
        }
        return ::operator new(bytes < sizeof(typename FreeList::Block) ? sizeof(typename FreeList::Block) : bytes);
    }
    static void operator delete(void *q, size_t bytes)
    {
        FreeList &fl = list();
        if (bytes == sizeof(T) && fl.n < FreeList::kMaxFree && !fl.closed) {
            typename FreeList::Block *b = static_cast<typename FreeList::Block *>(q);
            b->next = fl.head;
            fl.head = b;
            ++fl.n;
            return;
        }
        ::operator delete(q);
    }
#endif
};
}  // namespace kc

// One channel.  MEM: pitched f32 in HBM.  CONST: broadcast scalar (what the reference holds as
// vec![v; n]).  LAZY: a pointwise Mix chain that has not been run yet; forcing it launches the
// fused chain kernel and turns the plane into MEM.  RESIZE: `rz_src` resampled to w x h with
// `rz_filter`, not run yet: a Mix chain that consumes it resamples inside its own kernel
// (resize_chain_kernel), anything else forces it through the plain resize kernel.
struct kc_plane : kc::Pooled<kc_plane> {
    enum Kind { MEM = 0, CONST = 1, LAZY = 2, RESIZE = 3 };
    // Reference counts are plain integers: every C-ABI entry that creates, retains or releases a plane or an
    // image holds Context::mu (c_api.cpp), as the evaluator always did -- an evaluation touches them some
    // thirty times per node, and the locked read-modify-writes were a quarter of its host time.
    int refs = 1;
    uint32_t w = 0, h = 0;
    Kind kind = MEM;
    float *dptr = nullptr;
    size_t pitch = 0;  // bytes
    size_t bytes = 0;  // pool block size (owned planes)
    bool owned = false;
    float cval = 0.0f;
    kc::ChainLink *link = nullptr;  // LAZY: the last step and what it continues (see ChainLink)
    kc::Chain *chain = nullptr;     // LAZY: the flattened program, built when the plane is forced
    kc_plane *view_of = nullptr;  // MEM, not owned: rows of this (retained) plane, see bands.cpp
    kc_plane *rz_src = nullptr;  // retained; MEM
    int rz_filter = 0;
    // The lossless packed copy a chain kernel reads instead of the plane (chain_pack.cpp): MEM, owned, dense planes only.
    // `shadow` is a pool block of shadow_bytes, released with the plane; pack_tier its KC_PACK_* code.  Whoever writes into the
    // plane in place or hands its pointer out calls plane_shadow_drop first.
    enum PackState : uint8_t { PACK_UNTRIED = 0, PACKED = 1, PACK_NEVER = 2 };  // PACK_NEVER: fits no tier, or is not to be tried again
    void *shadow = nullptr;
    size_t shadow_bytes = 0;
    uint8_t pack_tier = 0, pack_state = PACK_UNTRIED, pack_seen = 0;  // pack_seen: sightings by HBM-bound chain launches so far
};

// SlotImage, src/slot_image.rs:15-19
struct kc_image : kc::Pooled<kc_image> {
    int refs = 1;  // under Context::mu, like kc_plane::refs
    int n = 0;  // 1 = Gray, 4 = Rgba
    kc_plane *planes[4] = { nullptr, nullptr, nullptr, nullptr };
    bool is_rgba() const { return n == 4; }
    uint32_t w() const { return planes[0]->w; }
    uint32_t h() const { return planes[0]->h; }
};

namespace kc {

struct ChainStep {
    uint8_t code;       // ChainCode
    kc_plane *operand;  // retained; MEM or CONST -- or, in a link, LAZY: a second chain joined in (plane_mix); in a flat
                        // Chain that one is expanded and the combining step's operand is saved_value_marker()
    uint8_t level = 0;  // flat Chain only: which saved value a CH_SAVE_LOAD writes / a step on saved_value_marker() reads
};
kc_plane *saved_value_marker();

struct Chain : Pooled<Chain> {
    kc_plane *start = nullptr;  // retained; MEM, CONST or RESIZE
    std::vector<ChainStep> steps;
    std::vector<kc_plane *> joined;  // retained; the LAZY planes whose chains were expanded into `steps` (CH_SAVE_LOAD)
    ~Chain();
};

// A lazy plane is "the plane it continues, plus one step": extending a chain is O(1) and consumers of
// the same prefix share it (a 64-node linear graph used to copy 3 x 64 x 32 steps per evaluation).
// The flat Chain is built from the links when the plane is forced; a `prev` that has been forced in
// the meantime is resident and simply becomes the start.
struct ChainLink : Pooled<ChainLink> {
    kc_plane *prev = nullptr;   // retained; the LAZY plane continued, or nullptr
    kc_plane *start = nullptr;  // retained; the chain's first value when prev == nullptr
    ChainStep step{};           // operand retained
    uint32_t length = 1;        // RECORDS up to and including this step (an upper bound once a prev was forced): a step that
                                // chain_fill folds into its predecessor's record (CH_*_INV) does not count
    bool fused = false;         // this step is such a folded one
    uint8_t saved = 0;          // saved values the chain needs at once: 0 = no joined chain, 1 = joins of plain chains, ...
    int n_in = 0;               // distinct MEM / RESIZE planes the whole chain reads (same bound)
    // Their identities BY VALUE (device pointer + pitch of a resident plane, address of a deferred resize):
    // the planes themselves are kept alive by the links that use them, which may be gone once a prefix
    // has been forced, so these are never dereferenced.  A stale entry only makes the bound more cautious.
    struct InKey {
        const void *p = nullptr;
        size_t q = 0;
        bool operator==(const InKey &o) const { return p == o.p && q == o.q; }
    };
    InKey ins[KC_CHAIN_MAX_IN + 1];
    ~ChainLink();
};

struct TapsHost {
    std::vector<uint32_t> left, count;
    std::vector<float> w;
    uint32_t stride = 1;     // max taps of any output index
    uint32_t min_count = 1;  // min taps of any output index
    // Integer-ratio down-sampling: output indices [reg_a, reg_b) all have reg_ages * reg_ratio taps, windows reg_ratio
    // apart and bit-identical weights (resize_poly_kernel); reg_ratio == 0: no such range.
    uint32_t reg_a = 0, reg_b = 0, reg_ages = 0, reg_ratio = 0;
    // Integer-ratio up-sampling (upsample.h): the table has that structure (up_axis_build checks it bit for bit);
    // up_rows = the class rows, up.cls points at their copy in HBM once the table is uploaded.
    bool up_ok = false;
    UpAxis up{};
    std::vector<float> up_rows, up_qrows;  // class rows per output / per column quad (tap-major)
    // resize_down2_kernel (down2.hip; built by down2_build for down-sampling axes, d2_want):
    //   as the VERTICAL table   d2_vrec: d2_nc records of KC_DOWN2_REC dwords per group of four output rows (kc_internal.hpp);
    //                           d2_nc == 0: some group's windows span more than KC_DOWN2_MAX_CHUNKS x 16 source rows (wrapped
    //                           rows of a band table, very large ratios)
    //   as the HORIZONTAL table d2_hw: the weights with rows padded to d2_hstride (a multiple of 4, +0.0 beyond a column's own
    //                           taps); d2_tile_w: the strip width whose widest source window is 64 quads (0: none)
    std::vector<uint32_t> d2_vrec, d2_strips;  // d2_strips: (first source column & ~3, source quads) per strip of d2_tile_w columns
    std::vector<float> d2_hw;
    bool d2_want = false;  // a down-sampling axis with windows of at least 4 taps
    uint32_t d2_nc = 0, d2_hstride = 0, d2_tile_w = 0;
    uint32_t p2_tile_w = 0;  // as the HORIZONTAL table of resize_poly2_kernel: the strip width (<= 128) whose widest window is 64 quads
    const uint32_t *d2_vrec_dev = nullptr, *d2_strips_dev = nullptr;
    const float *d2_hw_dev = nullptr;
};

struct TapsEntry {
    uint64_t last_use = 0;  // band tables only: LRU clock (Context::band_taps_clock)
    TapsHost host;
    void *dev_block = nullptr;
    size_t dev_bytes = 0;
    TapsDev dev{};
};

// What chain_launch leaves behind while an evaluation is being recorded for replay (replay.cpp): one record per launch.
struct ReplayLaunch {
    ChainProgram prog;  // as launched: input and output pointers of the recorded run
    int batch = 0, mode = 0;
    uint32_t in_refs[KC_CHAIN_MAX_IN] = {};
    uint32_t w = 0, h = 0;
    kc_plane *planes[KC_CHAIN_MAX_BATCH] = { nullptr, nullptr, nullptr, nullptr };  // the lazy planes the launch made resident
    // the planes behind the inputs, by object: a recording made before a source was packed launches its packed form afterwards.
    // Only those of inputs with in_from < 0 are used in a replay: the recording's images keep exactly those alive.
    kc_plane *in_plane[KC_CHAIN_MAX_BATCH][KC_CHAIN_MAX_IN] = {};
    // filled when the recording is closed: input (b, k) is output channel in_ch of recorded launch in_from (-1: a plane that
    // existed before the evaluation and is held by the recording)
    int in_from[KC_CHAIN_MAX_BATCH][KC_CHAIN_MAX_IN];
    int in_ch[KC_CHAIN_MAX_BATCH][KC_CHAIN_MAX_IN];
};
struct ReplayCapture {
    bool ok = true;
    std::vector<ReplayLaunch> launches;
};

struct Context {
    std::recursive_mutex mu;
    ReplayCapture *capture = nullptr;
    uint64_t band_taps_clock = 0;
    bool inited = false;
    int device = -1;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    Options opt = option_defaults();  // the A/B and tuning switches: the option table, c_api.cpp
    bool plain_chains = false;  // set during a graph's first evaluation: chains as the interpreter runs them (4 planes, no joins)
    std::multimap<size_t, void *> free_blocks;
    uint64_t bytes_in_use = 0, bytes_cached = 0, launches = 0;
    std::map<std::string, uint64_t> counters;  // named event counts (kc_stats_counter): which kernel family ran, transfers ...
    // packed copies of chain inputs (chain_pack.cpp): pack_sources 0 = off, 1 = sources that HBM-bound launches keep reading, 2 = every
    // eligible input at once (tests); shadow_bytes = what the shadows hold now, never more than pack_budget_mb
    int pack_sources = 1, pack_budget_mb = 4096;
    uint64_t shadow_bytes = 0;
    uint64_t alg_bytes = 0;  // algorithmic HBM bytes of every kernel launched so far (DESIGN.md section 3's per-kernel figures)
    std::map<std::tuple<uint32_t, uint32_t, int>, TapsEntry> taps;
    std::map<std::tuple<uint32_t, uint32_t, int, int32_t, int32_t, int32_t>, TapsEntry> band_taps;  // row-band vertical tables
    // Within one graph evaluation the same plane resized to the same size with the same filter is
    // computed once (the reference resamples it per consuming node, src/shared.rs:152-207; planes
    // are immutable, so the result is identical).  Both planes are retained while memoised.
    int memo_depth = 0;
    std::map<std::tuple<kc_plane *, uint32_t, uint32_t, int>, kc_plane *> resize_memo;
    // image_from_u8's pinned staging ring: the caller's pixels are copied into a slot, the slot is DMA'd and the
    // call returns without waiting for the stream; a slot is reused once the event recorded behind its copy has fired.
    struct UploadSlot {
        void *host = nullptr;
        size_t bytes = 0;
        hipEvent_t copied = nullptr;
    };
    static constexpr int kUploadSlots = 4;
    static constexpr size_t kUploadSlotMax = (size_t)4 << 20;  // larger images keep the synchronous path
    UploadSlot upload_ring[kUploadSlots];
    int upload_next = 0;
    // kc_image_channel_stats (stats.cpp): the workgroups' partial records and the result on the device, the result's pinned
    // host copy and the event the call waits on -- allocated on first use, the partials grown when needed, freed at kc_shutdown
    struct StatsBuffers {
        void *partials = nullptr;
        size_t partials_bytes = 0;
        unsigned long long *result = nullptr, *host = nullptr;
        hipEvent_t done = nullptr;
        uint32_t cus = 0;
    };
    StatsBuffers stats;
    // kc_image_previews (preview.cpp): the pinned host copy of a batch's job tables and the event behind its upload -- allocated
    // on first use, grown when needed, freed at kc_shutdown
    struct PreviewBuffers {
        void *host = nullptr;
        size_t bytes = 0;
        hipEvent_t copied = nullptr;
    };
    PreviewBuffers preview;
};

// RAII scope for the resize memo (nested Graph nodes share the outermost scope).
struct ResizeMemoScope {
    ResizeMemoScope();
    ~ResizeMemoScope();
};

Context &ctx();
void set_error(const std::string &msg);
const std::string &last_error();
int hip_fail(hipError_t e, const char *what);  // records the message, returns KC_ERR_HIP
int need_init();                               // KC_OK or KC_ERR_NO_DEVICE

// Host-side phase timers for tuning (build with KC_HOST_PROFILE=1 python -m kanter_core_amd.build --force): each
// KC_PROF("name") scope adds its TSC cycles to a named counter, printed at kc_shutdown.  Compiled out otherwise.
#ifdef KC_HOST_PROFILE
struct ProfScope {
    const char *name;
    unsigned long long t0;
    explicit ProfScope(const char *n) : name(n), t0(__builtin_ia32_rdtsc()) {}
    ~ProfScope();
};
void prof_report();
#define KC_PROF(name) kc::ProfScope _kc_prof_scope(name)
#else
#define KC_PROF(name) (void)0
#endif

#ifdef KC_HOST_SAMPLE
void sampler_start();   // SIGPROF sampling of the host side, see runtime.cpp
void sampler_report();
#endif

#define KC_HIP(call)                                           \
    do {                                                       \
        hipError_t _e = (call);                                \
        if (_e != hipSuccess) return kc::hip_fail(_e, #call);  \
    } while (0)
#define KC_TRY(expr)                   \
    do {                               \
        int _s = (expr);               \
        if (_s != KC_OK) return _s;    \
    } while (0)

// ---- pool / planes (runtime.cpp) ----
int pool_alloc(size_t bytes, void **out);
void pool_free(void *p, size_t bytes);
int pool_trim();
// A pool block of `bytes` rounded up to 256 for the scope's staging, back to the pool when the scope ends: after the work that
// uses it has been enqueued on, or waited for on, the library's stream (the pool hands a block out again only to that stream)
struct PoolStaging {
    void *ptr = nullptr;
    size_t block = 0;
    PoolStaging() = default;
    PoolStaging(const PoolStaging &) = delete;
    PoolStaging &operator=(const PoolStaging &) = delete;
    int alloc(size_t bytes)
    {
        block = (bytes + 255) / 256 * 256;
        return pool_alloc(block, &ptr);
    }
    ~PoolStaging()
    {
        if (ptr) pool_free(ptr, block);
    }
};

int plane_new_mem(uint32_t w, uint32_t h, kc_plane **out);
kc_plane *plane_new_const(uint32_t w, uint32_t h, float v);
inline void plane_retain(kc_plane *p)
{
    if (p) ++p->refs;
}
void plane_release(kc_plane *p);
int plane_force(kc_plane *p);                           // LAZY -> MEM (CONST stays CONST)
int planes_force(kc_plane *const *planes, int n);       // batches chains that share a program
int plane_materialize(kc_plane *p);                     // LAZY/CONST -> MEM
// l op r for one channel (src/node/mix.rs:136-192): lazy chain, constant fold or immediate kernel.
int plane_mix(int mix_type, kc_plane *l, kc_plane *r, kc_plane **out);
// Batches the forces plane_mix would do one plane at a time (the channels of one Mix node).
int planes_mix_prepare(kc_plane *const *ls, kc_plane *const *rs, int n);
Operand plane_operand(const kc_plane *p);               // MEM or CONST only

kc_image *image_new(int n, kc_plane *const *planes);    // retains the planes
inline void image_retain(kc_image *img)
{
    if (img) ++img->refs;
}
void image_release(kc_image *img);
int image_force(kc_image *img);
// What every exporter reads.  o = the channels of `img` (forced) as to_u8 sees them (Gray: (v, v, v, 1)); returns the distinct
// resident planes among the channels of `mask`, which is what a launch under that mask loads: the one n_resident of
// cache_policy_mask and of alg_bytes
uint32_t image_source_operands(const kc_image *img, uint32_t mask, Operand (&o)[4]);
// What every importer writes.  p = `n_planes` (1: Gray, 4) fresh w x h planes, the first `n_mem` in memory (dp = their device
// pointers), the others the constants 0, 0, 0, 1 by channel; on failure nothing is left allocated.  image_of_import_planes is
// the tail of such a call: the image of the planes where `status` is KC_OK, the planes released either way; returns `status`.
int image_planes_for_import(uint32_t w, uint32_t h, int n_mem, int n_planes, kc_plane *(&p)[4], float *(&dp)[4]);
int image_of_import_planes(int status, int n_planes, kc_plane *(&p)[4], kc_image **out);

// ---- node operators (ops.cpp) ----
int image_from_value(kc_size size, float v, bool rgba, kc_image **out);
int image_as_type(kc_image *img, bool rgba, kc_image **out);
int image_from_u8(const uint8_t *host, uint32_t w, uint32_t h, int channels, kc_image **out);
int image_to_u8(kc_image *img, bool srgb, uint8_t *host);
// The u8 launches on the library's stream, with their cache policy and counters, between whatever copies and events the caller
// puts around them (u8pipe.cpp): from_u8_kernel of the bytes at `dev_src` into a new RGBA image / to_u8_kernel of `img` (forced)
// into the w * h * 4 bytes at `dev_dst`
int enqueue_from_u8(const uint8_t *dev_src, int channels, uint32_t w, uint32_t h, kc_image **out);
int enqueue_to_u8(kc_image *img, bool srgb, uint8_t *dev_dst);
// device-memory images (devimage.cpp): the bodies of kc_device_image_validate / kc_image_from_device / kc_image_to_device
int device_image_validate(const kc_device_image *d, size_t *extent_bytes);
int image_from_device(const kc_device_image *src, uint32_t flags, void *hip_stream, kc_image **out);
int image_to_device(kc_image *img, const kc_device_image *dst, uint32_t flags, void *hip_stream);
// [ptr, ptr + ext) lies in one device allocation of the library's device (KC_ERR_NO_DEVICE before kc_init, KC_ERR_INVALID_ARG
// otherwise, with `who` in the error text); stream_edge: `to` waits for the work already enqueued on `from`
int device_extent_check(const void *ptr, size_t ext, const char *who);
int stream_edge(hipStream_t from, hipStream_t to);
// work() -- which enqueues on the library's stream and returns a status -- between the two edges that order it against the
// caller's `hip_stream`: the library's stream waits for what that stream holds now, and that stream waits for the work.  No edges
// for NULL or the library's own stream; a failure ends the sequence where it happens.
template <class Work> int with_stream_edges(void *hip_stream, Work work)
{
    hipStream_t hs = (hipStream_t)hip_stream, own = ctx().stream;
    const bool edges = hs && hs != own;
    if (edges) KC_TRY(stream_edge(hs, own));
    KC_TRY(work());
    if (edges) KC_TRY(stream_edge(own, hs));
    return KC_OK;
}
// block compression (bc.cpp): the bodies of kc_bc_image_validate / kc_image_to_bc / kc_image_to_bc_device
int bc_image_validate(const kc_bc_image *d, size_t *extent_bytes);
int image_to_bc(kc_image *img, int format, uint32_t flags, uint8_t *host, size_t host_bytes);
int image_to_bc_device(kc_image *img, const kc_bc_image *dst, uint32_t flags, void *hip_stream);
// What a block format is, for the whole host side: one row per kc_bc_format in bc.cpp's table
struct BcFormat {
    int format;             // kc_bc_format
    uint32_t block_bytes;   // 8 or 16
    uint32_t channels;      // the source channels an encoder and a comparison read: bit c = channel c, contiguous low bits
    int planes;             // the planes a decode writes (the others are the constants 0, 0, 1)
    bool srgb;              // KC_BC_SRGB is allowed
    bool counts_undecoded;  // has modes the decoder does not decode, which it counts
    uint32_t dxgi, dxgi_srgb;  // the DXGI_FORMAT number kc_dds_header writes; with KC_BC_SRGB (0: none)
    bool dds_read;          // kc_dds_parse accepts it
    uint32_t fourcc[2];     // the legacy FourCCs kc_dds_parse accepts besides a DX10 header (0: none)
};
constexpr uint32_t fourcc(char a, char b, char c, char d)  // a .dds FourCC as the little-endian word of the file
{
    return (uint32_t)(uint8_t)a | (uint32_t)(uint8_t)b << 8 | (uint32_t)(uint8_t)c << 16 | (uint32_t)(uint8_t)d << 24;
}
const BcFormat *bc_format(int format);  // nullptr for an unknown format
// the format kc_dds_parse reads for a DX10 header's dxgiFormat (cc = 0) or a legacy FourCC (dxgi = 0), with its flags; or nullptr
const BcFormat *bc_format_of_dds(uint32_t dxgi, uint32_t cc, uint32_t *flags);
size_t bc_block_bytes(int format);  // 8, 16, or 0 for an unknown format
size_t bc_level_bytes(uint32_t w, uint32_t h, const BcFormat &f);  // the bytes of the blocks of a w x h level
// *bx, *by = the blocks per row and the block rows of a w x h image; more than 2^31 blocks are KC_ERR_INVALID_ARG under `who`
int bc_block_count(uint32_t w, uint32_t h, const char *who, uint64_t *bx, uint64_t *by);
// the encoders' flag rule: bits outside `allowed`, or KC_BC_SRGB with a format without colour, are KC_ERR_UNSUPPORTED
// KC_BC_PUNCH_THROUGH in `allowed` brings its rule: BC1 only, a reference byte 1..255 in bits 24-31 (which it shares with
// KC_MIP_COVERAGE; a byte with neither flag is refused), not with KC_MIP_NORMALS
int bc_check_flags(int format, uint32_t flags, uint32_t allowed, const char *who);
// the bits an entry point that takes KC_BC_PUNCH_THROUGH allows for it, and the reference byte of a checked flags word (0: no flag)
constexpr uint32_t kBcPunchThroughBits = KC_BC_PUNCH_THROUGH | 0xff000000u;
inline uint32_t bc_punch_through_ref(uint32_t flags) { return (flags & KC_BC_PUNCH_THROUGH) ? flags >> 24 : 0u; }
// kc_bc1_punch_through_block's rule on the host: 16 RGBA8 texels -> the 8 bytes of the block (ref 1..255)
void bc1_punch_through_block(const uint8_t rgba[64], uint32_t ref, uint8_t block[8]);
// one launch of the encoder for `img` (forced already) into `dst`, block rows `row_pitch` bytes apart, on `s`
// (pt_ref != 0: KC_BC_PUNCH_THROUGH with that reference byte)
int bc_encode(kc_image *img, int format, bool srgb, char *dst, size_t row_pitch, hipStream_t s, uint32_t pt_ref = 0);
// the launchers of kc_internal.hpp by format: the one place that knows which device unit holds a format's kernels
hipError_t bc_launch_encode(int format, bool srgb, const Operand op[4], int gray, char *dst, uint64_t row_pitch, uint32_t w, uint32_t h,
                            uint32_t nt_mask, hipStream_t s, uint32_t pt_ref = 0);
hipError_t bc_launch_decode(int format, bool all_modes, const BcDecodeArgs &a, bool count, uint32_t nt_mask, uint32_t groups, hipStream_t s);
hipError_t bc_launch_compare(int format, bool srgb, bool all_modes, const Operand op[4], int gray, const char *blocks, uint64_t row_pitch, uint32_t w, uint32_t h,
                             uint32_t nt_mask, uint32_t groups, unsigned long long *partials, unsigned long long *result, hipStream_t s,
                             uint32_t pt_ref = 0);
// block decode, the error of an encoding and .dds input (bc_decode.cpp): the bodies of kc_image_from_bc, kc_image_from_bc_device,
// kc_image_bc_compare, kc_image_bc_error, kc_dds_parse and kc_image_read_dds
int image_from_bc(const uint8_t *host, size_t host_bytes, uint32_t w, uint32_t h, int format, uint32_t flags, kc_image **out,
                  uint64_t *undecoded_blocks);
int image_from_bc_device(const kc_bc_image *src, uint32_t flags, void *hip_stream, kc_image **out, uint64_t *undecoded_blocks);
int image_bc_compare(kc_image *img, const kc_bc_image *blocks, uint32_t flags, kc_bc_error *out);
int image_bc_error(kc_image *img, int format, uint32_t flags, kc_bc_error *out);
int dds_parse(const uint8_t *data, size_t bytes, kc_dds_info *info);
int image_read_dds(const char *path, uint32_t level, uint32_t flags, kc_image **out, kc_dds_info *info);
// mip chains (mip.cpp): the bodies of kc_mip_level_count, kc_preview_level, kc_image_build_mips, kc_mip_normal_texel
inline uint32_t floor_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }  // v > 0
inline uint32_t level_extent(uint32_t v, uint32_t k) { return k < 32 && (v >> k) ? v >> k : 1u; }
int mip_refuse(const char *who, const char *what);  // records "who: what", returns KC_ERR_INVALID_ARG
// One launch of a chain's level walk: it reads level k (sw x sh) and writes `fused` levels with the family's pyramid kernel, or,
// with fused == 0, one level with its one-level kernel; nt: the cache policy of the launch
struct MipStep {
    uint32_t k, sw, sh, fused;
    bool nt;
    uint32_t last() const { return k + (fused ? fused : 1u); }  // the last level the launch writes; more follow where last() + 1 < L
};
// The launches of a chain of L levels of a w x h image, in stream order, for every family; nothing is enqueued.  A launch fuses
// as many levels as both extents still halve, six at the most; none after an extent has reached 1, and none under `per_level`
// (KC_MIP_PER_LEVEL).  nt is cache_policy_mask's answer for a launch that reads in0 planes (at level 0; in_below at a level
// below it) and writes out_planes planes per level.
std::vector<MipStep> mip_plan(uint32_t w, uint32_t h, uint32_t L, bool per_level, uint32_t in0, uint32_t in_below, uint32_t out_planes,
                              const Options &o = options());
int mip_level_count(uint32_t w, uint32_t h, uint32_t *levels);
int preview_level(uint32_t w, uint32_t h, uint32_t max_extent, uint32_t *level, uint32_t *pw, uint32_t *ph);
float mip_const_fold(float c);  // ((c + c) + (c + c)) * 0.25f, as the device computes it
void mip_normal_texel(const float box[3], float out[3]);  // KC_MIP_NORMALS: the boxes of R, G, B -> the stored texel, as the device computes it
int image_build_mips(kc_image *img, uint32_t flags, kc_image **levels, uint32_t cap, uint32_t *count);
// roughness chains (mip.cpp): the rule's arithmetic as kc_mip_unit_normal and kc_mip_roughness_texel return it, as the device
// computes it, and the body of kc_image_build_roughness_mips
void mip_unit_normal(const float rgb[3], float u[3]);
float mip_roughness_texel(const float m[3], float r, float power);
int image_build_roughness_mips(kc_image *img, uint32_t channel, kc_image *normals, float power, uint32_t flags, kc_image **levels, uint32_t cap,
                               uint32_t *count);
// KC_MIP_ALPHA_WEIGHT (mip.cpp): the rule's arithmetic as kc_mip_alpha_weight and kc_mip_alpha_texel return it, as the device
// computes it (mip_alpha_texel returns known)
float mip_alpha_weight(float a);
bool mip_alpha_texel(const float p[3], float w, float q[3]);
int mip_check_alpha_flags(uint32_t flags, const char *who);  // the flag's own refusal: a vector is not a colour
// KC_MIP_COVERAGE (mip.cpp): the rule's arithmetic as kc_alpha_ref_threshold, kc_mip_coverage_target and kc_mip_coverage_scale
// return it, the flag rule of the chain entry points (bit 64 and the reference byte in bits 24-31 go together), and the body of
// kc_image_mip_coverage_info
constexpr uint32_t kCoverageFlagBits = KC_MIP_COVERAGE | 0xff000000u;
float alpha_ref_threshold(uint32_t ref_u8);
int mip_coverage_target(uint32_t w, uint32_t h, uint64_t covered0, uint32_t level, uint64_t *target);
float mip_coverage_scale(float v, uint32_t ref_u8);
int mip_check_coverage_flags(uint32_t flags, const char *who);
int image_mip_coverage_info(kc_image *img, uint32_t flags, kc_mip_coverage_level *out, uint32_t cap, uint32_t *count);
// the export of mip chains (mip_export.cpp): the bodies of kc_bc_mip_layout, kc_image_to_bc_mips, kc_image_to_bc_mips_device,
// kc_dds_header, kc_image_write_dds
int bc_mip_layout(uint32_t w, uint32_t h, int format, uint32_t *levels, size_t *offsets, uint32_t cap, size_t *total_bytes);
int image_to_bc_mips(kc_image *img, int format, uint32_t flags, uint8_t *host, size_t host_bytes);
int image_to_bc_mips_device(kc_image *img, int format, uint32_t flags, void *device_ptr, size_t bytes, void *hip_stream);
int dds_header(uint32_t w, uint32_t h, int format, uint32_t flags, uint32_t levels, uint8_t *out, size_t *bytes);
int image_write_dds(kc_image *img, const char *path, int format, uint32_t flags, int with_mips);
// a chain the caller holds (mip_export.cpp): the bodies of kc_image_levels_to_bc_mips (who: the entry point's name) and kc_image_levels_write_dds
int image_levels_to_bc_mips(kc_image *const *levels, uint32_t count, int format, uint32_t flags, uint8_t *host, size_t host_bytes, const char *who);
int image_levels_write_dds(kc_image *const *levels, uint32_t count, const char *path, int format, uint32_t flags);
// previews (preview.cpp): the bodies of kc_preview_plan, kc_image_previews, kc_image_previews_device and (given the slots' images)
// kc_live_graph_buffer_previews; `imgs` (optional): the image of request i instead of r[i].image.  The context's buffers.
int preview_plan(uint32_t w, uint32_t h, uint32_t level, uint32_t x, uint32_t y, uint32_t rect_w, uint32_t rect_h, kc_preview_plan_info *out);
// the checks that look at no image: the flags, the arguments, every request's rect, offset, pitch and last byte (images_named: and its image)
int preview_check(const kc_preview_request *r, uint32_t count, uint32_t flags, const void *out, size_t out_bytes, bool images_named, const char *who);
int image_previews(const kc_preview_request *r, kc_image *const *imgs, uint32_t count, uint32_t flags, uint8_t *host, size_t host_bytes, const char *who);
int image_previews_device(const kc_preview_request *r, uint32_t count, uint32_t flags, void *device_ptr, size_t bytes, void *hip_stream);
void preview_release();
// per-channel statistics (stats.cpp): the body of kc_image_channel_stats; the context's buffers, released at kc_shutdown
int image_channel_stats(kc_image *img, uint32_t flags, kc_channel_stats *out);
uint32_t quant_u8_host(float v);  // streaming.h's quant_u8 on the host
int stats_buffers(size_t partials_bytes);  // the context's StatsBuffers, with room for that many bytes of partial records
int stats_fetch(uint32_t words);  // the first `words` result words of a reduction, in StatsBuffers::host once the call's event has fired
void channel_stats_release();
// signed distance fields (sdf.cpp): the rule's arithmetic as kc_sdf_cap and kc_sdf_texel return it, as the device computes it
// (spread 1..KC_SDF_MAX_SPREAD), and the body of kc_image_distance_field
uint32_t sdf_cap(uint32_t spread);
float sdf_texel(uint32_t d2, bool inside, uint32_t spread);
int image_distance_field(kc_image *img, uint32_t channel, uint32_t ref_u8, uint32_t spread, uint32_t flags, kc_image **out);
// Gaussian blur (blur.cpp): the rule's arithmetic as kc_blur_weights and kc_blur_texel return it (blur_weights checks the sigma
// and the capacity itself; blur_texel takes R in 1..KC_BLUR_MAX_RADIUS), and the body of kc_image_blur
int blur_weights(float sigma, float *weights, uint32_t capacity, uint32_t *radius);
float blur_texel(const float *taps, const float *weights, uint32_t R);
int image_blur(kc_image *img, float sigma_x, float sigma_y, uint32_t channel_mask, uint32_t flags, kc_image **out);
int calculate_size(int policy, const kc_size *sizes, int n, int slot_index, kc_size specific, kc_size *out);
int mix_process(kc_image *left, kc_image *right, int mix_type, kc_image **out);
int separate_process(kc_image *in, kc_image *out[4]);
int combine_process(kc_image *const in[4], kc_image **out);
int value_process(float v, kc_image **out);
int height_to_normal_process(kc_image *in, kc_image **out);
int height_to_normal_band(kc_image *in_with_halo, uint32_t full_h, kc_image **out);  // rows + 1 input rows, halo first

// ---- resize (resize.cpp) ----
int build_taps_host(uint32_t in_n, uint32_t out_n, int filter, TapsHost &t);
int resize_image(kc_image *src, kc_size size, int filter, kc_image **out);
int resize_force(kc_plane *p);  // RESIZE -> MEM through the plain resize kernel
int resize_planes_band(kc_plane *const *srcs, int n, int32_t src_y0, uint32_t src_h_full, kc_size dst_full, int32_t a, int32_t b,
                       int filter, kc_plane **outs);
int resize_force_many(kc_plane *const *planes, int n);  // same; equal resamples share launches
// Runs a chain whose operands include ONE resampled plane per channel inside the resize kernel
// (phase 2 feeds the chain program).  *launched = false when the case is not eligible (taps not
// in registers, tile does not fit LDS, program too long): the caller forces the RESIZE planes.
int chain_resize_launch(const ChainProgram &P, int batch, int mode, kc_plane *const *sampled, bool *launched);

// ---- run-time specialisation of the chain kernel (chain_codegen.cpp: signature and text; specialize.cpp: hiprtc, registry, launches) ----
// *nt_mask, *quads (optional): the cache-policy bits and the float4 per lane of the kernel that was launched
hipError_t launch_chain_specialized(const ChainProgram &P, int batch, hipStream_t s, bool *launched, uint32_t *nt_mask, uint32_t *quads = nullptr);
// Which streams of a launch are marked nontemporal: `in_bytes` / `out_bytes` = what the launch reads from its n_resident
// full-size input planes / writes, summed over its channels, under the options o.  Returns the ChainProgram::nt_mask bits.
uint32_t cache_policy_mask(uint64_t in_bytes, uint64_t out_bytes, uint32_t n_resident, const Options &o = options());
uint32_t chain_cache_policy(const uint32_t *refs, uint32_t n, uint64_t stream_bytes, uint64_t out_bytes);
// src (optional): the planes behind the inputs, [channel][input], nullptr where a plane must stay f32; refs as for
// chain_cache_policy.  *packed_saved (optional): the bytes the launch did not read because inputs were packed.
hipError_t chain_dispatch(ChainProgram &P, int batch, int mode, uint32_t w, uint32_t h, size_t out_pitch_bytes,
                          kc_plane *const (*src)[KC_CHAIN_MAX_IN] = nullptr, const uint32_t *refs = nullptr, uint64_t *packed_saved = nullptr);
// ---- packed copies of chain inputs (chain_pack.cpp) ----
// The tiers of P's inputs for this launch (ChainProgram::in_tiers), packing planes whose turn has come; 0 when nothing is packed.
uint32_t pack_chain_inputs(const ChainProgram &P, int batch, kc_plane *const (*src)[KC_CHAIN_MAX_IN], const uint32_t *refs, uint32_t w, uint32_t h);
void plane_shadow_drop(kc_plane *p, bool never_again);  // before an in-place write (never_again: the pointer leaves the library)
uint32_t pack_bytes_per_quad(uint32_t tier);            // 16 for KC_PACK_NONE
bool chain_pack_program_ok(const ChainProgram &P);      // chain_codegen.cpp: a flat {+, -, *} program whose kernel may read packed inputs
hipError_t launch_upsample_chain_specialized(const ChainProgram &P, int batch, const UpsampleArgs &U, hipStream_t s, bool *launched);
int specialize_set_mode(int mode, int after);  // 0 off, 1 background compile after `after` sightings, 2 compile at once
int specialize_get_mode();
int specialize_set_chain_quads(int quads);  // 0 the generator's rule, 1 / 2 / 4 forced where the rule allows more than one
int specialize_get_chain_quads();
void specialize_wait();
void specialize_stats(uint64_t *compiled, uint64_t *failed, uint64_t *launches, uint64_t *pending);
std::string specialize_last_log();
void specialize_shutdown();
std::string specialize_source(const ChainProgram &P, const UpsampleArgs *U = nullptr);
int specialize_compile_only(const std::string &src, std::string *log);
// what a cache file depends on besides the source text; the compile unit (specialize.cpp) hands it to kernel_cache.cpp
struct CompilerId {
    const char *const *opts;
    int n_opts;
    int version[2];  // of hiprtc
};
const CompilerId &compiler_id();
int rtc_compile(const std::string &src, std::vector<char> &code, std::string *log);
// code objects that outlive the process (kernel_cache.cpp)
struct Signature;  // chain_codegen.h
bool disk_load(const Signature &sig, const std::string &src, const CompilerId &cc, std::vector<char> &code);
void disk_load_refused();
void disk_store(const Signature &sig, const std::string &src, const CompilerId &cc, const std::vector<char> &code);
void disk_counters(uint64_t *hits, uint64_t *rejected, uint64_t *written);
int kernel_cache_set_dir(const char *dir);
void kernel_cache_stats(uint64_t *hits, uint64_t *rejected, uint64_t *written, uint64_t *kernels_loaded);
bool kernel_cache_populated();
int kernel_cache_precompile(const uint32_t *words, uint32_t n_ops, uint32_t n_in, int32_t start_src, bool flat, uint32_t nt_mask, uint32_t in_tiers,
                            uint32_t up_taps, bool up_wide, const char *dir, std::string *log);

// ---- the u8 boundary as a pipeline (u8pipe.cpp) ----
int u8_pipe_create(uint32_t w, uint32_t h, int channels, int depth, kc_u8_pipe **out);
int u8_pipe_free(kc_u8_pipe *p);
int u8_pipe_buffers(kc_u8_pipe *p, int slot, uint8_t **host_in, const uint8_t **host_out);
int u8_pipe_upload(kc_u8_pipe *p, int slot, kc_image **out);
int u8_pipe_download(kc_u8_pipe *p, int slot, kc_image *img, bool srgb);
int u8_pipe_wait_download(kc_u8_pipe *p, int slot);

// ---- png / json (png.cpp, json.cpp) ----
int png_read(const std::string &path, std::vector<uint8_t> &px, uint32_t &w, uint32_t &h, int &channels);
int png_write_rgba8(const std::string &path, const uint8_t *px, uint32_t w, uint32_t h);

// ------------------------------------------------------------------------------------------
// Graph model: src/node_graph.rs, src/node/mod.rs:113-123, src/edge.rs
// ------------------------------------------------------------------------------------------
struct NodeGraph;

struct Node {
    uint32_t node_id = 0;
    int type = KC_NODE_VALUE;
    int mix_type = KC_MIX_ADD;
    float value = 0.0f;
    uint32_t embed_id = 0;
    std::string text;                  // Input/Output name, Image/Write path
    std::shared_ptr<NodeGraph> graph;  // Graph node
    int policy = KC_POLICY_MOST_PIXELS;
    uint32_t policy_slot = 0;
    kc_size policy_size{ 0, 0 };
    int filter = KC_FILTER_TRIANGLE;

    bool is_input() const { return type == KC_NODE_INPUT_GRAY || type == KC_NODE_INPUT_RGBA; }
    bool is_output() const { return type == KC_NODE_OUTPUT_GRAY || type == KC_NODE_OUTPUT_RGBA; }
    bool is_source() const { return type == KC_NODE_EMBED || type == KC_NODE_IMAGE || is_input(); }  // holds data somebody provided
};

enum SlotType { SLOT_GRAY = 0, SLOT_RGBA = 1, SLOT_GRAY_OR_RGBA = 2 };
struct Slot {
    std::string name;
    uint32_t slot_id;
    int slot_type;
};

// Look-up tables over NodeGraph::nodes / edges, rebuilt on first use after a change: the evaluator asks
// "which node is this id", "which edges enter / leave this node" several times per node, and linear
// scans made an evaluation quadratic in the node count.
struct GraphIndex {
    uint64_t version = ~0ull;
    size_t n_nodes = 0, n_edges = 0;
    std::unordered_map<uint32_t, uint32_t> node_pos;             // node id -> position in nodes
    std::unordered_map<uint32_t, std::vector<kc_edge>> in_edges;  // by input_id, in insertion order
    std::unordered_map<uint32_t, std::vector<kc_edge>> out_edges; // by output_id, in insertion order
};

struct NodeGraph {
    std::vector<Node> nodes;
    std::vector<kc_edge> edges;
    uint32_t node_id_counter = 0;
    uint64_t version = 0;      // bumped by every change to nodes / edges (touch())
    mutable GraphIndex idx;

    void touch() { ++version; }
    const GraphIndex &index() const;
    bool index_is_current() const;
    void appended_node(bool index_was_current);  // after nodes.push_back: bumps the version, patches a current index
    void appended_edge(bool index_was_current);  // after edges.push_back
    void erased_edge(const kc_edge &e, bool index_was_current);  // after edges.erase
    const std::vector<kc_edge> &edges_into(uint32_t id) const;
    const std::vector<kc_edge> &edges_out_of(uint32_t id) const;

    const Node *find(uint32_t id) const;
    Node *find(uint32_t id);
    uint32_t new_id();
    int add_node(Node n, uint32_t *id);
    int add_node_with_id(Node n);
    int connect(uint32_t on, uint32_t in, uint32_t os, uint32_t is);
    int try_connect(uint32_t on, uint32_t in, uint32_t os, uint32_t is);
    int remove_edge(kc_edge e);
    int remove_node(uint32_t id, std::vector<kc_edge> *removed);
    int disconnect_slot(uint32_t id, int side, uint32_t slot, std::vector<kc_edge> *removed);
    std::vector<uint32_t> get_children(uint32_t id) const;
    std::vector<uint32_t> get_children_recursive(uint32_t id) const;
    std::vector<uint32_t> get_parents(uint32_t id) const;
    std::vector<uint32_t> output_ids() const;
    int rename_output_node(uint32_t id, const std::string &new_name, std::string *old_name);
    std::vector<Slot> input_slots_of_graph() const;
    std::vector<Slot> output_slots_of_graph() const;
};

std::vector<Slot> node_input_slots(const Node &n, bool *unimplemented = nullptr);
std::vector<Slot> node_output_slots(const Node &n, bool *unimplemented = nullptr);
Node node_from_desc(const kc_node_desc &d);
// the ancestors of `root` (itself last) in topological order; "graph has a cycle through node N" otherwise
int ancestors_topological(const NodeGraph &g, uint32_t root, std::vector<uint32_t> &topo);
// the slot that stands for a requested node: a Graph node's first Output id; slot 0 otherwise (every other node's first output slot)
int root_output_slot(const NodeGraph &g, uint32_t root, uint32_t *slot);

int graph_from_json(const std::string &text, NodeGraph &g);
std::string graph_to_json(const NodeGraph &g);

}  // namespace kc

struct kc_node_graph {
    kc::NodeGraph g;
};

namespace kc {

struct SlotData {
    uint32_t node_id, slot_id;
    kc_image *image;  // retained
};

// A vector of plain records with room for N of them inside the object: the evaluator builds half a dozen
// two-or-three-element lists per node (inputs, resized, assigned, results ...) and the heap round trips for
// them were a measurable part of the ~0.7 us a node costs on the host.
template <class T, size_t N> class SmallVec {
    static_assert(std::is_trivially_copyable<T>::value, "SmallVec holds plain records only");
    T inl_[N];
    T *p_ = inl_;
    size_t n_ = 0, cap_ = N;

    void grow(size_t want)
    {
        size_t cap = cap_ * 2 > want ? cap_ * 2 : want;
        T *q = static_cast<T *>(::operator new(cap * sizeof(T)));
        std::memcpy(static_cast<void *>(q), p_, n_ * sizeof(T));
        if (p_ != inl_) ::operator delete(p_);
        p_ = q;
        cap_ = cap;
    }

public:
    SmallVec() = default;
    SmallVec(const T *first, size_t n) { assign(first, n); }
    SmallVec(const SmallVec &o) { assign(o.p_, o.n_); }
    SmallVec &operator=(const SmallVec &o)
    {
        if (this != &o) assign(o.p_, o.n_);
        return *this;
    }
    ~SmallVec()
    {
        if (p_ != inl_) ::operator delete(p_);
    }
    void assign(const T *first, size_t n)
    {
        n_ = 0;
        if (n > cap_) grow(n);
        if (n) std::memcpy(static_cast<void *>(p_), first, n * sizeof(T));
        n_ = n;
    }
    void push_back(const T &v)
    {
        if (n_ == cap_) {
            const T copy = v;  // v may live in this vector
            grow(n_ + 1);
            p_[n_++] = copy;
            return;
        }
        p_[n_++] = v;
    }
    void clear() { n_ = 0; }
    void erase_at(size_t i)
    {
        std::memmove(static_cast<void *>(p_ + i), p_ + i + 1, (n_ - i - 1) * sizeof(T));
        --n_;
    }
    size_t size() const { return n_; }
    bool empty() const { return n_ == 0; }
    T *data() { return p_; }
    const T *data() const { return p_; }
    T &operator[](size_t i) { return p_[i]; }
    const T &operator[](size_t i) const { return p_[i]; }
    T *begin() { return p_; }
    T *end() { return p_ + n_; }
    const T *begin() const { return p_; }
    const T *end() const { return p_ + n_; }
};
using SlotList = SmallVec<SlotData, 8>;
using EdgeList = SmallVec<kc_edge, 8>;
// node_type.rs:229-231: a node's edges sorted stably by input slot
EdgeList edges_by_input_slot(const kc_edge *edges, size_t n);
// shared.rs:113-131: which of `producers` (the inputs, in input order) a SpecificSlot policy means -- the edge on the named
// slot, else the one on the lowest connected slot; -1 for every other policy and when nothing is connected
int policy_slot_index(int policy, uint32_t policy_slot, const kc_edge *sorted, size_t n_sorted, const kc_edge *producers, size_t n);

struct EmbeddedSlotData {
    uint32_t slot_data_id, slot_id;
    kc_image *image;
    // row-band evaluation only (bands.cpp): full_h != 0 => `image` holds logical rows band_y0 .. of a full_h-row image
    int32_t band_y0 = 0;
    uint32_t full_h = 0;
};

}  // namespace kc

struct kc_tex_pro {
    uint64_t memory_threshold = 0;
    std::recursive_mutex mu;
};

struct kc_live_graph {
    kc_tex_pro *tp = nullptr;
    kc::NodeGraph g;
    // by producing node, slots in the order the node returned them (a linear list made every look-up and every
    // replacement a scan of all cached slots: quadratic with use_cache on a long graph)
    std::unordered_map<uint32_t, kc::SmallVec<kc::SlotData, 4>> slot_datas;
    const kc::SmallVec<kc::SlotData, 4> &slots_of(uint32_t node) const;
    std::vector<kc::EmbeddedSlotData> embedded;
    std::vector<kc::SlotData> input_slot_datas;
    std::unordered_map<uint32_t, int> node_state;  // looked up a dozen times per node and evaluation
    std::unordered_set<uint32_t> changed;  // reported in ascending id order (kc_live_graph_changed_consume)
    bool auto_update = false;
    bool use_cache = false;
    uint64_t walks = 0;  // evaluations that were walked (not replayed): the first one builds plain chains, see await_clean
    std::string base_dir;
    int depth = 0;  // nesting depth of Graph nodes (recursion guard)
    struct ReplayEntry;
    ReplayEntry *replay = nullptr;  // the last evaluation that qualified, recorded for replay (replay.cpp)
    void replay_clear();

    ~kc_live_graph();
    void clear_data();
    void remove_nodes_data(uint32_t id);
    const kc::SlotData *find_slot(uint32_t node, uint32_t slot) const;
    const kc::EmbeddedSlotData *find_embedded(uint32_t embed_id) const;
    const kc::SlotData *find_input(const kc::Node &n) const;  // InputRgba: the first entry (input_rgba.rs:7-13); InputGray: the node's own
    std::string resolve_path(const std::string &p) const;     // an Image / Write node's path, relative to base_dir
    int state_of(uint32_t id, int *st) const;
    int set_state(uint32_t id, int st);
    int force_state(uint32_t id, int st);
    void reset_node_states();
    int add_node(kc::Node n, uint32_t *id);
    int add_node_with_id(kc::Node n);
    int remove_node(uint32_t id);
    int connect(uint32_t on, uint32_t in, uint32_t os, uint32_t is);
    int remove_edge(kc_edge e);
    int disconnect_slot(uint32_t id, int side, uint32_t slot);
    int ensure_clean(uint32_t id);
    int import_slot_data(uint32_t node, uint32_t slot, kc_image *image);  // partition.cpp
    int await_clean(uint32_t id);
    int await_clean_walk(uint32_t id);
    int update();
    int process_one(uint32_t id);
};

// Multi-GPU placement plan (partition.cpp)
struct kc_partition {
    int world = 1, home = 0, n_levels = 1;
    int kind = KC_PLAN_BRANCHES;
    bool gather = true;  // KC_PLAN_BANDS: the bands end on the home rank (kc_partition_set_gather)
    uint32_t root = 0;
    std::vector<kc_placement> nodes;  // topological order
    std::vector<kc_transfer> xfers;   // execution order: level, producer's topological position, slot, destination
    std::vector<kc_band_range> bands;  // KC_PLAN_BANDS: rows [y0, y1) of the requested node per rank
    uint32_t full_w = 0, full_h = 0;
    double est_single = 0.0, est_branches = 0.0, est_bands = -1.0;  // what KC_PARTITION_AUTO compared (partition.cpp)
};

namespace kc {
// Row-band evaluation (bands.cpp)
int band_evaluate(kc_live_graph &lg, uint32_t root, uint32_t slot, int32_t y0, int32_t y1, kc_image **out);
int band_source_rows(kc_live_graph &lg, uint32_t root, int32_t y0, int32_t y1, std::vector<kc_band_rows> &out);
int partition_plan(kc_live_graph &lg, uint32_t root, int world, int policy, kc_partition **out);
int band_plan_info(kc_live_graph &lg, uint32_t root, kc_size *size, bool *rgba);  // the requested node's logical size, if the band walk takes the graph
// Replay of a recorded evaluation (replay.cpp)
struct ReplayRecorder;
int replay_try(kc_live_graph &lg, uint32_t id, bool *hit);
ReplayRecorder *replay_begin(kc_live_graph &lg, uint32_t id);
void replay_end(kc_live_graph &lg, uint32_t id, ReplayRecorder *r, int s);
// The exchange (comm.cpp): a shared-memory mailbox + IPC copies or RCCL.  Callers hold the context lock.
int comm_unique_id(void *id, size_t bytes);
int comm_init(int rank, int world, const void *id, size_t bytes);
int comm_destroy();
void comm_info(int *rank, int *world);
void comm_stats(uint64_t *planes_sent, uint64_t *planes_received, uint64_t *bytes_sent);
int comm_exchange(kc_live_graph &lg, const kc_transfer *t, uint32_t n);
int comm_evaluate_partitioned(kc_live_graph &lg, const kc_partition &plan, uint32_t root, kc_image **out);
int comm_gather_bands(kc_image *band, int32_t y0, uint32_t full_h, int home, kc_image **out);
const char *comm_wire_name();
void comm_blocks_freed();  // kc_pool_trim has given blocks back to the driver
void comm_sync();
// process_node, src/node/node_type.rs:213-248: inputs in edge insertion order.
int process_node(kc_live_graph &lg, const Node &node, const SlotList &inputs, const std::vector<kc_edge> &edges,
                 SlotList &out);
// process_node_internal, src/node/node_type.rs:98-138, on assigned inputs.  full_h > 1: `sd` holds row bands of images
// full_h rows high (bands.cpp), HeightToNormal's with the halo row first; 0: whole images.
int dispatch(kc_live_graph &lg, const Node &node, const SlotList &sd, uint32_t full_h, SlotList &out);
}  // namespace kc
