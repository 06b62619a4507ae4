/*
 * kanter_core_amd.h -- C ABI of the MI355X (gfx950) per-pixel evaluation backend for
 * kanter_core / vismut_core 0.10.0 graphs.
 *
 * This is the drop-in boundary: plain pointers, sizes and opaque handles, no C++ or torch types.
 * The reference (pure Rust, no FFI of its own) would bind these from an `extern "C"` block and
 * call them from the bodies behind its operator boundary, `process_node`
 * (src/node/node_type.rs:213-248) and the per-node `process` functions it dispatches to
 * (src/node/node_type.rs:107-122).  Each entry point cites the reference interface it replaces;
 * paths are relative to the reference checkout.  INTEGRATION.md shows the Rust-side binding.
 *
 * Data model (replaces src/slot_image.rs:12-19 and src/transient_buffer.rs):
 *   kc_plane  one channel: row-major f32, `pitch` bytes per row (pitch >= 4*width, 256-byte
 *             aligned for planes this library allocates) living in HBM -- or a broadcast
 *             constant / a not-yet-materialised pointwise chain (see kc_plane_materialize).
 *             Planes are immutable once published and shared by reference count exactly where
 *             the reference clones an Arc<TransientBufferContainer>.
 *   kc_image  SlotImage: Gray = 1 plane, Rgba = 4 planes (R, G, B, A).
 *
 * All functions return a kc_status (0 = ok).  1..19 mirror TexProError (src/error.rs:5-27);
 * >= 100 are backend errors.  Every entry point is thread-safe; work is enqueued in order on
 * one HIP stream per process (kc_set_stream) and is complete after kc_sync() or any call that
 * returns host data.
 */
#ifndef KANTER_CORE_AMD_H
#define KANTER_CORE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KC_API __attribute__((visibility("default")))

/* ---- status codes: TexProError, src/error.rs:5-27 --------------------------------------- */
typedef enum kc_status {
    KC_OK = 0,
    KC_ERR_GENERIC = 1,
    KC_ERR_CANCELED = 2,
    KC_ERR_IMAGE = 3,
    KC_ERR_INVALID_BUFFER_COUNT = 4,
    KC_ERR_INVALID_NODE_ID = 5,
    KC_ERR_INVALID_NODE_TYPE = 6,
    KC_ERR_INVALID_SLOT_ID = 7,
    KC_ERR_INVALID_SLOT_TYPE = 8,
    KC_ERR_INVALID_EDGE = 9,
    KC_ERR_NO_SLOT_DATA = 10,
    KC_ERR_SLOT_OCCUPIED = 11,
    KC_ERR_SLOT_NOT_OCCUPIED = 12,
    KC_ERR_UNABLE_TO_LOCK = 13,
    KC_ERR_NODE_PROCESSING = 14,
    KC_ERR_POISON = 15,
    KC_ERR_TRY_LOCK = 16,
    KC_ERR_NODE_DIRTY = 17,
    KC_ERR_IO = 18,
    KC_ERR_INVALID_NAME = 19,
    /* backend */
    KC_ERR_HIP = 100,          /* a HIP runtime call failed; kc_last_error() has the text */
    KC_ERR_NO_DEVICE = 101,    /* no gfx950 device / kc_init not called: there is NO CPU fallback */
    KC_ERR_INVALID_ARG = 102,
    KC_ERR_OUT_OF_MEMORY = 103,
    KC_ERR_UNSUPPORTED = 104
} kc_status;

/* MixType, src/node/mix.rs:20-27 */
typedef enum kc_mix_type { KC_MIX_ADD = 0, KC_MIX_SUBTRACT = 1, KC_MIX_MULTIPLY = 2, KC_MIX_DIVIDE = 3, KC_MIX_POW = 4 } kc_mix_type;
/* ResizeFilter, src/node/mod.rs:62-69 (default Triangle, :71-75) */
typedef enum kc_resize_filter { KC_FILTER_NEAREST = 0, KC_FILTER_TRIANGLE = 1, KC_FILTER_CATMULLROM = 2, KC_FILTER_GAUSSIAN = 3, KC_FILTER_LANCZOS3 = 4 } kc_resize_filter;
/* ResizePolicy, src/node/mod.rs:33-41 (default MostPixels, :43-47) */
typedef enum kc_resize_policy { KC_POLICY_MOST_PIXELS = 0, KC_POLICY_LEAST_PIXELS = 1, KC_POLICY_LARGEST_AXES = 2, KC_POLICY_SMALLEST_AXES = 3, KC_POLICY_SPECIFIC_SLOT = 4, KC_POLICY_SPECIFIC_SIZE = 5 } kc_resize_policy;
/* NodeType, src/node/node_type.rs:14-28 */
typedef enum kc_node_type {
    KC_NODE_INPUT_GRAY = 0, KC_NODE_INPUT_RGBA = 1, KC_NODE_OUTPUT_GRAY = 2, KC_NODE_OUTPUT_RGBA = 3,
    KC_NODE_GRAPH = 4, KC_NODE_IMAGE = 5, KC_NODE_EMBED = 6, KC_NODE_WRITE = 7, KC_NODE_VALUE = 8,
    KC_NODE_MIX = 9, KC_NODE_HEIGHT_TO_NORMAL = 10, KC_NODE_SEPARATE_RGBA = 11, KC_NODE_COMBINE_RGBA = 12
} kc_node_type;
/* NodeState, src/live_graph.rs:22-37 */
typedef enum kc_node_state { KC_STATE_CLEAN = 0, KC_STATE_DIRTY = 1, KC_STATE_REQUESTED = 2, KC_STATE_PRIORITISED = 3, KC_STATE_PROCESSING = 4, KC_STATE_PROCESSING_DIRTY = 5 } kc_node_state;
/* Side, src/node/mod.rs:101-105 */
typedef enum kc_side { KC_SIDE_INPUT = 0, KC_SIDE_OUTPUT = 1 } kc_side;

typedef struct kc_plane kc_plane;
typedef struct kc_image kc_image;
typedef struct kc_node_graph kc_node_graph;
typedef struct kc_live_graph kc_live_graph;
typedef struct kc_tex_pro kc_tex_pro;
typedef struct kc_partition kc_partition;   /* multi-GPU placement plan of one graph evaluation */
typedef struct kc_u8_pipe kc_u8_pipe;       /* pipelined u8 host boundary (pinned buffers, copy streams) */

/* Size, src/slot_data.rs:4-30 */
typedef struct kc_size { uint32_t width, height; } kc_size;
/* Edge, src/edge.rs:8-14 */
typedef struct kc_edge { uint32_t output_id, input_id, output_slot, input_slot; } kc_edge;

/* Node, src/node/mod.rs:113-123 (priority / cancel are host scheduling state, not carried). */
typedef struct kc_node_desc {
    uint32_t node_id;          /* NodeId */
    int32_t node_type;         /* kc_node_type */
    int32_t mix_type;          /* kc_mix_type, for KC_NODE_MIX */
    float value;               /* for KC_NODE_VALUE */
    uint32_t embed_id;         /* EmbeddedSlotDataId, for KC_NODE_EMBED */
    const char *text;          /* Input/Output name, Image/Write path; may be NULL */
    const kc_node_graph *graph;/* nested graph for KC_NODE_GRAPH (copied) */
    int32_t resize_policy;     /* kc_resize_policy */
    uint32_t policy_slot;      /* SpecificSlot(SlotId) */
    kc_size policy_size;       /* SpecificSize(Size) */
    int32_t resize_filter;     /* kc_resize_filter */
} kc_node_desc;

/* ========================================================================================== *
 * Device / context
 * ========================================================================================== */
/* Binds the process to one gfx950 device (one process per GPU).  Fails with KC_ERR_NO_DEVICE
 * when no GPU is present -- the library never computes on the CPU. */
KC_API int kc_init(int device_ordinal);
KC_API int kc_shutdown(void);
KC_API int kc_is_initialized(void);
/* Enqueue all work on the caller's hipStream_t (e.g. torch's current stream); NULL restores the
 * library's own stream.  Replaces the reference's thread-per-node scheduling, src/engine.rs:288. */
KC_API int kc_set_stream(void *hip_stream);
KC_API void *kc_get_stream(void);
KC_API int kc_sync(void);
KC_API const char *kc_last_error(void);
KC_API const char *kc_status_string(int status);
/* The options "fusion", "resize_mode" and "cache_policy" of kc_set_option. */
KC_API int kc_set_fusion(int enabled);
KC_API int kc_get_fusion(void);
KC_API int kc_set_resize_mode(int mode);
KC_API int kc_get_resize_mode(void);
KC_API int kc_set_cache_policy(int mode);
KC_API int kc_get_cache_policy(void);
/* Named A/B and tuning switches: results are bit-identical whatever they say.  An unknown name or a value outside the
 * accepted ones is refused (KC_ERR_INVALID_ARG, the option unchanged); a flag takes any integer and stores it as 0 / 1.
 * kc_init reads each option from KC_<NAME> (the name in upper case, e.g. KC_DOWN2=0) if set, as a whole decimal integer
 * (KC_NT_FORCE also 0x...); a value kc_set_option would refuse fails kc_init with KC_ERR_INVALID_ARG.  Name (default;
 * accepted values): meaning --
 *   "chain1" (1; flag): a single Mix step runs its ahead-of-time kernel; 0: the interpreter / specialiser, as longer programs.
 *   "replay" (1; flag): an evaluation that repeats the previous one of the same node exactly (same graph by content, node
 *     states, slot data and embedded images by identity) re-issues the recorded launches (src/engine.rs:200-307 not walked).
 *   "join" (1; flag): a Mix of two chains that have not run keeps both in one program (one launch, csrc/runtime.cpp plane_mix;
 *     only kernels compiled at run time, else the second chain runs on its own); 0: always run it on the spot.
 *   "wide" (1; flag): a fused chain reads up to 16 planes per channel (kernels compiled at run time; else 4); 0: 4.
 *   "fusion" (1; flag): pointwise Mix chains whose intermediates are never observed run as one kernel; 0: every node
 *     materialises its planes.
 *   "down2" (1; 0..2): down-sampling with more than 8 taps on both axes runs resize_down2_kernel never / except where
 *     resize_poly_kernel runs at ratio 4 or 8 / wherever its tables exist.
 *   "down2_by_rows" (-1; -1..1): resize_down2_kernel's jobs: four strips of one row group per workgroup, the XCDs' eighths row
 *     by row (1), four row groups of one strip (0), 1 where the windows span several chunks (-1).
 *   "poly2" (1; 0..1): integer vertical ratios from poly2_min_ratio with windows of 4 or 6 ages run resize_poly2_kernel.
 *   "poly2_min_ratio" (8; >= 2): see poly2 (8: where it measures faster; 2: everywhere it can run).
 *   "resize_mode" (0; 0..4): 0 every resize kernel; 1 no resize_poly_kernel; 2 no resize_down_kernel either; 3 two passes through
 *     HBM only; 4 no integer-ratio up-sampling kernels.  (The reference has one code path, src/shared.rs:159-199.)
 *   "resize_tile_w" (0; 0..1024), "resize_tile_h" (0; 0..64): the output tile of the tiled resize kernels where both are set and
 *     it fits; resize_tile_w alone: the up-sampling kernels' tile width; resize_tile_h = 32: resize_down_kernel 8 rows per wave.
 *   "poly_rows" (0; >= 0): rows per band of resize_poly(2)_kernel, rounded down to a multiple of 4, at least 4; 0: by the launch.
 *   "poly2_xcd" (-1; -1..2): resize_poly2_kernel's bands in plain order (0), XCD eighths strip-major (2) / band-major (-1, 1).
 *   "down2_xcd" (-1; -1..1): resize_down2_kernel's tiles in XCD order never (0), always (1), while they fit cache_budget_mb (-1).
 *   "h2n_tiled" (-1; -1..1): HeightToNormal's workgroups as tiles of column blocks; 0: round 2's plain mapping.
 *   "cache_policy" (1; 0..1): a launch that streams more than cache_budget_mb reads its full-size inputs nontemporal and keeps
 *     its result cacheable while that fits; 0: plain loads and stores everywhere.
 *   "cache_budget_mb" (208; >= 0): what the cache policy leaves cacheable: 13/16 of the MI355X's 256 MB Infinity Cache, the
 *     share that measured best (profiles/r03_tilecopy4.txt); HIP reports no size for that cache, so another part sets this.
 *   "nt_force" (-1; >= -1): this nontemporal mask for every launch the cache policy marks (bits 0-7 and 16-23 inputs, 8 result).
 *   "chain_unroll" (0; one of 0, 1, 2, 4, 6, 8): float4 per lane of the step interpreter without divide or pow; 0: measured.
 *   "max_blocks" (4096; >= 1): the step interpreter's grid cap, beyond which its workgroups stride over the plane.
 *   "tune_cap" (0; >= 0): the grid cap of the grid-stride streaming kernels (to_u8, from_u8, height_to_normal); 0: none.
 *   "upload_ring" (1; flag): kc_image_from_u8 of at most 4 MB copies into a pinned ring and returns; 0: copies and waits.
 *   "link_gbps" (153; >= 1), "hbm_gbps" (6100; >= 1): what kc_live_graph_partition prices a transfer / a streaming kernel at. */
KC_API int kc_set_option(const char *name, int value);
KC_API int kc_get_option(const char *name, int *value);
/* Diagnostics (host only, works without a device): the structure the integer-ratio up-sampling kernels rely on,
 * for one axis of image::imageops::resize (src/shared.rs:159-199) from in_n to out_n samples with `filter`.
 * *eligible = 0: the tap table does not have it (not a whole ratio, an even window ...) and the general kernels run.
 * Otherwise info = { ratio, taps, off, b_lo, b_hi }: the window of output o is source samples
 * [o / ratio - off, o / ratio - off + taps) cut to the source; outputs b_lo .. out_n - b_hi - 1 use weight row
 * o % ratio, the first b_lo and last b_hi outputs rows ratio + o and ratio + b_lo + (o - (out_n - b_hi));
 * `rows` receives those (ratio + b_lo + b_hi) x taps weights (as many as fit `cap` floats). */
KC_API int kc_resize_upsample_plan(uint32_t in_n, uint32_t out_n, int filter, int *eligible, int32_t info[5], float *rows,
                                   size_t cap);
/* Diagnostics (host only): what resize_down2_kernel (csrc/down2.hip: down-sampling with more than 8 taps on both axes) reads for
 * one axis of image::imageops::resize (src/shared.rs:159-199).  info = { stride (most taps of any output), nc, hstride, tile_w,
 * fewest taps of any output }.  nc = records per group of four outputs when the table serves as the VERTICAL one (0: it cannot --
 * at most 8 taps, or some group's windows span more than 64 source samples); hstride / tile_w = row pitch of the padded weights
 * and strip width when it serves as the HORIZONTAL one (0: it cannot).  Optional outputs: left_count = out_n window starts then
 * out_n tap counts, w = out_n x stride weights of the plain table, vrec = ceil(out_n / 4) x nc records of 72 dwords ([0] first
 * source sample, [1], [2] presence mask of tap (sample u, output k) at bit 4 u + k, [3] last sample of the group's windows, [4]
 * records in use, [5] the same in halves of 8 samples, [8 + 4 u + k] weights), hw = out_n x hstride padded weights; each as many elements as its capacity allows. */
KC_API int kc_resize_down2_plan(uint32_t in_n, uint32_t out_n, int filter, int32_t info[5], uint32_t *left_count, float *w, size_t wcap,
                                uint32_t *vrec, size_t vcap, float *hw, size_t hcap);
/* Pool statistics: bytes currently handed out, bytes cached for reuse, kernels launched. */
KC_API int kc_stats(uint64_t *bytes_in_use, uint64_t *bytes_cached, uint64_t *kernel_launches);
/* Algorithmic HBM bytes of every kernel launched so far: per launch, each resident input plane read once and each
 * result plane written once (what a roofline divides by; fused intermediates and constant planes cost nothing). */
KC_API int kc_stats_algorithmic_bytes(uint64_t *bytes);
/* Named event counters since kc_init (tests and profiling: which kernel family a call went through).  Unknown names
 * read 0.  Names: "upsample_launches", "upsample_chain_launches" (the integer-ratio up-sampling kernels),
 * "resize_chain_launches" (the general fused resample + chain kernel), "chain1_launches" (one-step programs through the
 * ahead-of-time kernels), "replayed_evaluations".  The plain resize forms: "poly2_launches", "down2_launches",
 * "resize_poly_launches", "resize_down_launches", "resize_lds_launches", "resize_wide_launches" (one per launch) and
 * "resize_two_pass_launches" (one per plane: a vertical and a horizontal pass); the variant each launch took from its size:
 * "poly_rows_<n>" / "poly2_rows_<n>" (band height), "poly2_xcd_order", "down2_xcd_order", "down2_by_rows" (job orders;
 * neither of down2's: the plain 2-D grid), "upsample_nt_stores", "upsample_half_quads" (ratio 2).  The chain forms (one per
 * launch): "chain_interp_k<K>_u<U>_m<MODE>" and the same with "_nt" (the step interpreter with K input planes, U float4 per
 * lane, op set MODE 0 {+, -, *}, 1 + divide, 2 + pow, and its nontemporal form), "chain_k0_m<MODE>" (no input plane),
 * "chain1_nt<0-7>" (a one-step kernel with its nontemporal bits: 1 the start plane, 2 the operand, 4 the result),
 * "specialized_nt_<3 hex digits>" (a kernel compiled at run time and its cache-policy bits: 0x001 << k input plane k < 8,
 * 0x100 the result), "specialized_nt_<3 hex digits>_q2" / "_q4" when that kernel handles 2 / 4 float4 per lane instead of one
 * (kc_set_chain_quads).  The mip kernels (one per launch): "mip_pyramid", "mip_level", under KC_MIP_NORMALS "mip_normals_pyramid",
 * "mip_normals_level" for R, G, B, "mip_nt" for each of those launches that reads its source nontemporally, "mip_coverage" for
 * the launches KC_MIP_COVERAGE adds, and under KC_MIP_ALPHA_WEIGHT "mip_alpha_pull_pyramid", "mip_alpha_pull_level" and
 * "mip_alpha_push".  The streaming kernels, by the form each launch took: HeightToNormal "h2n_launches", one
 * of "h2n_plain", "h2n_tiled_q5", "h2n_tiled_q6", "h2n_tiled_q7" (a row per 256 threads, or tiles of 32, 64, 128 column
 * quads), "h2n_band" (a row band with its halo row), "h2n_nt" (nontemporal stores); the u8 boundary "to_u8_nt", "from_u8_nt"
 * (kc_image_to_u8 / _from_u8 and the u8 pipe); device images "image_import_vec" or "image_import_scalar" and
 * "image_export_vec" or "image_export_scalar" (whether the descriptor's alignment allows whole-quad accesses),
 * "image_import_nt", "image_export_nt"; "stats_nt" (kc_image_channel_stats). */
KC_API int kc_stats_counter(const char *name, uint64_t *value);
KC_API int kc_pool_trim(void);
/* Run-time specialisation of the fused Mix-chain kernel.  A chain of N Mix nodes (src/node/mix.rs:136-192
 * applied N times) normally runs through a step-table interpreter; a program that keeps coming back is also
 * emitted as straight-line HIP, compiled with hiprtc (same parity flags as the offline build) and used from
 * then on.  Results are bit-identical either way; this is a throughput knob only.
 *   mode 0: interpreter only.  mode 1 (default, env KC_SPECIALIZE): compile in the background once a program
 *   has been seen `after` times (default 2; <= 0 keeps the current value); launches never wait.
 *   mode 2: compile at the first sighting, the launch waits for the compiler (tests, batch jobs).
 * kc_specialize_wait blocks until every queued compile has landed. */
KC_API int kc_set_specialize(int mode, int after);
KC_API int kc_get_specialize(void);
KC_API int kc_specialize_wait(void);
KC_API int kc_specialize_stats(uint64_t *kernels_compiled, uint64_t *compiles_failed, uint64_t *specialized_launches,
                               uint64_t *compiles_pending);
/* Diagnostics: generates the specialised kernel for a program given as step words (ChainCode | (source + 1) << 8,
 * source = -1 for the step's constant, k for input plane k) and compiles it for gfx950 WITHOUT loading it -- works
 * without a device.  The generated source is copied to `source` (NUL-terminated, truncated to `cap`) when given. */
KC_API int kc_specialize_compile_check(const uint32_t *words, uint32_t n_ops, uint32_t n_in, int start_src, int flat,
                                       char *source, size_t cap);
/* The same for the plain chain kernel under the cache-policy mask `nt_mask` (bits as in "specialized_nt_<hex>"). */
KC_API int kc_specialize_compile_check_mask(const uint32_t *words, uint32_t n_ops, uint32_t n_in, int start_src, int flat,
                                            uint32_t nt_mask, char *source, size_t cap);
/* float4 per lane of the compiled plain chain kernels, for A/B runs only.  0 (default): the generator's rule -- two where a
 * flat {+, -, *} program of at most 16 records leaves at least one input plain (cache resident) beside a nontemporal input or result, so that the
 * body of one quad runs under the outstanding loads of the next; one everywhere else.  1, 2, 4: that many where the rule
 * allows more than one.  Part of a kernel's signature: changing it never launches a kernel with another form's grid. */
KC_API int kc_set_chain_quads(int quads);
KC_API int kc_get_chain_quads(void);
/* The same for a program that runs inside the integer-ratio up-sampling kernel (the resampled operand is input slot
 * n_in - 1; `taps` = 1 or 3 per axis, `wide` = the 1024-column tile form): src/shared.rs:159-199 feeding
 * src/node/mix.rs:136-192 in one launch. */
KC_API int kc_specialize_compile_check_upsample(const uint32_t *words, uint32_t n_ops, uint32_t n_in, int start_src, uint32_t taps,
                                                int wide, char *source, size_t cap);
/* Compiled kernels outlive the process: every code object hiprtc produces is written to a directory, and the FIRST sighting of a
 * program in a later process loads it from there (no compile, no interpreter run) -- the reference's own usage is one evaluation
 * per process (tests/integration_tests.rs:47-49).  Directory: KC_KERNEL_CACHE_DIR, default $XDG_CACHE_HOME/kanter_core_amd or
 * ~/.cache/kanter_core_amd ("off": none); read-only second place: kernel_cache/ next to the library, filled by the build with
 * the BASELINE programs.  A file is trusted only if its signature equals the program's byte for byte, the hash of what TODAY's
 * generator, options and hiprtc version produce for it equals the stored one and the code's checksum holds; anything else is
 * ignored and replaced by a fresh compile.
 *   kc_kernel_cache_set_dir   NULL / "": the environment's choice again; "off": no cache;
 *   kc_kernel_cache_stats     files accepted / refused / written, kernels this process took from files;
 *   kc_kernel_cache_precompile  compiles the program given by value (step words as for kc_specialize_compile_check, cache-policy
 *                             mask, up_taps > 0: the up-sampling form) WITHOUT a device and writes its file into `dir`;
 *   kc_specialize_reset       forgets the kernels this process holds (files stay): the next sighting is a first one. */
KC_API int kc_kernel_cache_set_dir(const char *dir);
KC_API int kc_kernel_cache_stats(uint64_t *files_accepted, uint64_t *files_refused, uint64_t *files_written, uint64_t *kernels_loaded);
KC_API int kc_kernel_cache_precompile(const uint32_t *words, uint32_t n_ops, uint32_t n_in, int start_src, int flat, uint32_t nt_mask,
                                      uint32_t up_taps, int up_wide, const char *dir);
KC_API int kc_specialize_reset(void);
/* The same with packed inputs: in_tiers holds two bits per input plane k (bits 2k, 2k + 1): 0 = f32, 1 = FIX24, 2 = U8
 * (kc_set_pack_sources).  Flat plain chain programs only; in_tiers = 0 is kc_kernel_cache_precompile with up_taps = 0. */
KC_API int kc_kernel_cache_precompile_packed(const uint32_t *words, uint32_t n_ops, uint32_t n_in, int start_src, int flat,
                                             uint32_t nt_mask, uint32_t in_tiers, const char *dir);
/* Lossless packed copies of long-lived chain inputs.  A source embedded in a graph is read again, as f32, by every
 * evaluation, although its values are usually quantised: k * 2^-24 (every uniform-float generator; tier FIX24, 3 bytes per
 * sample) or k / 255.0f (an 8-bit file; tier U8, 1 byte).  The library keeps such a copy beside the f32 plane -- made once, and
 * only if every sample decodes back to its own bit pattern -- and the compiled flat {+, -, *} chain kernels of up to 16
 * records read it instead.  Results are bit-identical; this is a throughput knob only.
 *   kc_set_pack_sources  0: off.  1 (default): a plane is packed at its second sighting as input of a chain launch that does
 *                        not fit the cache budget ("cache_budget_mb") while somebody besides the chain holds it; planes of
 *                        smaller launches never are.  2: every eligible input at its first sighting whatever the size (tests).
 *                        Eligible: planes the library owns, dense, width a multiple of 4; never a wrapped plane, a row-band
 *                        view, or a plane whose pointer kc_plane_device_ptr has handed out.
 *   kc_set_pack_budget_mb  what the packed copies may hold in all (default 4096 MiB); past it nothing more is packed.
 * Counters (kc_stats_counter): "packed_planes", "pack_rejected" (planes that fit no tier), "packed_bytes" (held now),
 * "packed_launches", and "_pk" behind the "specialized_nt_..." name of a launch that read packed inputs. */
KC_API int kc_set_pack_sources(int mode);
KC_API int kc_get_pack_sources(void);
KC_API int kc_set_pack_budget_mb(int mb);
KC_API int kc_get_pack_budget_mb(void);

/* ========================================================================================== *
 * Planes -- replaces Buffer / TransientBufferContainer (src/slot_image.rs:12,
 * src/transient_buffer.rs:188-247); HBM replaces the RAM/disk tiering.
 * ========================================================================================== */
KC_API int kc_plane_alloc(uint32_t width, uint32_t height, kc_plane **out);
/* Broadcast constant: what `vec![v; n]` (src/slot_image.rs:28-64) and the 1x1 Value plane
 * (src/node/mod.rs:240-244) hold, kept as a scalar until somebody needs the bytes. */
KC_API int kc_plane_const(uint32_t width, uint32_t height, float value, kc_plane **out);
/* Wrap caller-owned device memory (e.g. a torch tensor, a view into a larger one, another library's surface); not freed by
 * the library.  device_ptr must be 16-byte aligned and pitch_bytes a multiple of 16, at least 16 * ceil(width / 4); nothing
 * more is assumed of either (no 32-, 64- or 256-byte row starts, no pitch equal to the pool's), else KC_ERR_INVALID_ARG.
 * What the library may READ through the plane: for each row y in [0, height) the 16 * ceil(width / 4) bytes from
 * device_ptr + y * pitch_bytes -- the row's pixels and the tail of its last quad of four floats -- and nothing else: not
 * the rest of the padding between rows, not the bytes before the first row or after the last.  The up to three floats of a
 * last quad's tail may be loaded but never reach a pixel, whatever they hold (NaN, infinities).  The library never WRITES
 * there: every operation on a wrapped plane puts its result into planes of its own.  The memory must stay valid and
 * unchanged until the work that reads it is done (kc_sync) and the plane is released.  tests/test_gpu_wrapped_planes.py runs
 * every plane-reading kernel on such planes inside guard-filled tensors. */
KC_API int kc_plane_wrap(void *device_ptr, uint32_t width, uint32_t height, size_t pitch_bytes, kc_plane **out);
KC_API int kc_plane_retain(kc_plane *p);
KC_API int kc_plane_release(kc_plane *p);
KC_API int kc_plane_size(const kc_plane *p, uint32_t *width, uint32_t *height);
KC_API int kc_plane_is_const(const kc_plane *p, int *is_const, float *value);
/* Forces the plane into HBM (runs any pending fused chain, fills constants). */
KC_API int kc_plane_materialize(kc_plane *p);
/* Materialises, then returns the device pointer and pitch (valid while the plane is retained). */
KC_API int kc_plane_device_ptr(kc_plane *p, void **device_ptr, size_t *pitch_bytes);
KC_API int kc_plane_upload_f32(kc_plane *p, const float *host, size_t host_pitch_bytes);
KC_API int kc_plane_download_f32(kc_plane *p, float *host, size_t host_pitch_bytes);

/* ========================================================================================== *
 * Images -- SlotImage, src/slot_image.rs:15-264
 * ========================================================================================== */
KC_API int kc_image_gray(kc_plane *p, kc_image **out);                 /* SlotImage::Gray */
KC_API int kc_image_rgba(kc_plane *const planes[4], kc_image **out);   /* SlotImage::Rgba */
KC_API int kc_image_retain(kc_image *img);
KC_API int kc_image_release(kc_image *img);
KC_API int kc_image_is_rgba(const kc_image *img, int *is_rgba);        /* slot_image.rs:123-139 */
KC_API int kc_image_size(const kc_image *img, kc_size *size);          /* slot_image.rs:116-121 */
KC_API int kc_image_plane(const kc_image *img, int channel, kc_plane **out); /* +1 reference */
KC_API int kc_image_from_value(kc_size size, float value, int rgba, kc_image **out); /* :28-64 */
KC_API int kc_image_as_type(const kc_image *img, int rgba, kc_image **out);          /* :212-256 */
KC_API int kc_image_materialize(kc_image *img);
/* deconstruct_image + read_slot_image, src/shared.rs:16-56,218-261: interleaved u8 with 1..4
 * channels -> RGBA planes (/255., missing R,G,B = 0, A = 1). */
KC_API int kc_image_from_u8(const uint8_t *host, uint32_t width, uint32_t height, int channels, kc_image **out);
/* to_u8 / to_u8_srgb, src/slot_image.rs:141-207: -> interleaved RGBA8 (width*height*4 bytes). */
KC_API int kc_image_to_u8(kc_image *img, int srgb, uint8_t *host_rgba8);
/* The same two as a PIPELINE for jobs that run one graph over many images: `depth` slots, each with a pinned host buffer for an
 * input image (width * height * channels bytes), one for an RGBA8 output image, and device staging for both; the copies run on
 * two streams of the pipe's own, ordered with the compute stream by events, so the upload of image k + 1 and the download of
 * image k - 1 overlap the evaluation of image k and no call waits on the host except kc_u8_pipe_wait_download.
 *   kc_u8_pipe_buffers        the slot's buffers: fill `*host_in` before kc_u8_pipe_upload, read `*host_out` after
 *                             kc_u8_pipe_wait_download (and before the slot's next kc_u8_pipe_download);
 *   kc_u8_pipe_upload         deconstruct_image of the slot's input buffer: `*out` (+1 ref) is usable at once (its planes are
 *                             ready in stream order).  Call it for the NEXT image after the current one's evaluation has been
 *                             enqueued -- the copy then runs during that evaluation;
 *   kc_u8_pipe_download       to_u8 (srgb = 0) / to_u8_srgb (1) of `img` into the slot's output buffer, asynchronously;
 *   kc_u8_pipe_wait_download  blocks until that buffer holds the image. */
KC_API int kc_u8_pipe_create(uint32_t width, uint32_t height, int channels, int depth, kc_u8_pipe **out);
KC_API int kc_u8_pipe_free(kc_u8_pipe *pipe);
KC_API int kc_u8_pipe_buffers(kc_u8_pipe *pipe, int slot, uint8_t **host_in, const uint8_t **host_out);
KC_API int kc_u8_pipe_upload(kc_u8_pipe *pipe, int slot, kc_image **out);
KC_API int kc_u8_pipe_download(kc_u8_pipe *pipe, int slot, kc_image *img, int srgb);
KC_API int kc_u8_pipe_wait_download(kc_u8_pipe *pipe, int slot);
KC_API int kc_image_from_f32(const float *const host_planes[], int n_planes, uint32_t width, uint32_t height, kc_image **out);
KC_API int kc_image_to_f32(kc_image *img, float *const host_planes[], int n_planes);
/* Images in DEVICE memory (a torch tensor, a renderer's buffer, the input of the next graph): converted on the device, no
 * trip through host memory.  kc_plane_wrap borrows a single aligned f32 plane without a copy; these entries convert from and
 * to the common element types and layouts, into library-owned planes / caller memory.
 *   kc_device_image      a caller's buffer: `ptr` is device memory of the library's device; element (x, y, channel c) lies at
 *                        ptr + y * row_pitch_bytes + (x * channels + c) * elem (INTERLEAVED, HWC) or
 *                        ptr + c * channel_pitch_bytes + y * row_pitch_bytes + x * elem (PLANAR, CHW).
 *   kc_device_image_validate  launches nothing.  Arithmetic checks first (no kc_init needed): channels 1..4, known dtype and
 *                        layout, width and height > 0, ptr and the pitches multiples of the element size, row pitch >= the row's
 *                        bytes, PLANAR planes that do not overlap (channel pitch >= height * row pitch, when channels > 1); a
 *                        failure is KC_ERR_INVALID_ARG.  Then `*extent_bytes` (optional) = end of the last element - ptr.  Once
 *                        initialised, [ptr, ptr + extent) must lie in ONE device allocation of the library's device
 *                        (KC_ERR_INVALID_ARG otherwise, e.g. a host pointer); before kc_init the call returns KC_ERR_NO_DEVICE
 *                        after the arithmetic, with the extent written.  The three entries below call it first.
 *   kc_image_from_device deconstruct_image (src/shared.rs:16-56) on the device: U8 v / 255., U16 v / 65535., F16 / BF16 exact
 *                        widening, F32 the bits as they are; an RGBA image with missing R, G, B = 0 and a missing A = 1 --
 *                        or, with KC_DEVICE_GRAY and channels == 1, a Gray image.  `*out` (+1 ref) owns copies of the pixels.
 *   kc_image_to_device   channel c (0..3) of `dst` = R, G, B, A of the image as to_u8 sees it (Gray = (v, v, v, 1)): U8
 *                        exactly what kc_image_to_u8 writes (KC_DEVICE_SRGB: to_u8_srgb; another dtype with it is
 *                        KC_ERR_UNSUPPORTED), U16 ((v.clamp(0,1) * 65535.).min(65535.)) truncated (NaN -> 65535), F16 / BF16
 *                        round to nearest even (no clamp), F32 the bits.  Bytes outside the described elements are not touched.
 *   kc_live_graph_buffer_device  the same for a slot's image (buffer_rgba, src/live_graph.rs:93-95).
 * Ordering: the conversion is enqueued on the library's stream (kc_get_stream) and the calls return without waiting.  With a
 * non-NULL `hip_stream` the library's stream first waits for the work already enqueued on `hip_stream`, and `hip_stream` then
 * waits for the conversion; kc_set_stream is not changed.  NULL orders nothing: a caller on HIP's legacy NULL stream makes the
 * two edges itself against kc_get_stream() (the Python binding does so for torch's default stream).  The caller's buffer may be overwritten or freed by work ordered
 * after the conversion: on `hip_stream` after the call returns, or after kc_sync. */
typedef enum kc_dtype { KC_DTYPE_U8 = 0, KC_DTYPE_U16 = 1, KC_DTYPE_F16 = 2, KC_DTYPE_BF16 = 3, KC_DTYPE_F32 = 4 } kc_dtype;
typedef enum kc_layout { KC_LAYOUT_INTERLEAVED = 0 /* HWC */, KC_LAYOUT_PLANAR = 1 /* CHW */ } kc_layout;
typedef struct kc_device_image {
    void *ptr;                    /* device memory on the library's device */
    uint32_t width, height;
    int32_t channels;             /* 1..4 */
    int32_t dtype, layout;        /* kc_dtype, kc_layout */
    size_t row_pitch_bytes;       /* distance between rows */
    size_t channel_pitch_bytes;   /* PLANAR only: distance between channel planes; ignored for INTERLEAVED */
} kc_device_image;
#define KC_DEVICE_SRGB 1u /* export, U8 only: to_u8_srgb on R, G, B (alpha stays linear), as kc_image_to_u8 */
#define KC_DEVICE_GRAY 2u /* import, channels == 1 only: a Gray image instead of the RGBA rule */
KC_API int kc_device_image_validate(const kc_device_image *d, size_t *extent_bytes);
KC_API int kc_image_from_device(const kc_device_image *src, uint32_t flags, void *hip_stream, kc_image **out);
KC_API int kc_image_to_device(kc_image *img, const kc_device_image *dst, uint32_t flags, void *hip_stream);
/* Per-channel statistics of an image, computed on the device: the value range and NaN count of every channel and, on request,
 * the histogram of the 8-bit export -- without downloading the pixels (an editor's levels view, a range check before a u8
 * export).  Not a node: a query like kc_image_to_device.
 *   min / max     over the channel's non-NaN pixels in the total order of the floats: -0.0 < +0.0, infinities included,
 *                 denormals as they are (compared through the key k = bits >> 31 ? ~bits : bits | 0x80000000, not fminf);
 *                 NaN when the channel has no such pixel, and for channels >= `channels`.
 *   nan_count     the channel's NaN pixels (any payload, either sign); 0 for channels >= `channels`.
 *   histogram     with KC_STATS_HISTOGRAM: histogram[c][b] = the pixels that kc_image_to_u8 writes as b in channel c (the
 *                 same quantiser functions); with KC_STATS_SRGB as well, as kc_image_to_u8 with srgb = 1 writes them: R, G, B of
 *                 an RGBA image and the channel of a Gray image through to_u8_srgb, alpha linear.  Only the first `channels`
 *                 rows are filled; all zero without the flag.
 * `channels` is the image's own (1 Gray, 4 RGBA), not to_u8's (v, v, v, 1).  Bytes of a plane's rows past `width` (the
 * padding kc_plane_wrap allows) are never read as pixels.  Errors: NULL img / lg / out KC_ERR_INVALID_ARG; flag bits other
 * than the two KC_ERR_UNSUPPORTED; KC_STATS_SRGB without KC_STATS_HISTOGRAM KC_ERR_INVALID_ARG; then KC_ERR_NO_DEVICE before
 * kc_init.  kc_live_graph_buffer_channel_stats returns KC_ERR_NO_SLOT_DATA where kc_live_graph_buffer_device does.  `*out` is
 * written on KC_OK only.
 * The call runs after the work already enqueued on the library's stream and blocks until the host values are there (an event of
 * its own; other streams are not waited for).  A pending chain or resample is run first.  A constant channel is answered on the
 * host; the distinct resident planes are read once, by one launch plus a small combining launch (kc_stats: two launches,
 * width * height * 4 algorithmic bytes per plane read); an image of constant channels launches nothing. */
#define KC_STATS_HISTOGRAM 1u /* also fill histogram[][] */
#define KC_STATS_SRGB 2u      /* histogram bins as to_u8_srgb assigns them (R, G, B; alpha linear); needs KC_STATS_HISTOGRAM */
typedef struct kc_channel_stats {
    uint32_t channels;          /* 1: Gray, 4: Rgba -- the image's own channels, not to_u8's (v, v, v, 1) */
    uint32_t flags;             /* the flags the call was given */
    uint64_t pixels;            /* width * height */
    float min[4], max[4];       /* over the non-NaN pixels; NaN when a channel has none; NaN for channels >= `channels` */
    uint64_t nan_count[4];
    uint64_t histogram[4][256]; /* KC_STATS_HISTOGRAM: histogram[c][b] = #pixels that kc_image_to_u8 (or _srgb) writes as b in
                                   channel c; all zero without the flag */
} kc_channel_stats;
KC_API int kc_image_channel_stats(kc_image *img, uint32_t flags, kc_channel_stats *out);
/* Block-compressed textures, encoded on the device: BC1 (colour), BC3 (colour and alpha), BC4 (one channel), BC5 (two
 * channels), BC7 (colour and alpha at 8 bits an endpoint) and BC6H (HDR colour as half floats, see its paragraph), the formats
 * a GPU samples.  BC6H apart, the blocks are a function of the RGBA8 bytes kc_image_to_u8(img, srgb) writes (Gray =
 * (v, v, v, 1); KC_BC_SRGB: R, G, B as with srgb = 1, alpha always linear); everything after that quantisation is integer
 * arithmetic, so the output is bit-exact.  The grid is bx = ceil(w / 4) by by = ceil(h / 4) blocks; texel t = 4y + x (x, y in
 * 0..3) of block (i, j) is pixel (min(4i + x, w - 1), min(4j + y, h - 1)): edge blocks repeat the last column or row.
 *   BC4 of values v_t: e0 = max, e1 = min, d = e0 - e1.  d == 0: bytes e0, e1, then six zero bytes.  Otherwise the ramp
 *           position r = floor((14 (v - e1) + d) / (2 d)) (0..7) gives the index 0 for r == 7, 1 for r == 0 and 8 - r otherwise.
 *           Bytes: e0, e1, then a 48-bit little-endian word with texel t's index at bits 3t..3t+2.
 *   BC1 of texels p_t = (r, g, b): per channel lo = min, hi = max; the reference channel k has the largest hi - lo (ties: R, then
 *           G, then B); s_c = sum_t (2 p_t,k - lo_k - hi_k)(2 p_t,c - lo_c - hi_c).  a_c = hi_c - m_c, b_c = lo_c + m_c with
 *           m_c = (hi_c - lo_c) >> 4, swapped where s_c < 0 (the colour box's anti-diagonal).  c0 = pack(a), c1 = pack(b),
 *           pack = q5(R) << 11 | q6(G) << 5 | q5(B), q5(x) = (31x + 127) div 255, q6(x) = (63x + 127) div 255; swapped when
 *           c0 < c1.  E(c) expands by bit replication; the scaled palette is P0 = 3E(c0), P1 = 3E(c1), P2 = 2E(c0) + E(c1),
 *           P3 = E(c0) + 2E(c1).  c0 == c1: every index 0; otherwise texel t's index is the j minimising
 *           sum_c (3 p_t,c - P_j,c)^2, the lowest j on a tie.  Bytes: c0 and c1 as u16 LE, then a u32 LE with texel t's index at
 *           bits 2t..2t+1.  A block with a non-zero index has c0 > c1: it decodes in four-colour mode, never transparent.
 *   BC1 with punch-through alpha (KC_BC_PUNCH_THROUGH, BC1 only): the format of alpha-TESTED cutouts at 8 bytes a block, its
 *           1-bit alpha exactly the bit the test keeps.  The reference byte B, 1..255, travels in bits 24-31 of the flags word,
 *           KC_BC_PUNCH_THROUGH_REF(B): the field of KC_MIP_COVERAGE_REF, which the two flags share in one word --
 *           KC_BC_PUNCH_THROUGH | KC_MIP_COVERAGE_REF(B) builds the chain that keeps coverage at B and cuts every level at B.
 *           The texels are kc_image_to_u8's bytes with alpha (always linear; edge blocks repeat the last column and row, alpha
 *           included).  Texel t is opaque when its alpha byte is >= B: KC_MIP_COVERAGE's "covered" exactly (NaN alpha
 *           quantises to 255 and is opaque).  n = the opaque texels of the block.  All integer arithmetic, so bit-exact
 *           (tests/bc1a_ref.py is the same rule in numpy; kc_bc1_punch_through_block is the rule on one block, no device).
 *             n == 16:     the plain BC1 block above, bit for bit.
 *             n == 0:      the bytes 00 00 00 00 FF FF FF FF: c0 = c1 = 0, every index 3.
 *             0 < n < 16:  lo, hi, k and s_c as for BC1 -- the same formulas and tie order -- with every min, max and sum over the
 *                          opaque texels only.  m_c = (hi_c - lo_c) >> 3: twice the four-colour inset, because a three-colour
 *                          palette has one interior point and its ends sit further in (a fixed part of the rule).  a_c = hi_c -
 *                          m_c, b_c = lo_c + m_c, swapped where s_c < 0; c0 = pack(a), c1 = pack(b), swapped when c0 > c1: the
 *                          block has c0 <= c1 and decodes in three-colour mode (c0 == c1 is legal).  The palette is the
 *                          decoder's: Q0 = E(c0), Q1 = E(c1), Q2 = (E(c0) + E(c1)) div 2 per channel.  An opaque texel takes the
 *                          j in 0..2 minimising sum_c (p_c - Q_j,c)^2, the lowest j on a tie; a texel that is not opaque takes
 *                          index 3.  The byte layout is BC1's.
 *           So a decoded texel has alpha 0 exactly where the source texel is not opaque; the colour under such texels never
 *           influences a block; and an image whose alpha is everywhere >= B gives plain BC1, bit for bit.  The file is an
 *           ordinary BC1 file (dxgiFormat 71 / 72): kc_dds_header, like kc_image_build_mips, kc_image_build_roughness_mips, the
 *           previews and the decode entry points, refuses the flag as an unknown bit, and kc_image_from_bc / kc_image_read_dds
 *           return such blocks with alpha 0 or 1 as they always have.  Accepted by kc_image_to_bc, kc_image_to_bc_device,
 *           kc_live_graph_buffer_bc; kc_image_bc_error, kc_live_graph_buffer_bc_error, kc_image_bc_compare;
 *           kc_image_to_bc_mips, kc_image_to_bc_mips_device, kc_live_graph_buffer_bc_mips; kc_image_levels_to_bc_mips,
 *           kc_image_write_dds, kc_image_levels_write_dds.  It combines with KC_BC_SRGB, KC_MIP_PER_LEVEL, KC_MIP_COVERAGE and
 *           KC_MIP_ALPHA_WEIGHT.  KC_ERR_UNSUPPORTED, refused with the other flag errors (before NULL arguments and kc_init):
 *           the flag with a format other than KC_BC1, with a zero byte or with KC_MIP_NORMALS; a byte with neither this flag nor
 *           KC_MIP_COVERAGE (as ever).  A Gray image is KC_ERR_INVALID_ARG exactly where KC_MIP_COVERAGE refuses it.
 *           The error measure under the flag (kc_bc_error keeps its layout): channel_mask is 0xF; the source alpha is 255 where
 *           the source texel is opaque and 0 otherwise, and sse[3] / max_abs[3] compare the decoded alpha against that; a pixel
 *           whose source texel is not opaque contributes 0 to R, G and B (the renderer discards it, and its decoded colour is
 *           the format's black); `pixels` stays width * height.  kc_stats: the encode is one launch, with 4 w h algorithmic
 *           bytes per distinct resident plane of R, G, B and A plus the blocks' bytes (a constant alpha costs no loads); the
 *           comparison stays two launches.
 *   BC3     the BC4 block of alpha, then the BC1 block (16 bytes).  BC5: the BC4 block of R, then that of G (16 bytes).  BC1
 *           ignores alpha (without KC_BC_PUNCH_THROUGH); BC4 reads R only, BC5 R and G.
 *   BC7 of texels p_t = (r, g, b, a), 16 bytes: the two single-subset modes 6 and 5 (rotation 0) only.
 *           interp(e0, e1, w) = ((64 - w) e0 + w e1 + 32) >> 6; W4 = 0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64;
 *           W2 = 0, 21, 43, 64.  axis(p over channels C): per channel lo = min, hi = max; k the first channel (order R, G, B, A)
 *           of the largest hi - lo; a_t = 2 p_t,k - lo_k - hi_k; s_c = sum_t a_t (2 p_t,c - lo_c - hi_c); e0_c = hi_c if
 *           s_c < 0 else lo_c, e1_c the other one (BC1's covariance-sign diagonal, without the inset).  An index is the arg-min
 *           of the squared distance summed over the channels of its palette, the lowest index on a tie; a mode's error is the
 *           sum of those minima.
 *           Mode 6: (e0, e1) = axis(p over R, G, B, A).  Each endpoint on its own: for pb in 0, 1,
 *           q_c = clamp((e_c - pb + 1) >> 1, 0, 127), v_c = 2 q_c + pb, cost sum_c (v_c - e_c)^2; pb = 1 only if its cost is
 *           strictly lower.  Palette i = interp(v0, v1, W4[i]) per channel.  If texel 0's index is >= 8 the endpoints swap
 *           together with their p-bits and every index becomes 15 - index (the weights are symmetric).
 *           Mode 5: (e0, e1) = axis(p over R, G, B); q_c = (127 e_c + 127) div 255 decodes to v_c = (q_c << 1) | (q_c >> 6);
 *           colour palette interp(v0, v1, W2[i]); alpha endpoints a0 = min, a1 = max, palette interp(a0, a1, W2[i]); err5 = the
 *           colour error plus the alpha error.  The two index sets are anchored independently: a texel-0 index >= 2 swaps that
 *           set's endpoints and turns its indices into 3 - index.
 *           Mode 5 if and only if err5 < err6.  Bit n of the block is bit n % 8 of byte n / 8; fields are LSB first.
 *           Mode 6: bits 0-6 the value 64; R0, R1, G0, G1, B0, B1, A0, A1 of 7 bits each (7-62); P0 bit 63, P1 bit 64; texel 0's
 *           index in 3 bits (65-67), texels 1-15 in 4 bits each (68-127).  Mode 5: bits 0-5 the value 32; rotation (6-7) 0; R0,
 *           R1, G0, G1, B0, B1 of 7 bits each (8-49); A0, A1 of 8 bits each (50-65); colour indices, texel 0 in 1 bit (66),
 *           texels 1-15 in 2 bits each (67-96); alpha indices likewise (97, 98-127).
 *   BC6H (KC_BC6H, unsigned, DXGI_FORMAT_BC6H_UF16), 16 bytes: the HDR format, sampled as half floats.  It does NOT start from
 *           kc_image_to_u8's bytes: a plane value v is quantised to h(v) = f16(min(max(v, 0), 65504)) as a 16-bit pattern,
 *           rounded to nearest even, denormal halves kept; NaN, the negatives, -0 and -inf give 0, +inf and everything >= 65504
 *           give 0x7BFF.  Texels are p_t = (h(R), h(G), h(B)), integers 0..31743 (Gray: (v, v, v)); alpha is never read; nothing
 *           is clamped to 1.  After that everything is integer arithmetic on the patterns (tests/bc6h_ref.py is the same rules
 *           in numpy).  unq10(q) = 0 for q = 0, 0xFFFF for q = 1023, else 64 q + 32; fin(x) = (31 x) >> 6; E(q) = fin(unq10(q)).
 *           Only mode 11 is written (one subset, 10-bit endpoints).  (e0, e1) = axis(p over R, G, B) as for BC7, the sums s_c in
 *           64 bits.  Each endpoint channel is the smallest q in 0..1023 minimising |E(q) - e|.  Palette i =
 *           fin(interp(unq10(q0), unq10(q1), W4[i])) per channel; texel t takes the i minimising sum_c (p_t,c - P_i,c)^2, the
 *           lowest i on a tie.  If texel 0's index is >= 8 the endpoints swap and every index becomes 15 - index.  Bits 0-4
 *           the value 3; R0, G0, B0 of 10 bits each (5-34); R1, G1, B1 (35-64); texel 0's index in 3 bits (65-67), texels 1-15
 *           in 4 bits each (68-127).  KC_BC_SRGB with KC_BC6H is KC_ERR_UNSUPPORTED.
 *   kc_bc_image           a caller's buffer of blocks: block (i, j) at ptr + j * row_pitch_bytes + i * block bytes.
 *   kc_bc_image_validate  launches nothing; like kc_device_image_validate.  Arithmetic first (no kc_init needed): a known
 *                         format, width and height > 0, bx * by <= 2^31, ptr and row_pitch_bytes multiples of the block
 *                         bytes, row pitch >= bx * block bytes, no overflow; a failure is KC_ERR_INVALID_ARG.  Then
 *                         `*extent_bytes` (optional) = (by - 1) * row_pitch_bytes + bx * block bytes.  Once initialised, the
 *                         extent must lie in ONE device allocation of the library's device (KC_ERR_INVALID_ARG otherwise);
 *                         before kc_init the call returns KC_ERR_NO_DEVICE after the arithmetic, with the extent written.
 *   kc_image_to_bc        blocks into host memory, tightly packed rows (bx * by * block bytes; `host_bytes` at least that).
 *                         Blocks until they are there, as kc_image_to_u8.
 *   kc_image_to_bc_device blocks into `dst`, ordered against `hip_stream` by the two event edges of kc_image_to_device (the
 *                         host does not wait).  kc_live_graph_buffer_bc: the same for a slot's image.
 * Errors: flag bits other than KC_BC_SRGB and KC_BC_PUNCH_THROUGH_REF, KC_BC_SRGB with BC4 / BC5 / BC6H, or
 * KC_BC_PUNCH_THROUGH against its rule above, KC_ERR_UNSUPPORTED; a NULL argument, an unknown
 * format, a descriptor size that differs from the image's or `host_bytes` below the blocks' bytes KC_ERR_INVALID_ARG; then
 * KC_ERR_NO_DEVICE before kc_init; kc_live_graph_buffer_bc returns KC_ERR_NO_SLOT_DATA where kc_live_graph_buffer_device does.
 * A refused call launches nothing.  A pending chain or resample runs first; then one launch (kc_stats), constant channels
 * included, with width * height * 4 algorithmic bytes per distinct resident plane the format reads plus the blocks' bytes.
 * Bytes outside the blocks are never written.
 * KC_BC7 is 98, DXGI_FORMAT_BC7_UNORM's own number, not 7: the value 7 has always been refused as an unknown format and stays
 * refused.  KC_BC6H is 95, DXGI_FORMAT_BC6H_UF16's number, likewise; 6 and the signed form's 96 are refused. */
typedef enum kc_bc_format { KC_BC1 = 1, KC_BC3 = 3, KC_BC4 = 4, KC_BC5 = 5, KC_BC6H = 95, KC_BC7 = 98 } kc_bc_format;
typedef struct kc_bc_image {
    void *ptr;               /* device memory of the library's device */
    uint32_t width, height;  /* the image's pixels */
    int32_t format;          /* kc_bc_format; block bytes 8 (BC1, BC4) or 16 (BC3, BC5, BC6H, BC7) */
    size_t row_pitch_bytes;  /* distance between block rows */
} kc_bc_image;
#define KC_BC_SRGB 1u        /* BC1 / BC3 / BC7: R, G, B as kc_image_to_u8 with srgb = 1 writes them; alpha linear */
#define KC_BC_PUNCH_THROUGH 256u  /* BC1 only: texels whose alpha byte is below the byte in bits 24-31 decode transparent (above) */
#define KC_BC_PUNCH_THROUGH_REF(b) (256u | ((uint32_t)(b) << 24))  /* KC_BC_PUNCH_THROUGH with the reference byte b, 1..255 */
KC_API int kc_bc_image_validate(const kc_bc_image *d, size_t *extent_bytes);
/* The punch-through rule on one block, without a device: texel t is rgba + 4 t, ref_u8 the reference byte B.  A NULL pointer or
 * a byte outside 1..255 is KC_ERR_INVALID_ARG and nothing is written. */
KC_API int kc_bc1_punch_through_block(const uint8_t rgba[64], uint32_t ref_u8, uint8_t block[8]);
KC_API int kc_image_to_bc(kc_image *img, int format, uint32_t flags, uint8_t *host, size_t host_bytes);
KC_API int kc_image_to_bc_device(kc_image *img, const kc_bc_image *dst, uint32_t flags, void *hip_stream);
/* Mip chains, built on the device, and their export as BC textures and DDS files: what a renderer samples is a chain, not one
 * level.  The rule is f32 throughout and bit-exact (tests/mip_ref.py is the same rule in numpy).
 *   Levels.   Level 0 is the image; level k is max(1, w >> k) by max(1, h >> k); there are L = 1 + floor(log2(max(w, h)))
 *             levels, the last 1 x 1.
 *   A texel.  For a level made from the source level s of size (w, h), every plane on its own:
 *                 x0 = 2x, x1 = min(2x + 1, w - 1), y0 = 2y, y1 = min(2y + 1, h - 1)
 *                 d(x, y) = ((s(x0, y0) + s(x1, y0)) + (s(x0, y1) + s(x1, y1))) * 0.25f
 *             three f32 additions in exactly that order and one multiplication.  Nothing is fused, denormals are kept, nothing
 *             is clamped; NaN and the infinities follow IEEE (inf + -inf = NaN; a source of only -0.0 gives -0.0); NaN payload
 *             and sign are not part of the contract.  x1 and y1 clamp only when that extent of the source is already 1.  With
 *             an odd source extent the last column or row does not contribute: this is the usual 2 x 2 box, not a filter over
 *             the whole footprint -- kc_resize_image is the filtered minification of odd sizes.
 *   Level k depends only on level k - 1 as stored: each level is rounded to f32 before the next is made, so the fused kernel
 *             (up to six levels per launch from one read of a 64 x 64 tile) and the level-by-level one give the same bits.
 *   Planes.   A constant plane stays a constant plane at every level, its value the same expression in f32 on the host,
 *             ((c + c) + (c + c)) * 0.25f once per level (not c for very large or denormal c).  Planes that alias
 *             (kc_image_as_type's [p, p, p, ones]) are reduced once and the level images alias the same way.  Pending chains and
 *             deferred resizes run first.  Planes are linear f32 and sRGB is applied at export (KC_BC_SRGB, kc_image_to_u8 with
 *             srgb), so the average is taken in linear light.
 *   Normal maps (KC_MIP_NORMALS).  The box of four unit vectors is shorter than 1, and a renderer that rebuilds Z from a BC5
 *             texel as sqrt(1 - x^2 - y^2) reads the shortened XY pair as a flatter surface at every coarser level.  With the
 *             flag, an RGBA image is a normal map: X, Y, Z are R, G, B stored as n * 0.5 + 0.5 (what kc_height_to_normal_process
 *             writes), and every level is renormalised on the device before the next is made (tests/mip_normals_ref.py is the
 *             same rule in numpy).  Level 0 is the image itself, untouched.  Level k >= 1 is made from level k - 1 as stored;
 *             per texel, with b_c the plain rule's box of channel c (the same expression, order and clamps), c over R, G, B:
 *                 v_c = b_c * 2.0f - 1.0f                      one multiplication, one subtraction, nothing fused
 *                 q = (v_x * v_x + v_y * v_y) + v_z * v_z,  l = sqrtf(q)    correctly rounded
 *                 u_c = v_c / l (IEEE divide) if l > 0 && l < +inf, else u = (0, 0, 1)
 *                 d_c = u_c * 0.5f + 0.5f
 *             The comparison is false for NaN: a zero vector, an underflowed or overflowed q and a NaN or infinity in any of
 *             the three channels all store exactly (0.5, 0.5, 1.0), so R, G, B of levels >= 1 never hold a NaN (NaN payloads
 *             do not enter the contract).  Denormals are kept.  Alpha follows the plain rule unchanged, constant or resident.
 *             Each level is normalised and rounded to f32 before the next is made, so the fused form and KC_MIP_PER_LEVEL give
 *             the same bits.  Planes: if R, G and B are all constant, levels >= 1 are constant planes, folded on the host with
 *             the same expression (kc_mip_normal_texel of the three folded boxes) and nothing is launched for them; if at least
 *             one is resident, every level >= 1 has three new resident planes for R, G, B -- a constant channel enters the first
 *             level as its value (its box is ((c + c) + (c + c)) * 0.25f), aliased channels are read once and written three
 *             times.  kc_stats: the same launches as the plain chain of the three planes (counters "mip_normals_pyramid",
 *             "mip_normals_level"; a resident alpha is reduced by launches of its own under "mip_pyramid" / "mip_level"), so a
 *             kc_height_to_normal_process result takes as many launches as its plain chain; 4 w h algorithmic bytes per
 *             distinct resident plane among R, G, B read plus 12 sum_{k >= 1} W_k H_k written, plus alpha's by the plain rule.
 *             Accepted by kc_image_build_mips, kc_image_to_bc_mips, kc_image_to_bc_mips_device, kc_live_graph_buffer_bc_mips
 *             and kc_image_write_dds (without mips it has no effect); any BC format (BC5 is the point; BC4 reads R alone).
 *             With KC_BC_SRGB it is KC_ERR_UNSUPPORTED (a vector is not a colour), refused with the other flag errors; a Gray
 *             image is KC_ERR_INVALID_ARG, after KC_ERR_NO_DEVICE, with nothing launched or allocated (`*count` is written).
 *             kc_dds_header refuses the flag: the header does not depend on it.  Previews stay defined by the plain rule.
 *   Alpha-tested textures (KC_MIP_COVERAGE).  Foliage, fences and hair cards are cutouts: a renderer discards a texel whose
 *             alpha byte is below a reference B.  The box pulls alpha towards the middle, so thin features fall under B and the
 *             object thins out with distance.  With the flag every level's alpha is rescaled so that the share of texels that
 *             pass the test stays what it was at level 0 (tests/mip_coverage_ref.py is the same rule in numpy).  Everything is
 *             f32 or integer and bit-exact.  B, 1..255, travels in bits 24-31 of the flags word: KC_MIP_COVERAGE_REF(B).
 *               Covered.  A texel with alpha a is covered when quant_u8(a) >= B, kc_image_to_u8's linear quantiser (clamp,
 *                         * 255.0f, truncate, NaN -> 255); equivalently clamp01(a) >= r_B, r_B = (float)B / 255.0f (one IEEE
 *                         divide; kc_alpha_ref_threshold): the smallest f32 that quantises to at least B.
 *               Key.      key(a) = a clamped to [0, 1], NaN -> 1.0f, -0.0 and anything not greater than 0 -> +0.0f.
 *               Level k >= 1.  N_k its texels, p_k the plain rule's alpha (always made from the unscaled p_{k-1}: the scaling never
 *                         compounds), C_0 the covered texels of level 0, P_k those of p_k;
 *                         T_k = 0 if C_0 == 0, else min(N_k, max(1, (C_0 * N_k + N_0 / 2) / N_0)) in integers
 *                         (kc_mip_coverage_target).  If T_k == 0 or P_k == T_k the level keeps the plain alpha bit for bit
 *                         (s_k = 1.0f): a fully opaque or fully empty texture never changes.  Otherwise v_k = the T_k-th largest
 *                         key of the level, ve = max(v_k, 0x1p-16f) (alpha below one step of a 16-bit export counts as empty, which
 *                         keeps s finite), s_k = r_B / ve (IEEE divide), and while quant_u8(ve * s_k) < B, s_k is the next f32
 *                         above it (kc_mip_coverage_scale; the loop is the definition).  The stored alpha is d = p * s_k: one f32
 *                         multiplication, nothing clamped; NaN stays NaN, zeros stay zeros, infinities follow IEEE.
 *                         Whenever s_k != 1 and v_k >= 2^-16 the covered texels C_k of the stored level satisfy
 *                         T_k <= C_k <= #{key(p_k) >= v_k * (1 - 2^-20)}: ties, plus the texels within a few ulps below v_k.
 *             Planes: the flag is for RGBA images; a Gray image is KC_ERR_INVALID_ARG exactly where KC_MIP_NORMALS refuses it.  R,
 *             G, B follow the plain rule, or the normals rule with KC_MIP_NORMALS (the two combine); KC_MIP_PER_LEVEL gives the
 *             same bits.  A constant alpha is left as the plain rule leaves it and launches nothing.  A resident alpha gets a new
 *             plane of its own at every level >= 1, also where it aliases R, G or B at level 0: the shared plain plane is never
 *             scaled.  Level 0 is the image itself.  Images of more than 2^31 texels are KC_ERR_INVALID_ARG ("image too large").
 *             Bits 24-31 without KC_MIP_COVERAGE, or KC_MIP_COVERAGE with B == 0, are KC_ERR_UNSUPPORTED, refused with the other
 *             flag errors.  Accepted by the entry points that accept KC_MIP_NORMALS; kc_dds_header refuses it; previews stay
 *             defined by the plain rule.  On the device the T_k-th largest key is an exact radix select over integer counts (three
 *             passes of 10 key bits over all levels at once), so no bit depends on the launch shape.  kc_stats: seven launches
 *             on top of the plain chain's whatever the level count (three counts, three picks, one scale, behind one
 *             hipMemsetAsync that zeroes the scratch; none for a 1 x 1 image or a constant alpha; counter "mip_coverage" counts
 *             them), and 4 N_0 + 20 sum_{k >= 1} N_k algorithmic bytes:
 *             level 0's alpha read once, every further level once per pass and once for the scale, and written once.  The
 *             scratch comes from the pool and goes back to it; the call still does not wait.
 *   Alpha-weighted colour (KC_MIP_ALPHA_WEIGHT).  The plain rule boxes R, G, B without regard to alpha, so whatever colour lies
 *             under the transparent texels of a cutout (black, magenta, what the graph left there) is averaged into the edge
 *             texels of every coarser level: a halo that grows with distance, and at level 0 block endpoints and bilinear taps
 *             spent on a colour nobody should see.  With the flag the colour of every level is the alpha-weighted average of
 *             the texels under it, and the texels that have none are filled from the coarser levels (pull-push;
 *             tests/mip_alpha_ref.py is the same rule in numpy).  Everything is f32, nothing is fused, denormals are kept, / is
 *             the correctly rounded divide.  Inputs: an RGBA image, colour c = (R, G, B), alpha a.
 *               Weight.   w0 = a > 0 ? min(a, 1.0f) : 0.0f                                  (kc_mip_alpha_weight)
 *                         The comparison is false for NaN: NaN, -0.0 and negatives give +0.0.
 *               Premultiplied level 0.  p_c = w0 > 0 ? c * w0 : 0.0f: a select, not a product, so a NaN or an infinity under a
 *                         transparent texel never enters.
 *               Pull.     P_c,k and W_k are the plain rule's chains of p_c and w0 (the box above, the same order and clamps, every
 *                         level rounded to f32 before the next is made, so the fused form and KC_MIP_PER_LEVEL give the same
 *                         bits).  A texel of level k >= 1 is known when W_k > 0, and its colour is then q_c = P_c,k / W_k
 *                         (kc_mip_alpha_texel, which also reports known or unknown; unknown: q = 0).  A texel of level 0 is known
 *                         when w0 > 0, and its colour is c itself, bit for bit.  A known texel with a NaN or infinite colour
 *                         follows IEEE; NaN payloads are not in the contract.
 *               Push.     F_k(x, y), the stored colour: q where the texel is known; otherwise
 *                         F_{k+1}(min(x >> 1, W - 1), min(y >> 1, H - 1)) with W x H the size of level k + 1; an unknown texel of
 *                         the last level stores +0.0 in all three channels.  Equivalently a texel takes the q of its nearest known
 *                         ancestor (min(x >> (j - k), W_j - 1), min(y >> (j - k), H_j - 1)), j > k, or 0.0 if it has none; the
 *                         per-texel form has no ordering between levels, and it is what the device runs.
 *               Alpha     is not touched: the plain rule, or coverage's with KC_MIP_COVERAGE (the two combine: coverage rewrites
 *                         alpha and never looks at colour, this rule rewrites colour and reads only level 0's alpha).
 *             Consequences: a constant alpha of 1 gives the plain chain bit for bit (c * 1 = c, box(1) = 1, P / 1 = P); an image
 *             without a positive alpha gets zero colour everywhere; a known texel's colour lies in the hull of the known
 *             level-0 colours under it, up to rounding; on odd extents the box drops the last column or row, so an opaque texel
 *             there has no known ancestor above it.
 *             Levels: under the flag levels[0] is an image of its own (+1 reference as before): its R, G, B are new planes --
 *             the known texels copied, the unknown ones filled -- and its alpha is img's plane, shared; every level >= 1 gets
 *             new colour planes.  Constants: a constant alpha >= 1 makes the call the plain chain of the image (levels[0] is
 *             img itself, nothing new is launched); a constant alpha of weight 0 gives constant-zero colour planes at every
 *             level and launches nothing new; constant or aliased colour planes beside a resident alpha, and a constant alpha
 *             strictly between 0 and 1, go through the kernels (a constant channel is a value in the launch's arguments, aliased
 *             ones are loaded once each from memory); four constant planes are folded on the host through kc_mip_alpha_texel.
 *             The flag is for RGBA images: a Gray image is KC_ERR_INVALID_ARG exactly where KC_MIP_COVERAGE refuses it.  With
 *             KC_MIP_NORMALS it is KC_ERR_UNSUPPORTED (a vector is not a colour), refused with the other flag errors.  It
 *             combines with KC_MIP_COVERAGE_REF(B), KC_MIP_PER_LEVEL and KC_BC_SRGB.  Accepted by the entry points that accept
 *             KC_MIP_COVERAGE (kc_image_write_dds without mips: no effect); kc_dds_header, kc_image_build_roughness_mips and
 *             kc_image_mip_coverage_info refuse it, and previews stay defined by the plain rule.
 *             kc_stats: the four channels p_r, p_g, p_b, w go down together in one thread, so the pull takes the launches of
 *             the plain chain of one plane (4096 x 4096: two; counters "mip_alpha_pull_pyramid", "mip_alpha_pull_level"; the
 *             first launch also stores level 0's colour); the push is one launch over all levels ("mip_alpha_push") and runs
 *             whenever the pull does; a 1 x 1 image takes one "mip_alpha_pull_level" launch that only writes level 0, and the
 *             push.  A resident alpha keeps its plain launches.  Algorithmic bytes, with N_k = W_k H_k: 4 N_0 per distinct
 *             resident plane read by the pull, 12 N_0 for level 0's colour, 16 N_k for the three colours and the weight of every
 *             level k >= 1 (the weights live in scratch planes from the pool, returned when the call returns), 28 N_k for every
 *             level whose P and W are handed to a further launch (three state planes written and read, the weight read), and
 *             for the push 4 N_0 where alpha is resident plus 4 N_k for every k >= 1 -- 38.7 bytes per level-0 texel of an
 *             image of four resident planes, 44.0 with alpha's plain chain; the unknown texels the push writes (12 bytes each,
 *             with the ancestors' colours they read) depend on the data and are not counted.
 *   kc_mip_alpha_weight, kc_mip_alpha_texel  w0 of an alpha, and q = P / W with known = 1 where W > 0, q = 0 with known = 0
 *                        elsewhere: arithmetic, no kc_init needed; the constant fold calls them.  A NULL argument is
 *                        KC_ERR_INVALID_ARG.
 *   Roughness chains (kc_image_build_roughness_mips).  Renormalising a coarser level of a normal map throws away the length of
 *             the averaged vector, the only record of how much the normals varied under the texel: beside a plain-boxed
 *             roughness chain, bumpy surfaces turn mirror-smooth with distance and sparkle.  This chain raises every level of a
 *             roughness plane by the variance of the normals under the texel (Toksvig; tests/mip_roughness_ref.py is the same
 *             rule in numpy).  Inputs: a roughness plane rho, one channel of an image, linear f32; a normal map of the same
 *             size, an RGBA image with X, Y, Z in R, G, B stored as n * 0.5 + 0.5; `power`, a finite f32, 0 < power <= 65536.
 *             Everything is f32, nothing is fused, denormals are kept, / and sqrtf are correctly rounded.
 *               Level 0 of the normals: unit vectors.  Per texel, with e_c the stored channel:
 *                         v_c = e_c * 2.0f - 1.0f,  q = (v_x * v_x + v_y * v_y) + v_z * v_z,  l0 = sqrtf(q),
 *                         u_c = v_c / l0 if l0 > 0 && l0 < +inf, else u = (0, 0, 1)      (kc_mip_unit_normal)
 *                         The comparison is false for NaN: a zero vector, an overflow, a NaN or an infinity in any channel
 *                         give (0, 0, 1), and u is always finite.  A map that went through 8 bits has lengths of 1 +- 0.004;
 *                         without this step that quantisation error would read as variance on every smooth surface.
 *               State.    m_c,k is the plain rule's chain of u_c (the box above, the same order and clamps, every level rounded
 *                         to f32 before the next is made); m lives in vector space, never re-encoded and never renormalised.
 *                         r_k is the plain rule's chain of rho, always made from the unadjusted r_{k-1}: the adjustment never
 *                         compounds, exactly as coverage treats alpha.
 *               A texel of level k >= 1, d = rough(m, r, power)                          (kc_mip_roughness_texel):
 *                         if r != r:                 d = r          (NaN stays NaN; payload not in the contract)
 *                         q = (m_x * m_x + m_y * m_y) + m_z * m_z,  l = sqrtf(q)
 *                         else if l == 0:            d = 1.0f       (the normals cancel: every direction is present)
 *                         else t = (1.0f - l) / l
 *                              if !(t > 0x1p-14f):   d = r          (a flat footprint keeps the plain box bit for bit, unclamped)
 *                              else te = t - 0x1p-14f
 *                                   rc = min(max(r, 0.0f), 1.0f),  a = rc * rc,  a2 = a * a
 *                                   B  = ((2.0f * te) * power) * (a2 - 1.0f)
 *                                   n  = (B - a2) / (B - 1.0f)
 *                                   d  = sqrtf(sqrtf(n))
 *                         B <= 0 and B - 1 <= -1, so n lies in [a2, 1] up to rounding and no NaN or infinity arises for a
 *                         non-NaN r; d may lie an ulp or two below rc near 1, which is not part of the contract.  The floor
 *                         2^-14 swallows the rounding of the normalisation (unit vectors and their 8-bit quantisations have
 *                         t <= 1.8e-7), so a normal map that is flat under a texel leaves the roughness chain equal to the plain
 *                         chain bit for bit.  Level 0 is the image itself, untouched.  m and r are rounded per level, so the
 *                         fused form and KC_MIP_PER_LEVEL give the same bits.
 *             kc_image_build_roughness_mips: `img` is Gray (`channel` must be 0) or RGBA (`channel` 0..3: an ORM texture keeps
 *             roughness in G, a normal map often in its own alpha, so img == normals is legal).  `levels`, `count` and `cap` as
 *             kc_image_build_mips: levels[0] is img (+1 reference), the level images are of img's kind.  The named channel
 *             follows the rule above and gets a new resident plane of its own at every level >= 1, also where it aliases
 *             another channel at level 0 or is a constant plane; every other channel follows the plain rule (constants folded,
 *             aliases shared).  If R, G and B of `normals` are all constant planes the rule gives d = r everywhere: the call is
 *             then the plain chain of img and launches nothing new.  Pending chains and deferred resizes of both images run
 *             first.  flags: KC_MIP_PER_LEVEL only.  Errors, in this order: other flag bits KC_ERR_UNSUPPORTED; a NULL argument
 *             or a `power` that is NaN, not finite, <= 0 or > 65536 KC_ERR_INVALID_ARG; KC_ERR_NO_DEVICE; then, with `*count`
 *             written and nothing launched or allocated, KC_ERR_INVALID_ARG for `normals` not RGBA, sizes that differ (there is
 *             no implicit resize), `channel` out of range for the kind, cap < L, or the size limits of kc_image_build_mips.  A
 *             failure part-way releases what it made.  kc_stats: the four channels go down together, so the launches are those
 *             of the plain chain of one plane (4096 x 4096: two; counters "mip_roughness_pyramid", "mip_roughness_level"), beside
 *             the plain launches of the other resident channels; 4 w h algorithmic bytes per distinct resident plane read among
 *             the four, 4 sum_{k >= 1} W_k H_k written, and 32 W_k H_k for every level k whose four boxes are handed to a
 *             further launch through planes from the pool (written once, read once).
 *   kc_mip_unit_normal, kc_mip_roughness_texel  u of a stored texel and rough() of the rule above: arithmetic, no kc_init needed.
 *                        A NULL argument, or a `power` outside (0, 65536], is KC_ERR_INVALID_ARG.
 *   kc_image_levels_to_bc_mips, kc_image_levels_write_dds  encode a chain the caller holds -- kc_image_build_roughness_mips's
 *                        result, or any edited chain: 1 <= count <= L of levels[0]'s size, every levels[k] non-NULL, of one
 *                        kind and max(1, w >> k) by max(1, h >> k); anything else is KC_ERR_INVALID_ARG.  flags: KC_BC_SRGB
 *                        under kc_image_to_bc's rule for the format.  Level k goes at its kc_bc_mip_layout offset; `host_bytes`
 *                        is at least the bytes of the first `count` levels.  The DDS form writes kc_dds_header(..., count) in
 *                        front.  Pending chains of the levels run first; blocks until the bytes are there.
 *   kc_alpha_ref_threshold, kc_mip_coverage_target, kc_mip_coverage_scale  r_B, T_k (level 0: C_0) and s_k of the rule above:
 *                        arithmetic, no kc_init needed.  A NULL output, ref_u8 outside 1..255, a zero size, more than 2^31 texels,
 *                        covered0 > N_0 or level >= L is KC_ERR_INVALID_ARG.
 *   kc_image_mip_coverage_info  one record per level of what kc_image_build_mips with the same flags does to alpha (flags must
 *                        hold KC_MIP_COVERAGE_REF(B); RGBA only): texels N_k, target T_k, plain_covered P_k, v = v_k and scale =
 *                        s_k (v = 0 where nothing was selected; level 0: C_0 in both counts, scale 1).  `*count` = L; cap < L is
 *                        KC_ERR_INVALID_ARG.  Runs alpha's plain chain and the select (not the scale) and blocks until the records
 *                        are back; a constant alpha is answered on the host.
 *   kc_mip_normal_texel  the rule above from the three boxes to the stored texel, out = d(box): the function the constant fold
 *                        calls.  Arithmetic, no kc_init needed.  A NULL argument is KC_ERR_INVALID_ARG.
 *   kc_mip_level_count  L for a size; arithmetic, no kc_init needed.
 *   kc_preview_level     the level a thumbnail or a viewport of at most max_extent texels a side is cut from: the smallest k with
 *                        max(W_k, H_k) <= max_extent, and that level's size (k < L always: the last level is 1 x 1).  Arithmetic, no
 *                        kc_init needed.  max_extent == 0, a zero size or a NULL output is KC_ERR_INVALID_ARG and writes nothing.
 *   kc_image_build_mips  levels[0] = img itself (+1 reference), levels[k] a new image of the same kind (+1 reference each);
 *                        `*count` = L whenever the image is known; cap < L is KC_ERR_INVALID_ARG with nothing launched and nothing
 *                        allocated.  Enqueued on the library's stream; the call does not wait.  A failure part-way releases what
 *                        it made.  KC_MIP_PER_LEVEL: one launch per level (A/B runs and tests; the same bits).  KC_MIP_NORMALS,
 *                        KC_MIP_COVERAGE, KC_MIP_ALPHA_WEIGHT: above.
 *                        kc_stats: one launch per up to six levels while both extents still halve, one per level after that
 *                        (4096 x 4096: two; counters "mip_pyramid", "mip_level"); 4 w h algorithmic bytes per distinct resident
 *                        plane read plus 4 sum_{k >= 1} W_k H_k per plane written; constant planes launch nothing.
 *   kc_bc_mip_layout     the BC chain of a size: level k's blocks are tightly packed rows, ceil(W_k / 4) x ceil(H_k / 4) blocks
 *                        (the 2 x 2 and 1 x 1 levels are one edge block), exactly what kc_image_to_bc writes for that level;
 *                        levels 0 .. L - 1 follow one another.  `*levels` = L, offsets[k] = level k's first byte (`offsets` may be
 *                        NULL; otherwise cap < L is KC_ERR_INVALID_ARG), `*total_bytes` = the chain's bytes.  Arithmetic, no kc_init.
 *   kc_image_to_bc_mips  kc_image_build_mips, then the encoder of kc_image_to_bc once per level, into host memory (`host_bytes`
 *                        at least the total); blocks until the bytes are there.  flags: KC_BC_SRGB (BC1 / BC3 / BC7) | KC_MIP_PER_LEVEL |
 *                        KC_MIP_NORMALS | KC_MIP_COVERAGE_REF(B) | KC_MIP_ALPHA_WEIGHT.
 *                        KC_BC6H quantises every level's own f32 values, so the chain keeps the range of the planes.
 *   kc_image_to_bc_mips_device  the same into device memory (a multiple of the block bytes; `bytes` at least the total, the
 *                        total's extent in one allocation of the library's device), ordered against `hip_stream` by the two event
 *                        edges of kc_image_to_bc_device.  Bytes past the total are never written.
 *                        kc_live_graph_buffer_bc_mips: the same for a slot's image.
 *   kc_dds_header        the 148 bytes in front of the blocks in a .dds file, DX10 form: "DDS ", DDS_HEADER (dwSize 124, flags
 *                        0x81007 plus 0x20000 with levels > 1, height, width, level 0's block bytes as the linear size, depth 0,
 *                        `levels` as the mip count, pixel format {32, DDPF_FOURCC, "DX10"}, caps 0x1000 plus 0x400008 with
 *                        levels > 1), DDS_HEADER_DXT10 {dxgiFormat, TEXTURE2D, 0, 1, 0}; dxgiFormat BC1 71, BC3 77, BC4 80,
 *                        BC5 83, BC6H 95, BC7 98, with KC_BC_SRGB BC1 72, BC3 78, BC7 99.  1 <= levels <= L.  `*bytes` (optional) = 148.
 *                        No kc_init.
 *   kc_image_write_dds   the header, then the chain (with_mips != 0) or level 0 alone.
 * Errors, in this order: unknown flag bits, KC_BC_SRGB with BC4 / BC5 / BC6H, KC_MIP_NORMALS with KC_BC_SRGB or with
 * KC_MIP_ALPHA_WEIGHT, or a reference byte without KC_MIP_COVERAGE or the reverse, KC_ERR_UNSUPPORTED; a NULL argument, a zero size, an
 * unknown format, a size below the total KC_ERR_INVALID_ARG; KC_ERR_NO_DEVICE before kc_init; KC_ERR_NO_SLOT_DATA where
 * kc_live_graph_buffer_bc returns it; KC_ERR_IO for a file that cannot be written. */
#define KC_MIP_PER_LEVEL 2u  /* one launch of the one-level kernel per level instead of the fused pyramid kernel; a bit of its
                                own beside KC_BC_SRGB, since the chain exporters take both in one flags word */
#define KC_MIP_NORMALS 32u   /* R, G, B are a normal map: every level is renormalised before the next is made (above); 4 and 8
                                stay refused by the chain entry points, 16 is KC_BC_ALL_MODES */
#define KC_MIP_COVERAGE 64u  /* alpha is tested against the byte in bits 24-31: every level keeps level 0's coverage (above) */
#define KC_MIP_COVERAGE_REF(b) (64u | ((uint32_t)(b) << 24))  /* KC_MIP_COVERAGE with the reference byte b, 1..255 */
#define KC_MIP_ALPHA_WEIGHT 128u  /* R, G, B of every level are alpha-weighted and the empty texels filled from the coarser levels (above) */
typedef struct kc_mip_coverage_level {
    uint64_t texels, target, plain_covered;  /* N_k, T_k, P_k (level 0: C_0 in both counts) */
    float v, scale;                          /* v_k (0 where nothing was selected) and s_k */
} kc_mip_coverage_level;
KC_API int kc_mip_level_count(uint32_t width, uint32_t height, uint32_t *levels);
KC_API int kc_preview_level(uint32_t width, uint32_t height, uint32_t max_extent, uint32_t *level, uint32_t *level_width,
                            uint32_t *level_height);
/* Previews: rects of mip levels of many images as RGBA8, without building a chain -- the thumbnails of an editor's nodes and
 * the viewport of the selected one, in one call.  The bytes of one request are exactly kc_image_to_u8(levels[level], srgb) of
 * kc_image_build_mips(image), cut to the rect: the 2 x 2 box above with every level rounded to f32, kc_image_to_u8's quantisers
 * (Gray is (v, v, v, 255), alpha stays linear under KC_PREVIEW_SRGB, NaN exports as 255), constant planes folded on the host once
 * per level.  Row j of the rect starts at byte offset_bytes + j * row_pitch_bytes of the output; bytes between the rows of a rect
 * and bytes outside every rect are never written.  Requests whose byte ranges overlap are the caller's error: the library does
 * not detect it and what such bytes hold afterwards is undefined.
 *   Passes.   With H = min(floor(log2 w), floor(log2 h)) -- how often both extents halve -- a request with level <= H is fused:
 *             one workgroup per 64 x 64 source tile that touches the rect's footprint reduces it min(level, 6) levels in
 *             registers and stores only the last, straight to RGBA8 when level <= 6.  A deeper level first writes the level-6
 *             values of the footprint (the rect scaled by 2^(level - 6)) to an f32 scratch, which the next pass reads as an image
 *             of its own, and so on: ceil(level / 6) passes, no level in between ever stored.  Level 0 is read directly, four
 *             texels per thread.  A request with level > H (one extent has reached 1, the box clamps) takes the fallback:
 *             kc_image_build_mips, then the rect of levels[level] (counter "preview_fallback").  An image of constant planes
 *             reads nothing and is filled by the same launch.
 *   Launches. All requests of a call share each pass: a batch without fallbacks is max(1, ceil(max level / 6)) launches whatever
 *             `count` is (kc_stats; counter "preview_launches"), the jobs of a pass one table uploaded with one copy.  Planes that
 *             alias (kc_image_as_type's [p, p, p, ones]) are read once.  kc_stats_algorithmic_bytes: 4 bytes per source texel
 *             read -- the tiles that touch the footprint, clipped to the image; the rect itself at level 0 -- per distinct
 *             resident plane, plus the bytes written (4 per texel of the rect, 4 per plane and scratch texel).
 *   kc_image_previews         into host memory; blocks until the bytes are there.
 *   kc_image_previews_device  into device memory (a multiple of 4; `bytes` at least the last byte of any request, that extent in
 *                             one allocation of the library's device, as kc_image_to_bc_mips_device validates it), ordered
 *                             against `hip_stream` by the two event edges of kc_image_to_device.
 *   kc_live_graph_buffer_previews  request i reads the image of slot slot_ids[i] of node node_ids[i]; r[i].image is ignored.
 *   kc_preview_plan           what one request of a w x h image takes: arithmetic, no kc_init needed -- the same host function the
 *                             entry points plan with.  An all-constant image is not planned: it always runs as one level-0 pass.
 * Pending chains and deferred resizes of every named image run first.  count == 0 is KC_OK and launches nothing; count > 4096 is
 * KC_ERR_INVALID_ARG.  Errors, in this order: flag bits other than KC_PREVIEW_SRGB KC_ERR_UNSUPPORTED; a NULL argument (also with
 * count == 0), a NULL image, an empty rect, an offset or a pitch that is not a multiple of 4, a pitch below 4 * width, a request
 * whose last byte lies past the buffer KC_ERR_INVALID_ARG; KC_ERR_NO_DEVICE before kc_init; KC_ERR_NO_SLOT_DATA where
 * kc_live_graph_buffer_device returns it; a level at or above L or a rect that reaches outside the level KC_ERR_INVALID_ARG.  A
 * failed call writes nothing. */
typedef struct kc_preview_request {
    kc_image *image;              /* ignored by the live-graph form */
    uint32_t level;               /* 0 .. L-1 */
    uint32_t x, y, width, height; /* rect in texels of that level: non-empty, inside the level */
    size_t offset_bytes;          /* first byte of the rect's RGBA8 rows in the output; multiple of 4 */
    size_t row_pitch_bytes;       /* multiple of 4, >= 4 * width */
} kc_preview_request;
#define KC_PREVIEW_SRGB 1u        /* R, G, B (Gray: the value) as kc_image_to_u8 with srgb = 1 writes them; alpha linear */
#define KC_PREVIEW_MAX_PASSES 6
typedef struct kc_preview_plan_info {
    uint32_t passes;              /* launches the request takes part in (the fallback: 1, after the chain's own) */
    uint32_t fallback;            /* 1: level > H, kc_image_build_mips runs first */
    uint32_t level_width, level_height;                   /* the extent of the requested level */
    uint32_t levels[KC_PREVIEW_MAX_PASSES];               /* per pass: the levels it reduces, 0 .. 6 */
    uint32_t workgroups[KC_PREVIEW_MAX_PASSES];           /* per pass: its workgroups of 256 threads */
    uint32_t scratch_width[KC_PREVIEW_MAX_PASSES];        /* per pass: the extent it writes to the f32 scratch of the next */
    uint32_t scratch_height[KC_PREVIEW_MAX_PASSES];       /*   pass; 0 x 0 for the last pass */
    uint64_t scratch_bytes[KC_PREVIEW_MAX_PASSES];        /* per pass: that scratch's bytes per distinct resident plane */
} kc_preview_plan_info;
KC_API int kc_image_previews(const kc_preview_request *r, uint32_t count, uint32_t flags, uint8_t *host, size_t host_bytes);
KC_API int kc_image_previews_device(const kc_preview_request *r, uint32_t count, uint32_t flags, void *device_ptr, size_t bytes,
                                    void *hip_stream);
KC_API int kc_live_graph_buffer_previews(kc_live_graph *lg, const uint32_t *node_ids, const uint32_t *slot_ids,
                                         const kc_preview_request *r, uint32_t count, uint32_t flags, uint8_t *host, size_t host_bytes);
KC_API int kc_preview_plan(uint32_t width, uint32_t height, uint32_t level, uint32_t x, uint32_t y, uint32_t rect_w, uint32_t rect_h,
                           kc_preview_plan_info *out);
KC_API int kc_mip_normal_texel(const float box[3], float out[3]);
KC_API int kc_alpha_ref_threshold(uint32_t ref_u8, float *r);
KC_API int kc_mip_coverage_target(uint32_t width, uint32_t height, uint64_t covered0, uint32_t level, uint64_t *target);
KC_API int kc_mip_coverage_scale(float v, uint32_t ref_u8, float *s);
KC_API int kc_image_mip_coverage_info(kc_image *img, uint32_t flags, kc_mip_coverage_level *out, uint32_t cap, uint32_t *count);
KC_API int kc_mip_alpha_weight(float a, float *w);
KC_API int kc_mip_alpha_texel(const float p[3], float w, float q[3], int *known);
KC_API int kc_image_build_mips(kc_image *img, uint32_t flags, kc_image **levels, uint32_t cap, uint32_t *count);
KC_API int kc_bc_mip_layout(uint32_t width, uint32_t height, int format, uint32_t *levels, size_t *offsets, uint32_t cap,
                            size_t *total_bytes);
KC_API int kc_image_to_bc_mips(kc_image *img, int format, uint32_t flags, uint8_t *host, size_t host_bytes);
KC_API int kc_image_to_bc_mips_device(kc_image *img, int format, uint32_t flags, void *device_ptr, size_t bytes, void *hip_stream);
KC_API int kc_dds_header(uint32_t width, uint32_t height, int format, uint32_t flags, uint32_t levels, uint8_t out[148], size_t *bytes);
KC_API int kc_image_write_dds(kc_image *img, const char *path, int format, uint32_t flags, int with_mips);
KC_API int kc_mip_unit_normal(const float rgb[3], float u[3]);
KC_API int kc_mip_roughness_texel(const float m[3], float r, float power, float *d);
KC_API int kc_image_build_roughness_mips(kc_image *img, uint32_t channel, kc_image *normals, float power, uint32_t flags,
                                         kc_image **levels, uint32_t cap, uint32_t *count);
KC_API int kc_image_levels_to_bc_mips(kc_image *const *levels, uint32_t count, int format, uint32_t flags, uint8_t *host,
                                      size_t host_bytes);
KC_API int kc_image_levels_write_dds(kc_image *const *levels, uint32_t count, const char *path, int format, uint32_t flags);
/* Signed distance fields: the cutout seen from close up.  The chains above keep a cutout right under minification; under
 * magnification a bilinear tap of a 1-bit or steep alpha gives staircase edges, and the standard answer (alpha-tested
 * magnification) is to ship the signed distance field of the mask instead: built at the authoring resolution, resized down
 * hard, stored in one BC4 channel, and tested against 0.5.  kc_image_distance_field builds the field on the device; the rule
 * is integer arithmetic up to one f64 expression, so the f32 words are exact (tests/sdf_ref.py is the same rule in numpy).
 *   Inside.   With B = ref_u8 (1..255) a texel of the channel is inside when quant_u8(a) >= B: the "covered" test of
 *             KC_MIP_COVERAGE and kc_alpha_ref_threshold; NaN counts as inside.  Every other texel is outside.
 *   D2.       For the texel at integer coordinates (x, y), the smallest dx^2 + dy^2 over all texels of the other class: a plain
 *             integer.  Texels beyond the image do not exist; with KC_SDF_WRAP the image tiles on both axes and dx, dy are
 *             torus distances, min(|d|, n - |d|).  If the other class is empty, D2 is "none".
 *   Cap.      With S = spread (1..KC_SDF_MAX_SPREAD), cap = S S + S + 1 and D2c = min(D2, cap), "none" giving cap.  The largest
 *             integer D2 with sqrt(D2) < S + 0.5 is S S + S, and a texel at that distance has |dx| <= S and |dy| <= S: a search
 *             window of radius S on each axis is exact for everything below the cap, and everything else saturates.
 *   Value.    D2c == cap: v = 1.0f inside, 0.0f outside.  Otherwise, in f64: d = sqrt((double)D2c), sd = inside ? d - 0.5 :
 *             0.5 - d, v = (float)(0.5 + sd / (2.0 * S)) -- IEEE sqrt, divide and add, one rounding to f32 at the end.  The
 *             boundary sits midway between texel centres: an inside texel next to an outside one gets 0.5 + 0.25 / S, so
 *             v >= 0.5 holds exactly for the inside texels of the source.
 *   kc_image_distance_field  `*out` (+1 reference) = a new Gray image of the source's size; the source is untouched.  channel:
 *             0 for Gray, 0..3 for RGBA.  A pending chain of the image runs first.  A constant plane launches nothing and gives
 *             the constant image 1.0 (inside) or 0.0 (outside).  Otherwise two launches whatever the size (kc_stats; counters
 *             "sdf_columns", "sdf_rows"): per column the distance to the nearest texel of the other class within S rows, then
 *             per row the minimum over the columns within S; 12 algorithmic bytes per texel (4 read, a 16-bit intermediate
 *             written and read back, 4 written).  Enqueued on the library's stream; the call does not wait.
 *             Errors, in this order: KC_ERR_NO_DEVICE before kc_init; flag bits other than KC_SDF_WRAP KC_ERR_UNSUPPORTED; a NULL
 *             argument, ref_u8 outside 1..255, spread outside 1..KC_SDF_MAX_SPREAD, a channel the image does not have, more
 *             than 2^31 texels KC_ERR_INVALID_ARG.  Nothing is launched or allocated on a refusal.
 *   kc_sdf_texel  the value rule on one texel: d2 is taken after capping (d2 >= cap saturates), inside != 0 is the class.
 *   kc_sdf_cap    cap for a spread.  Both are arithmetic, no kc_init needed; a NULL output or a spread outside
 *             1..KC_SDF_MAX_SPREAD is KC_ERR_INVALID_ARG.
 * Not here: anti-aliased (sub-texel) edge estimates from fractional alpha, per-axis wrap, a graph node type, multi-channel fields. */
#define KC_SDF_WRAP 1u         /* the image tiles on both axes: torus distances */
#define KC_SDF_MAX_SPREAD 254  /* a capped axis distance, S + 1, fits one byte */
KC_API int kc_image_distance_field(kc_image *img, uint32_t channel, uint32_t ref_u8, uint32_t spread, uint32_t flags, kc_image **out);
KC_API int kc_sdf_texel(uint32_t d2, int inside, uint32_t spread, float *v);
KC_API int kc_sdf_cap(uint32_t spread, uint32_t *cap);
/* Blur: a separable Gaussian of the planes of an image, on the device -- a height map smoothed before HeightToNormal, a
 * distance field softened before it is resized down, a mask feathered, roughness low-passed, a tileable texture kept tileable.
 * The result is exact as a function of its f32 weights (tests/blur_ref.py is the same rule in numpy).
 *   Radius.   For an axis with sigma > 0: R = max(1, (uint32_t)ceil(3.0 * (double)sigma)); R > KC_BLUR_MAX_RADIUS is refused.
 *             sigma == 0 means "this axis is not blurred": no pass, no rounding.  NaN, negative and infinite sigmas are refused.
 *   Weights.  On the host in f64, rounded to f32 once: with s = (double)sigma, g_k = exp(-(double)(k k) / (2.0 s s)) for
 *             k = 0..R, total = g_0 + 2 (g_1 + g_2 + ... + g_R) with the inner sum taken in ascending k, w_k = (float)(g_k / total).
 *             Weights that underflow to 0 stay taps.  The f32 weights do not sum to exactly 1, so a constant changes by a few
 *             ulps: part of the rule, not an error.
 *   Taps.     For output position i on an axis of n texels, tap j (-R..R) reads position i + j: clamped to 0..n-1 (the edge texel
 *             repeats), or with KC_BLUR_WRAP reduced by a true modulo n -- R may exceed n, the image may wrap more than once.
 *   Texel.    All in f32, every operation rounded on its own (no fused multiply-add), the outermost pair first, so that the
 *             small terms are summed before the large one:
 *                 acc = w_R (t[-R] + t[+R]);  for k = R-1 down to 1: acc = acc + w_k (t[-k] + t[+k]);  acc = acc + w_0 t[0]
 *             No tap is skipped: a zero weight times an infinity is NaN, as IEEE says.  Pairing the two sides makes the result
 *             exactly mirror-symmetric: blur(flip(x)) == flip(blur(x)) bit for bit.
 *   Passes.   Along x first, into an f32 intermediate, then along y on the intermediate; an axis with sigma == 0 is left out.
 *   kc_image_blur  `*out` (+1 reference) = a new image of the source's type and size; the source is untouched.  A pending chain
 *             or resample of the image runs first.  Bit c of channel_mask selects channel c (Gray: bit 0; RGBA: bits 0..3);
 *             unselected channels are the source's planes themselves.  Channels that are one plane in the source are blurred
 *             once and are one plane in the result.  A selected constant plane stays constant and is answered on the host: the
 *             texel rule on all-equal taps with the x weights, then on that result with the y weights; it allocates and launches
 *             nothing.  With both sigmas 0 the result shares every plane with the source and nothing is launched.  Otherwise one
 *             launch per blurred axis for all selected resident planes together -- two launches, or one when one sigma is 0,
 *             whatever the size and the channel count (kc_stats; counters "blur_rows", "blur_columns", and "blur_rows_nt",
 *             "blur_columns_nt" where the cache policy marks the source of the first pass, the result of the last, nontemporal);
 *             8 algorithmic bytes per texel, per blurred axis, per distinct resident plane.  The intermediate is a staging block
 *             of the pool that goes back when the call returns.  Enqueued on the library's stream; the call does not wait.
 *             Errors, in this order: KC_ERR_NO_DEVICE before kc_init; flag bits other than KC_BLUR_WRAP KC_ERR_UNSUPPORTED; a NULL
 *             argument, a sigma that is NaN, negative or infinite, a radius above KC_BLUR_MAX_RADIUS, a mask of 0, a mask with a
 *             bit the image has no channel for, more than 2^31 texels KC_ERR_INVALID_ARG.  Nothing is launched or allocated on a
 *             refusal, and `*out` is not written.
 *   kc_blur_weights  weights[0..R] and R for a sigma, as kc_image_blur uses them.  A NULL pointer, a capacity below R + 1, a sigma
 *             kc_image_blur would refuse, or sigma == 0, is KC_ERR_INVALID_ARG.
 *   kc_blur_texel    the texel rule on taps[0..2R] (the centre at R) with weights[0..R]; a NULL pointer or a radius outside
 *             1..KC_BLUR_MAX_RADIUS is KC_ERR_INVALID_ARG.  Both are arithmetic, no kc_init needed.
 * Not here: a graph node type, radii above 64 (blur twice: variances add; or resize down first), non-Gaussian kernels, per-axis
 * wrap, a single-launch fused form for small radii. */
#define KC_BLUR_WRAP 1u        /* the image tiles on both axes: taps are taken modulo the extent */
#define KC_BLUR_MAX_RADIUS 64  /* ceil(3 sigma): sigma up to 21.33 */
KC_API int kc_image_blur(kc_image *img, float sigma_x, float sigma_y, uint32_t channel_mask, uint32_t flags, kc_image **out);
KC_API int kc_blur_weights(float sigma, float *weights, uint32_t capacity, uint32_t *radius);
KC_API int kc_blur_texel(const float *taps, const float *weights, uint32_t radius, float *v);
/* The way back: BC blocks decoded on the device, the error of an encoding measured on the device, and .dds files read.
 * Decoding is integer arithmetic on the block's bytes, so the pixels are exact (tests/bc_decode_ref.py is the same rules in
 * numpy).  Pixel (x, y) is texel 4 (y % 4) + x % 4 of block (x / 4, y / 4); texels of edge blocks outside the image are dropped.
 *   BC1     c0, c1 u16 LE, then a u32 LE with texel t's index at bits 2t..2t+1; E() expands 5:6:5 by bit replication.  c0 > c1:
 *           palette E0, E1, (2 E0 + E1 + 1) div 3, (E0 + 2 E1 + 1) div 3, alpha 255.  Otherwise E0, E1, (E0 + E1) div 2 with alpha
 *           255, and index 3 is (0, 0, 0) with alpha 0.
 *   BC4     bytes e0, e1, then a 48-bit LE word with texel t's index at bits 3t..3t+2.  Indices 0 and 1 are e0 and e1.  e0 > e1:
 *           index i >= 2 is ((8 - i) e0 + (i - 1) e1 + 3) div 7.  Otherwise i in 2..5 is ((6 - i) e0 + (i - 1) e1 + 2) div 5,
 *           i = 6 is 0 and i = 7 is 255.
 *   BC3     the BC4 block is alpha; the BC1 block after it always decodes in four-colour mode, whatever the order of c0 and c1.
 *   BC5     the BC4 block of R, then that of G.
 *   BC7     the three single-subset modes 4, 5 and 6, in full: everything kc_image_to_bc writes and everything else that needs
 *           no partition table.  The mode is the position of the lowest set bit of byte 0; bit order, interp, W2 and W4 as for
 *           the encoder above; W3 = 0, 9, 18, 27, 37, 46, 55, 64.  Modes 6 and 5 have the layouts given above, mode 5 with any
 *           rotation.  Mode 4: bits 0-4 the value 16; rotation (5-6); index selection (7); R0, R1, G0, G1, B0, B1 of 5 bits
 *           each (8-37), decoded (q << 3) | (q >> 2); A0, A1 of 6 bits each (38-49), decoded (q << 2) | (q >> 4); the 2-bit
 *           index set, texel 0 in 1 bit (50), texels 1-15 in 2 bits each (51-80); the 3-bit set, texel 0 in 2 bits (81-82),
 *           texels 1-15 in 3 bits each (83-127).  Index selection 0: colour takes the 2-bit set with W2, alpha the 3-bit set with
 *           W3; 1: colour the 3-bit set with W3, alpha the 2-bit set with W2.  Rotation r in 1..3 (modes 4 and 5) swaps alpha
 *           with channel r - 1 after the interpolation.  Byte 0 == 0 is the reserved mode: (0, 0, 0, 0), as the format defines.
 *           Blocks of the partitioned modes 0, 1, 2, 3 and 7 are NOT decoded: they give (0, 0, 0, 0) and are counted in
 *           `*undecoded_blocks`.  BC1, BC3, BC4 and BC5 always count 0.
 *   BC6H    the four single-subset modes 11, 12, 13 and 14, in full: everything kc_image_to_bc writes and everything else that
 *           needs no partition table.  The mode field: bit 1 of byte 0 clear, 2 bits, 0 is mode 1 and 1 is mode 2; otherwise 5
 *           bits: 2, 6, 10, 14, 18, 22, 26, 30 are modes 3-10, 3, 7, 11, 15 are modes 11-14, and 19, 23, 27, 31 are reserved.
 *           Mode 11 has the layout given above.  Modes 12, 13, 14 store endpoint 0 in n = 11, 12, 16 bits and endpoint 1 as a
 *           signed delta of 9, 8, 4 bits: bits 5-34 are the low 10 bits of R0, G0, B0; then for R, G, B in turn a group of 10
 *           bits, LSB first: mode 12 delta[0..8], e0[10]; mode 13 delta[0..7], e0[11], e0[10]; mode 14 delta[0..3], e0[15],
 *           e0[14], e0[13], e0[12], e0[11], e0[10].  e1 = (e0 + sign_extend(delta)) mod 2^n.  unq_n(x) = x for n = 16, otherwise 0
 *           for x = 0, 0xFFFF for x = 2^n - 1 and ((x << 16) + 0x8000) >> n else.  The indices lie as in mode 11.  A texel channel
 *           is fin(interp(unq_n(e0), unq_n(e1), W4[index])), a half bit pattern <= 0x7BFF: never infinite, never NaN.  The image
 *           is RGBA: R, G and B resident planes that hold the halves' exact f32 values (not bytes / 255: up to 65504), A a
 *           constant plane of 1.  A block with a reserved mode field gives (0, 0, 0), as the format defines, and is not counted.
 *           Blocks of the two-subset modes 1-10 are NOT decoded: they give (0, 0, 0) and are counted in `*undecoded_blocks`.
 *   KC_BC_ALL_MODES  (a decode-side flag) every mode the two formats define: BC7 modes 0-7 and BC6H modes 1-14, so that another
 *           encoder's blocks decode in full (tests/bc_modes_ref.py is the same rules in numpy).  Nothing is undecoded:
 *           `*undecoded_blocks` and kc_bc_error.undecoded_blocks are 0, and the count is written without a wait.
 *           BC7.  A mode's fields follow one another from bit mode + 1: the partition index (4 bits in mode 0, 6 in modes 1, 2, 3,
 *           7), the rotation and the index selection (modes 4, 5), every R, every G, every B, then every A, the p-bits, the
 *           index sets.  Endpoint 2 s + k is endpoint k of subset s.  Per mode: subsets, endpoint bits, p-bits, index bits --
 *           0: 3, RGB 4, one p-bit per endpoint, 3;  1: 2, RGB 6, one p-bit per subset (shared by its two endpoints), 3;
 *           2: 3, RGB 5, none, 2;  3: 2, RGB 7, per endpoint, 2;  7: 2, RGBA 5, per endpoint, 2 (alpha takes the colour's index);
 *           modes 4, 5, 6 as above.  An endpoint channel of n stored bits q and p-bit p is x = 2 q + p in n + 1 bits (x = q
 *           without p-bits), expanded (x << (8 - bits)) | (x >> (2 bits - 8)); alpha is 255 in modes 0-3.  2-, 3- and 4-bit
 *           indices weigh by W2, W3 and W4; interp, the rotation and the reserved block (byte 0 == 0) as above.
 *           The subset of texel t is bit t of the two-subset table's entry, or bits 2t..2t+1 of the three-subset table's:
 *           two subsets, entries 0-63 (16 bits each):
 *             CCCC 8888 EEEE ECC8 C880 FEEC FEC8 EC80 C800 FFEC FE80 E800 FFE8 FF00 FFF0 F000
 *             F710 008E 7100 08CE 008C 7310 3100 8CCE 088C 3110 6666 366C 17E8 0FF0 718E 399C
 *             AAAA F0F0 5A5A 33CC 3C3C 55AA 9696 A55A 73CE 13C8 324C 3BDC 6996 C33C 9966 0660
 *             0272 04E4 4E40 2720 C936 936C 39C6 639C 9336 9CC6 817E E718 CCF0 0FCC 7744 EE22
 *           three subsets, entries 0-63 (32 bits each; mode 0 uses the first 16):
 *             AA685050 6A5A5040 5A5A4200 5450A0A8 A5A50000 A0A05050 5555A0A0 5A5A5050
 *             AA550000 AA555500 AAAA5500 90909090 94949494 A4A4A4A4 A9A59450 2A0A4250
 *             A5945040 0A425054 A5A5A500 55A0A0A0 A8A85454 6A6A4040 A4A45000 1A1A0500
 *             0050A4A4 AAA59090 14696914 69691400 A08585A0 AA821414 50A4A450 6A5A0200
 *             A9A58000 5090A0A8 A8A09050 24242424 00AA5500 24924924 24499224 50A50A50
 *             500AA550 AAAA4444 66660000 A5A0A5A0 50A050A0 69286928 44AAAA44 66666600
 *             AA444444 54A854A8 95809580 96969600 A85454A8 80959580 AA141414 96960000
 *             AAAA1414 A05050A0 A0A5A5A0 96000000 40804080 A9A8A9A8 AAAAAA44 2A4A5254
 *           Anchors.  Texel 0 is the anchor of subset 0; the anchors of the other subsets, per entry:
 *             two subsets, subset 1:    15 15 15 15 15 15 15 15 15 15 15 15 15 15 15 15 15  2  8  2  2  8  8 15  2  8  2  2  8  8  2  2
 *                                       15 15  6  8  2  8 15 15  2  8  2  2  2 15 15  6  6  2  6  8 15 15  2  2 15 15 15 15 15  2  2 15
 *             three subsets, subset 1:   3  3 15 15  8  3 15 15  8  8  6  6  6  5  3  3  3  3  8 15  3  3  6 10  5  8  8  6  8  5 15 15
 *                                        8 15  3  5  6 10  8 15 15  3 15  5 15 15 15 15  3 15  5  5  5  8  5 10  5 10  8 13 15 12  3  3
 *             three subsets, subset 2:  15  8  8  3 15 15  3  8 15 15 15 15 15 15 15  8 15  8 15  3 15  8 15  8  3 15  6 10 15 15 10  8
 *                                       15  3 15 10 10  8  9 10  6 15  8 15  3  6  6  8 15  3 15 15 15 15 15 15 15 15 15 15  3 15 15  8
 *           An anchor's index has one bit less than the others (its top bit is 0), so in a set of n-bit indices that starts at bit
 *           `base`, texel t's index lies at base + n t - (the anchors below t) and has n - 1 bits if t is an anchor.
 *           BC6H.  Modes 1-10 have two subsets: the first 32 entries of the two-subset table and of its anchors, 3-bit indices
 *           from bit 82 weighed by W3, and per channel four endpoints e0..e3 (subset s: e_2s, e_2s+1).  e0 has n bits; in modes
 *           1-9 e1, e2, e3 are signed deltas of (dR, dG, dB) bits, e_k = (e0 + sign_extend(delta)) mod 2^n; mode 10 stores four
 *           plain 6-bit endpoints.  n (dR dG dB) for modes 1-10: 10 (5 5 5), 7 (6 6 6), 11 (5 4 4), 11 (4 5 4), 11 (4 4 5),
 *           9 (5 5 5), 8 (6 5 5), 8 (5 6 5), 8 (5 5 6), 6 (plain).  The header, in every mode: the low min(n, 10) bits of R0, G0,
 *           B0 from bits 5, 15, 25; R1, R2, R3 from bits 35, 65, 71 (dR bits each); G1 from bit 45 (dG bits); G2[3:0] and G3[3:0]
 *           at 41-44 and 51-54; B1 from bit 55 (dB bits); B2[3:0] at 61-64; the partition at 77-81.  The remaining bits, as
 *           `block bit: value bit`, per mode --
 *             1:  2:G2[4] 3:B2[4] 4:B3[4] 40:G3[4] 50:B3[0] 60:B3[1] 70:B3[2] 76:B3[3]
 *             2:  2:G2[5] 3:G3[4] 4:G3[5] 12:B3[0] 13:B3[1] 14:B2[4] 22:B2[5] 23:B3[2] 24:G2[4] 32:B3[3] 33:B3[5] 34:B3[4]
 *             3:  40:R0[10] 49:G0[10] 50:B3[0] 59:B0[10] 60:B3[1] 70:B3[2] 76:B3[3]
 *             4:  39:R0[10] 40:G3[4] 50:G0[10] 59:B0[10] 60:B3[1] 69:B3[0] 70:B3[2] 75:G2[4] 76:B3[3]
 *             5:  39:R0[10] 40:B2[4] 49:G0[10] 50:B3[0] 60:B0[10] 69:B3[1] 70:B3[2] 75:B3[4] 76:B3[3]
 *             6:  14:B2[4] 24:G2[4] 34:B3[4] 40:G3[4] 50:B3[0] 60:B3[1] 70:B3[2] 76:B3[3]
 *             7:  13:G3[4] 14:B2[4] 23:B3[2] 24:G2[4] 33:B3[3] 34:B3[4] 50:B3[0] 60:B3[1]
 *             8:  13:B3[0] 14:B2[4] 23:G2[5] 24:G2[4] 33:G3[5] 34:B3[4] 40:G3[4] 60:B3[1] 70:B3[2] 76:B3[3]
 *             9:  13:B3[1] 14:B2[4] 23:B2[5] 24:G2[4] 33:B3[5] 34:B3[4] 40:G3[4] 50:B3[0] 70:B3[2] 76:B3[3]
 *             10: 11:G3[4] 12:B3[0] 13:B3[1] 14:B2[4] 21:G2[5] 22:B2[5] 23:B3[2] 24:G2[4] 31:G3[5] 32:B3[3] 33:B3[5] 34:B3[4]
 *           unq_n, interp (with its + 32) and fin as above; a reserved mode field gives (0, 0, 0).
 *           The flag is accepted by kc_image_from_bc, kc_image_from_bc_device, kc_image_read_dds and kc_image_bc_compare, with
 *           every format: with BC1, BC3, BC4 and BC5 it changes nothing (it combines with KC_BC_GRAY for BC4), so a caller who
 *           reads arbitrary files can always pass it.  Without it nothing changes.  kc_image_bc_error,
 *           kc_live_graph_buffer_bc_error, the encoders and the mip exporters refuse it as an unknown bit.  kc_stats: a BC7 or
 *           BC6H decode under the flag is one launch, with or without `undecoded_blocks`; the comparison stays two.
 *           kc_bc_error.flags echoes the flag and bc7_mode_blocks is filled as without it.
 *   kc_image_from_bc         `host`: tightly packed block rows, exactly what kc_image_to_bc writes (`host_bytes` at least
 *                            bx * by * block bytes).  `*out` (+1 reference) owns new planes; a decoded byte b is the f32
 *                            b / 255.f with the IEEE divide, as kc_image_from_u8 makes it, so kc_image_to_u8(*out, 0) returns
 *                            exactly the decoded bytes.  No transfer function is applied.  The image is RGBA: BC1 / BC3 / BC7
 *                            four resident planes (BC1's alpha 0 or 1); BC4 R resident, G = B = 0 and A = 1 constant planes;
 *                            BC5 R and G resident, B = 0 and A = 1 constant (the sampling convention; constant planes cost no
 *                            stores).  KC_BC_GRAY (BC4 only): a Gray image of the channel.  The call waits for its upload.
 *   kc_image_from_bc_device  the same from a kc_bc_image (kc_bc_image_validate's rules), ordered against `hip_stream` by the two
 *                            event edges of kc_image_to_bc_device; nothing aliases the caller's blocks.  With a non-NULL
 *                            `undecoded_blocks` and KC_BC7 or KC_BC6H the call blocks until the count is on the host, as
 *                            kc_image_channel_stats does; with NULL, or another format (count 0), it does not wait.
 *                            Errors, in this order: flag bits other than KC_BC_GRAY and KC_BC_ALL_MODES (KC_BC_SRGB included), or KC_BC_GRAY with a
 *                            format other than KC_BC4, KC_ERR_UNSUPPORTED; a NULL argument (`undecoded_blocks` may be NULL), an
 *                            unknown format, a zero size, more than 2^31 blocks, `host_bytes` below the blocks' bytes or a
 *                            descriptor kc_bc_image_validate refuses KC_ERR_INVALID_ARG; KC_ERR_NO_DEVICE before kc_init.
 *                            kc_stats: one launch (KC_BC7 / KC_BC6H with a count: two, the second sums the workgroups' counts), the
 *                            blocks' bytes plus 4 w h algorithmic bytes per resident plane written; a refused call launches nothing.
 *   kc_bc_error              the error of blocks against an image.  The source bytes are what kc_image_to_u8(img, srgb) writes
 *                            with srgb = flags & KC_BC_SRGB (Gray = (v, v, v, 1); the encoders' quantiser functions); the
 *                            decoded bytes are those above.  Only the image's pixels count, not the replicated texels of edge
 *                            blocks; undecoded blocks contribute their (0, 0, 0, 0).  The mask holds the channels the format
 *                            encodes (BC1: not alpha, which its encoder ignores).  KC_BC6H: the differences are taken
 *                            between half bit patterns, decoded minus h(source), as integers -- exact and independent of the
 *                            order like the byte formats; a log-like measure, since a half's pattern grows like the logarithm
 *                            of its value.  The mask is 0x7 and bc7_mode_blocks is zero.
 *   kc_image_bc_compare      any blocks of the image's size, the library's own or another encoder's.
 *   kc_image_bc_error        encodes into pool staging with kc_image_to_bc's encoder, then compares.
 *                            kc_live_graph_buffer_bc_error: the same for a slot's image.
 *                            Both block until the host values are there (kc_image_channel_stats' event).  Flags: kc_image_to_bc's
 *                            rule; kc_image_bc_compare also takes KC_BC_ALL_MODES.  Errors, in this order: that rule's KC_ERR_UNSUPPORTED; a NULL argument, an unknown format, a
 *                            descriptor kc_bc_image_validate refuses KC_ERR_INVALID_ARG; KC_ERR_NO_DEVICE before kc_init; a
 *                            descriptor size that differs from the image's KC_ERR_INVALID_ARG; KC_ERR_NO_SLOT_DATA where
 *                            kc_live_graph_buffer_bc returns it.  `*out` is written on KC_OK only.  A pending chain or resample
 *                            runs first.  kc_stats: kc_image_bc_compare two launches (the comparison, whose workgroups each
 *                            leave one record of integer sums, and a small combining launch), 4 w h
 *                            algorithmic bytes per distinct resident plane the format reads plus the blocks' bytes;
 *                            kc_image_bc_error three launches, the encoder's launch and bytes first.  Constant planes cost no
 *                            loads.
 *   kc_dds_parse             arithmetic on a buffer that holds a whole .dds file; no kc_init.  Accepted: the
 *                            DX10 form kc_dds_header writes (dxgiFormat 71, 72, 77, 78, 80, 83, 98 or 99, TEXTURE2D, array size
 *                            1, no cube flag; data at byte 148) and the legacy FourCCs DXT1, DXT5, ATI1 / BC4U, ATI2 / BC5U (data
 *                            at byte 128).  `levels` = dwMipMapCount when DDSD_MIPMAPCOUNT is set and the count non-zero, else 1;
 *                            at most kc_mip_level_count.  `data_bytes` = what kc_bc_mip_layout gives for those levels.  Errors, in
 *                            this order: a NULL argument, fewer than 128 bytes (148: DX10), a bad magic, dwSize != 124, a pixel
 *                            format size != 32 or a zero extent KC_ERR_INVALID_ARG; a well-formed header of anything else
 *                            (uncompressed, BC2, BC6H, signed, typeless, arrays, cube maps, volumes) KC_ERR_UNSUPPORTED (so the
 *                            dxgiFormat 95 file kc_image_write_dds writes for KC_BC6H is not read back: pass its blocks, from
 *                            byte 148 on, to kc_image_from_bc); `levels`
 *                            above the level count, or a buffer shorter than data_offset + data_bytes, KC_ERR_INVALID_ARG.
 *   kc_image_read_dds        kc_image_from_bc of level `level` of the file (kc_bc_mip_layout's offsets).  flags: KC_BC_GRAY | KC_BC_ALL_MODES.
 *                            `info` (optional) is written once the header has parsed.  Errors, in this order: flag bits other
 *                            than these two KC_ERR_UNSUPPORTED; a NULL path or `out` KC_ERR_INVALID_ARG; a file that cannot be
 *                            opened or read KC_ERR_IO; kc_dds_parse's errors (a file shorter than its header says is
 *                            KC_ERR_INVALID_ARG); level >= levels KC_ERR_INVALID_ARG; then kc_image_from_bc's. */
#define KC_BC_GRAY 4u  /* decode, BC4 only: a Gray image of the channel instead of the RGBA rule */
#define KC_BC_ALL_MODES 16u  /* decode and kc_image_bc_compare: every BC7 and BC6H mode, partitioned ones included; 8 stays refused */
typedef struct kc_bc_error {
    int32_t format;              /* kc_bc_format of the blocks */
    uint32_t flags;              /* the flags the call was given */
    uint32_t channel_mask;       /* bit c: channel c is compared: BC1 / BC6H 0x7, BC3 / BC7 / KC_BC_PUNCH_THROUGH 0xF, BC4 0x1, BC5 0x3 */
    uint64_t pixels;             /* width * height: the image's pixels, not the blocks' texels */
    uint64_t sse[4];             /* sum over the pixels of (decoded byte - source byte)^2; 0 outside the mask; BC6H: half bit patterns */
    uint32_t max_abs[4];         /* largest |decoded byte - source byte|; 0 outside the mask; BC6H: of half bit patterns, <= 31743 */
    uint64_t undecoded_blocks;   /* as kc_image_from_bc_device counts them (BC7's partitioned modes, BC6H's two-subset modes) */
    uint64_t bc7_mode_blocks[8]; /* BC7: blocks per mode 0..7 (reserved blocks in none); zero for the other formats */
} kc_bc_error;
typedef struct kc_dds_info {
    uint32_t width, height;
    int32_t format;              /* kc_bc_format */
    uint32_t flags;              /* KC_BC_SRGB for dxgiFormat 72 / 78 / 99 */
    uint32_t levels;
    size_t data_offset, data_bytes;
} kc_dds_info;
KC_API int kc_image_from_bc(const uint8_t *host, size_t host_bytes, uint32_t width, uint32_t height, int format, uint32_t flags,
                            kc_image **out, uint64_t *undecoded_blocks);
KC_API int kc_image_from_bc_device(const kc_bc_image *src, uint32_t flags, void *hip_stream, kc_image **out, uint64_t *undecoded_blocks);
KC_API int kc_image_bc_compare(kc_image *img, const kc_bc_image *blocks, uint32_t flags, kc_bc_error *out);
KC_API int kc_image_bc_error(kc_image *img, int format, uint32_t flags, kc_bc_error *out);
KC_API int kc_dds_parse(const uint8_t *data, size_t bytes, kc_dds_info *info);
KC_API int kc_image_read_dds(const char *path, uint32_t level, uint32_t flags, kc_image **out, kc_dds_info *info);
/* read_slot_image, src/shared.rs:218-261 (PNG only; decode on host, planes built on device). */
KC_API int kc_image_read_png(const char *path, kc_image **out);
KC_API int kc_image_write_png(kc_image *img, const char *path);        /* src/node/write.rs:5-21 */

/* ========================================================================================== *
 * Per-node operators -- the functions behind process_node_internal, src/node/node_type.rs:98-138.
 * Inputs arrive already resized and keyed by input slot (NULL = slot not connected), as after
 * resize_buffers + assign_slot_ids (node_type.rs:229-237,250-267).
 * ========================================================================================== */
/* calculate_size, src/shared.rs:61-139.  sizes[] in edge insertion order; slot_index = index of
 * the input SpecificSlot resolves to, or -1. */
KC_API int kc_calculate_size(int policy, const kc_size *sizes, int n, int slot_index, kc_size specific, kc_size *out);
/* image::imageops::resize per plane, call sites src/shared.rs:159-199. */
KC_API int kc_resize_image(kc_image *src, kc_size size, int filter, kc_image **out);
/* resize_buffers, src/shared.rs:141-216: images[] in edge insertion order, edges[] sorted by
 * input_slot (node_type.rs:230-231); keys[i] = (output node id, output slot id) of images[i]. */
KC_API int kc_resize_buffers(kc_image *const images[], const kc_edge keys[], int n, const kc_edge *edges_sorted,
                             int n_edges, int policy, uint32_t policy_slot, kc_size policy_size, int filter,
                             kc_image *out[]);
/* mix::process, src/node/mix.rs:51-134.  *out = NULL with KC_OK when the reference returns an
 * empty Vec (mixed Gray/Rgba after type matching, :126). */
KC_API int kc_mix_process(kc_image *left, kc_image *right, int mix_type, kc_image **out);
/* separate_rgba::process, src/node/separate_rgba.rs:38-69 */
KC_API int kc_separate_rgba_process(kc_image *input, kc_image *out[4]);
/* combine_rgba::process, src/node/combine_rgba.rs:14-97; first = slot_datas.get(0) (size source). */
KC_API int kc_combine_rgba_process(kc_image *const inputs[4], kc_image **out);
/* value::process, src/node/value.rs:14-26 */
KC_API int kc_value_process(float value, kc_image **out);
/* height_to_normal::process, src/node/height_to_normal.rs:16-77; *out = NULL when the reference
 * returns an empty Vec (no input / RGBA input). */
KC_API int kc_height_to_normal_process(kc_image *input, kc_image **out);

/* ========================================================================================== *
 * NodeGraph -- src/node_graph.rs:16-590
 * ========================================================================================== */
KC_API int kc_node_graph_new(kc_node_graph **out);                                  /* :25-31 */
KC_API int kc_node_graph_clone(const kc_node_graph *g, kc_node_graph **out);
KC_API int kc_node_graph_free(kc_node_graph *g);
KC_API int kc_node_graph_from_path(const char *path, kc_node_graph **out);          /* :33-46 */
KC_API int kc_node_graph_from_json(const char *json, kc_node_graph **out);          /* :104-107 */
KC_API int kc_node_graph_export_json(const kc_node_graph *g, const char *path);     /* :98-102 */
/* Serialises into buf (NUL-terminated); *needed = bytes required including the NUL. */
KC_API int kc_node_graph_to_json(const kc_node_graph *g, char *buf, size_t cap, size_t *needed);
KC_API int kc_node_graph_add_node(kc_node_graph *g, const kc_node_desc *node, uint32_t *node_id);       /* :315-320 */
KC_API int kc_node_graph_add_node_with_id(kc_node_graph *g, const kc_node_desc *node);                  /* :322-331 */
KC_API int kc_node_graph_connect(kc_node_graph *g, uint32_t output_node, uint32_t input_node, uint32_t output_slot, uint32_t input_slot); /* :416-446 */
KC_API int kc_node_graph_try_connect(kc_node_graph *g, uint32_t output_node, uint32_t input_node, uint32_t output_slot, uint32_t input_slot); /* :396-413 */
KC_API int kc_node_graph_remove_node(kc_node_graph *g, uint32_t node_id);                              /* :473-481 */
KC_API int kc_node_graph_remove_edge(kc_node_graph *g, kc_edge edge);                                  /* :462-471 */
KC_API int kc_node_graph_disconnect_slot(kc_node_graph *g, uint32_t node_id, int side, uint32_t slot_id); /* :496-515 */
KC_API int kc_node_graph_node_count(const kc_node_graph *g, uint32_t *count);
KC_API int kc_node_graph_node_ids(const kc_node_graph *g, uint32_t *ids, uint32_t cap, uint32_t *count); /* :125-127 */
KC_API int kc_node_graph_edges(const kc_node_graph *g, kc_edge *edges, uint32_t cap, uint32_t *count);
KC_API int kc_node_graph_input_slot_id_with_name(const kc_node_graph *g, const char *name, uint32_t *slot_id);  /* :271-276 */
KC_API int kc_node_graph_output_slot_id_with_name(const kc_node_graph *g, const char *name, uint32_t *slot_id); /* :278-283 */
KC_API int kc_node_graph_set_mix_type(kc_node_graph *g, uint32_t node_id, int mix_type);               /* :48-63 */
KC_API int kc_node_graph_set_image_node_path(kc_node_graph *g, uint32_t node_id, const char *path);    /* :65-83 */
/* Gives an Output node a new (de-collided) name; old_name (may be NULL) receives the previous one. */
KC_API int kc_node_graph_rename_output_node(kc_node_graph *g, uint32_t node_id, const char *new_name, char *old_name, size_t cap); /* :232-269 */

/* ========================================================================================== *
 * TextureProcessor / LiveGraph -- src/texture_processor.rs:18-115, src/live_graph.rs:63-645.
 * Evaluation is synchronous and stream-ordered: await_clean runs every dirty ancestor in
 * topological order on the calling thread (replaces engine::process_loop, src/engine.rs:25-312).
 * ========================================================================================== */
KC_API int kc_tex_pro_new(uint64_t memory_threshold, kc_tex_pro **out);              /* texture_processor.rs:34-56 */
KC_API int kc_tex_pro_free(kc_tex_pro *tp);
KC_API int kc_tex_pro_new_live_graph(kc_tex_pro *tp, kc_live_graph **out);           /* :58-64 */
KC_API int kc_live_graph_free(kc_live_graph *lg);
KC_API int kc_live_graph_set_flags(kc_live_graph *lg, int auto_update, int use_cache); /* live_graph.rs:71-72 */
KC_API int kc_live_graph_get_flags(const kc_live_graph *lg, int *auto_update, int *use_cache);
KC_API int kc_live_graph_set_node_graph(kc_live_graph *lg, const kc_node_graph *g);  /* :605-609 */
KC_API int kc_live_graph_node_graph(const kc_live_graph *lg, kc_node_graph **out_clone);
KC_API int kc_live_graph_add_node(kc_live_graph *lg, const kc_node_desc *node, uint32_t *node_id);      /* :426-433 */
KC_API int kc_live_graph_add_node_with_id(kc_live_graph *lg, const kc_node_desc *node);                 /* :435-444 */
KC_API int kc_live_graph_remove_node(kc_live_graph *lg, uint32_t node_id);                              /* :452-475 */
KC_API int kc_live_graph_connect(kc_live_graph *lg, uint32_t output_node, uint32_t input_node, uint32_t output_slot, uint32_t input_slot); /* :488-511 */
KC_API int kc_live_graph_remove_edge(kc_live_graph *lg, kc_edge edge);                                  /* :551-566 */
KC_API int kc_live_graph_disconnect_slot(kc_live_graph *lg, uint32_t node_id, int side, uint32_t slot_id); /* :568-594 */
KC_API int kc_live_graph_set_mix_type(kc_live_graph *lg, uint32_t node_id, int mix_type);               /* node_mut, :369-374 */
KC_API int kc_live_graph_rename_output_node(kc_live_graph *lg, uint32_t node_id, const char *new_name, char *old_name, size_t cap); /* :625-627 */
KC_API int kc_live_graph_set_resize(kc_live_graph *lg, uint32_t node_id, int policy, uint32_t policy_slot, kc_size policy_size, int filter);
KC_API int kc_live_graph_node_state(const kc_live_graph *lg, uint32_t node_id, int *state);             /* :244-250 */
KC_API int kc_live_graph_request(kc_live_graph *lg, uint32_t node_id);                                  /* :219-227 */
KC_API int kc_live_graph_prioritise(kc_live_graph *lg, uint32_t node_id);                               /* :229-237 */
/* await_clean_read / await_clean_write, :164-195: returns once node_id is Clean. */
KC_API int kc_live_graph_await_clean(kc_live_graph *lg, uint32_t node_id);
/* One scheduler pass: processes every Requested / Prioritised node (all non-clean nodes when
 * auto_update), src/engine.rs:128-183. */
KC_API int kc_live_graph_update(kc_live_graph *lg);
KC_API int kc_live_graph_slot_data(kc_live_graph *lg, uint32_t node_id, uint32_t slot_id, kc_image **out);   /* :415-420, +1 ref */
KC_API int kc_live_graph_slot_data_size(kc_live_graph *lg, uint32_t node_id, uint32_t slot_id, kc_size *size); /* :406-408 */
KC_API int kc_live_graph_slot_in_memory(kc_live_graph *lg, uint32_t node_id, uint32_t slot_id, int *in_memory); /* :410-412 */
KC_API int kc_live_graph_node_slot_ids(kc_live_graph *lg, uint32_t node_id, uint32_t *slot_ids, uint32_t cap, uint32_t *count); /* node_slot_datas, :389-404 */
KC_API int kc_live_graph_buffer_rgba(kc_live_graph *lg, uint32_t node_id, uint32_t slot_id, int srgb, uint8_t *host_rgba8); /* :93-95 */
/* buffer_rgba into device memory in any kc_device_image form (see kc_image_to_device) */
KC_API int kc_live_graph_buffer_device(kc_live_graph *lg, uint32_t node_id, uint32_t slot_id, const kc_device_image *dst, uint32_t flags,
                                       void *hip_stream);
/* kc_image_channel_stats of a slot's image */
KC_API int kc_live_graph_buffer_channel_stats(kc_live_graph *lg, uint32_t node_id, uint32_t slot_id, uint32_t flags,
                                              kc_channel_stats *out);
KC_API int kc_live_graph_buffer_bc(kc_live_graph *lg, uint32_t node_id, uint32_t slot_id, const kc_bc_image *dst,
                                   uint32_t flags, void *hip_stream); /* kc_image_to_bc_device of a slot's image */
KC_API int kc_live_graph_buffer_bc_mips(kc_live_graph *lg, uint32_t node_id, uint32_t slot_id, int format, uint32_t flags,
                                        void *device_ptr, size_t bytes, void *hip_stream); /* kc_image_to_bc_mips_device likewise */
KC_API int kc_live_graph_buffer_bc_error(kc_live_graph *lg, uint32_t node_id, uint32_t slot_id, int format, uint32_t flags,
                                         kc_bc_error *out); /* kc_image_bc_error of a slot's image */
KC_API int kc_live_graph_embed_slot_data_with_id(kc_live_graph *lg, kc_image *image, uint32_t slot_id, uint32_t embed_id); /* :324-341 */
KC_API int kc_live_graph_add_input_slot_data(kc_live_graph *lg, uint32_t node_id, uint32_t slot_id, kc_image *image);     /* :347-350 */
KC_API int kc_live_graph_changed_consume(kc_live_graph *lg, uint32_t *ids, uint32_t cap, uint32_t *count);               /* :156-160 */
KC_API int kc_live_graph_output_ids(const kc_live_graph *lg, uint32_t *ids, uint32_t cap, uint32_t *count);              /* :621-623 */
KC_API int kc_live_graph_node_ids(const kc_live_graph *lg, uint32_t *ids, uint32_t cap, uint32_t *count);                /* :629-631 */
KC_API int kc_live_graph_edges(const kc_live_graph *lg, kc_edge *edges, uint32_t cap, uint32_t *count);                  /* :633-635 */
/* Base directory that relative Image / Write paths resolve against (the reference resolves them
 * against the process's working directory). */
KC_API int kc_live_graph_set_base_dir(kc_live_graph *lg, const char *dir);

/* ========================================================================================== *
 * Multi-GPU: one process per GPU, every process holds the same graph.  The reference runs every ready
 * node on its own thread and needs nothing but the parents' slot data to do so (src/engine.rs:213-275,
 * :288); here the same rule lets independent branches run on different GPUs.  kc_live_graph_partition
 * derives, from the graph alone (so every rank computes the same answer without communicating), which rank
 * evaluates which ancestor of `root` and which slots cross a rank boundary -- or that every rank takes a band of rows.  The
 * library moves the slots itself (kc_comm_*, kc_live_graph_evaluate_partitioned below); a host with a transport of its own
 * can do it through kc_plane_device_ptr / kc_plane_alloc + kc_image_gray / kc_image_rgba and kc_live_graph_import_slot_data.
 * INTEGRATION.md shows both.
 * ========================================================================================== */
typedef enum kc_partition_policy {
    KC_PARTITION_AUTO = 0,   /* the cheapest of {one GPU, branches with transfers charged, row bands + gather of the result},
                              * priced in one unit (one RGBA 4096^2 slot over xGMI ~ 12 fused Mix chains): small graphs stay
                              * on one GPU, wide pointwise graphs (BASELINE config #4) go by rows */
    KC_PARTITION_SPREAD = 1, /* branches, transfers not charged: independent branches fill all ranks */
    KC_PARTITION_BANDS = 2   /* row bands (KC_ERR_UNSUPPORTED when the band walk does not take the graph or the sources'
                              * sizes are not known yet) */
} kc_partition_policy;
typedef enum kc_plan_kind {
    KC_PLAN_SINGLE = 0,   /* everything on the home rank, nothing moves */
    KC_PLAN_BRANCHES = 1, /* nodes placed per rank, `transfers` cross rank boundaries */
    KC_PLAN_BANDS = 2     /* every rank evaluates rows [y0, y1) of the requested node (kc_partition_bands); the pointwise
                           * nodes (src/node/mix.rs:136-192) need no exchange at all, the finished bands are gathered on the
                           * home rank unless kc_partition_set_gather(plan, 0) */
} kc_plan_kind;
typedef struct kc_band_range { int32_t y0, y1; } kc_band_range;
typedef enum kc_node_kind {
    KC_KIND_SOURCE = 0,     /* Embed / Image / Input*: data somebody put there; lives on `rank` */
    KC_KIND_REPLICATED = 1, /* no source among its ancestors (Value nodes and constants built from them):
                             * evaluated on every rank that needs it, never sent; rank = -1 */
    KC_KIND_COMPUTE = 2     /* evaluated on `rank` only */
} kc_node_kind;
typedef struct kc_placement { uint32_t node_id; int32_t rank; int32_t component; int32_t kind; } kc_placement;
/* One slot moving from the rank that produced it to ONE consumer rank; a slot consumed on several ranks (a
 * broadcast) appears once per destination, consecutively.  Transfers are listed in the order every rank must
 * work through them; `level` = how many rank boundaries the data has crossed before (0 for branch results). */
typedef struct kc_transfer { uint32_t node_id, slot_id; int32_t src_rank, dst_rank; int32_t level; } kc_transfer;
KC_API int kc_live_graph_partition(kc_live_graph *lg, uint32_t root_node_id, int world_size, int policy, kc_partition **out);
KC_API int kc_partition_free(kc_partition *p);
KC_API int kc_partition_info(const kc_partition *p, int *world_size, int *home_rank, int *levels);
/* Ancestors of the root (root included) in topological order, with their placement. */
KC_API int kc_partition_nodes(const kc_partition *p, kc_placement *out, uint32_t cap, uint32_t *count);
KC_API int kc_partition_transfers(const kc_partition *p, kc_transfer *out, uint32_t cap, uint32_t *count);
/* Which of the three a plan is, and what KC_PARTITION_AUTO compared (estimated times in units of one fused RGBA Mix chain over
 * the image; `bands` < 0: no band plan exists).  Any of the out pointers may be NULL. */
KC_API int kc_partition_kind(const kc_partition *p, int *kind, double *est_single, double *est_branches, double *est_bands);
/* KC_PLAN_BANDS: the rows of the requested node per rank (`count` = world size) and the node's full size.  A rank holds the rows
 * kc_live_graph_band_source_rows names for its band of every source (kc_live_graph_embed_slot_data_band), or whole sources. */
KC_API int kc_partition_bands(const kc_partition *p, kc_band_range *out, uint32_t cap, uint32_t *count, uint32_t *full_width, uint32_t *full_height);
/* KC_PLAN_BANDS: gather = 0 leaves every rank's band where it is (kc_live_graph_evaluate_partitioned then returns the band on
 * every rank); the default, 1, assembles the image on the home rank. */
KC_API int kc_partition_set_gather(kc_partition *p, int gather);
/* Stores `image` (+1 ref) as slot `slot_id` of `node_id` and marks the node Clean, exactly as the engine does with
 * the result of a finished node (src/engine.rs:34-57): the receiving side of a transfer. */
KC_API int kc_live_graph_import_slot_data(kc_live_graph *lg, uint32_t node_id, uint32_t slot_id, kc_image *image);

/* The exchange itself, inside the library (csrc/comm.cpp): the slots a branch plan cuts, and the finished bands of a band plan,
 * move between the processes of one node.  Descriptions of slots (size; constant planes travel as scalars, aliased planes once)
 * go through a shared-memory mailbox, host to host; the planes go over one of two wires, chosen by rank 0 when it makes the id
 * (environment KC_COMM_TRANSPORT):
 *   "ipc" (default)  the consumer maps the producer's planes (hipIpcOpenMemHandle), one stream per peer waits ON THE DEVICE for a
 *                    counter the producer's stream writes behind its kernels, copies (hipMemcpyAsync: the DMA engines over xGMI)
 *                    and acknowledges the same way; works between processes sharing one GPU too;
 *   "rccl"           ncclSend / ncclRecv, all transfers of a level in one group (librccl bound at first use; a process that never
 *                    asks for it needs no RCCL).
 * No host thread waits for plane data with either.  One communicator per process:
 *   kc_comm_unique_id   rank 0 fills `id` (KC_COMM_ID_BYTES); the host passes it to every rank by whatever channel it has
 *                       (a file, a pipe, MPI, torch.distributed's store ...);
 *   kc_comm_init        collective over all ranks (at most 16), after kc_init; a failure is a status (nothing is retried);
 *   kc_live_graph_exchange  works through `transfers` level by level -- every rank passes the same list, e.g. what
 *                       kc_partition_transfers returns; transfers of one level must not depend on each other.  Per level the
 *                       producer's rank evaluates the node (kernels enqueued, nobody waits) and posts the description; a
 *                       consumer's rank allocates planes, receives into them and hands the slot over exactly as
 *                       kc_live_graph_import_slot_data does, its compute stream waiting for the transfer on the device.
 *                       Consecutive entries of one slot are one multi-destination send.  An entry from a rank to itself is legal
 *                       (the slot is replaced by the copy that came back).
 *   kc_comm_gather_bands  every rank passes its band (rows y0 .. of an image `full_height` rows high, e.g. what
 *                       kc_live_graph_evaluate_band returned); on `home_rank`, `*out` (+1 ref) is the assembled image (the
 *                       bands must tile it), NULL elsewhere.  Each band travels over its own link, straight to its row offset.
 *   kc_live_graph_evaluate_partitioned  the whole evaluation of a plan: KC_PLAN_SINGLE / KC_PLAN_BRANCHES -- what this rank can
 *                       compute before anything arrives is enqueued first (it overlaps the transfers), then the exchange, then
 *                       `root` on the plan's home rank: `*out` (+1 ref) is the root's result there and NULL on the other ranks;
 *                       KC_PLAN_BANDS -- this rank's rows of `root`, then the gather (or, after kc_partition_set_gather(plan, 0),
 *                       `*out` = the band on every rank).
 * Any failure on any rank makes every host-side wait of every rank fail (they also time out: KC_COMM_TIMEOUT_S seconds, default
 * 120); the communicator is unusable afterwards.  The readiness rule that makes all this correct is the reference's: a node needs
 * nothing but its parents' slot data (src/engine.rs:213-275). */
#define KC_COMM_ID_BYTES 256
KC_API int kc_comm_unique_id(void *id);
KC_API int kc_comm_init(int rank, int world_size, const void *id);
KC_API int kc_comm_destroy(void);
KC_API int kc_comm_info(int *rank, int *world_size);  /* 0, 0 without a communicator */
KC_API int kc_comm_transport(char *buf, size_t cap);  /* "ipc", "rccl" or "" */
KC_API int kc_comm_stats(uint64_t *planes_sent, uint64_t *planes_received, uint64_t *bytes_sent);
KC_API int kc_live_graph_exchange(kc_live_graph *lg, const kc_transfer *transfers, uint32_t count);
KC_API int kc_comm_gather_bands(kc_image *band, int32_t y0, uint32_t full_height, int home_rank, kc_image **out);
KC_API int kc_live_graph_evaluate_partitioned(kc_live_graph *lg, const kc_partition *plan, uint32_t root_node_id, kc_image **out);

/* Row bands: rows [y0, y1) of a node's result without computing the rest -- the data-level way to put several GPUs on one
 * graph.  Every pixel goes through the same operations as in the whole-image evaluation (process_node, src/node/
 * node_type.rs:213-248), so the bands of all ranks, stacked, equal it bit for bit.  Pointwise nodes need the same rows
 * of their inputs; HeightToNormal one more row on top (toroidal: the band that starts at row 0 needs the LAST row,
 * src/node/process_shared.rs:31-65); an implicit resize the rows its vertical taps read (src/shared.rs:159-199).  The
 * evaluation widens every intermediate band by those halo rows and computes them redundantly: no exchange between ranks.
 * Graph nodes (src/node/graph.rs:14-51) are expanded into their graphs before the walk (the resize the Graph node applies to
 * its inputs becomes a SpecificSize pass-through in front of every inner Input node), nested ones too; Write nodes are
 * not supported here.
 *   kc_live_graph_evaluate_band: `*out` (+1 ref) is an image of (y1 - y0) rows, resident on return.
 *   kc_live_graph_band_source_rows: which rows of every SOURCE (Embed / Image / Input*) that evaluation reads, so that
 *     sources which are themselves sharded by rows can be loaded with exactly their halo.  y0 may be negative: row -1 is
 *     the image's last row (the wrap).  Host only, no device needed.
 *   kc_live_graph_embed_slot_data_band: like kc_live_graph_embed_slot_data_with_id, but `image` holds only logical rows
 *     band_y0 .. band_y0 + rows - 1 of an image `full_height` rows high (band_y0 < 0: the wrapped rows come first). */
typedef struct kc_band_rows { uint32_t node_id; int32_t y0, y1; uint32_t width, height; } kc_band_rows;
KC_API int kc_live_graph_evaluate_band(kc_live_graph *lg, uint32_t node_id, uint32_t slot_id, int32_t y0, int32_t y1, kc_image **out);
KC_API int kc_live_graph_band_source_rows(kc_live_graph *lg, uint32_t node_id, int32_t y0, int32_t y1, kc_band_rows *rows, uint32_t cap, uint32_t *count);
KC_API int kc_live_graph_embed_slot_data_band(kc_live_graph *lg, kc_image *image, uint32_t slot_id, uint32_t embed_id, int32_t band_y0, uint32_t full_height);

#ifdef __cplusplus
}
#endif
#endif /* KANTER_CORE_AMD_H */
