// Internal declarations shared by the HIP kernels (the .hip files, one per kernel family) and the host runtime.
// Not part of the C ABI (include/kanter_core_amd.h).
//
// The kernels are hand-written CDNA4 (gfx950) code for the kanter_core per-pixel hot path.
// All of these are HBM-bandwidth-bound pointwise / small-stencil kernels: 16-byte (dwordx4)
// coalesced row-major accesses on 256-byte-pitched f32 planes, 64-wide wavefronts, no MFMA.
// Build flags that matter for parity with the reference's scalar Rust loops:
//   -ffp-contract=off                         no FMA contraction (Rust never fuses a*b+c)
//   -fhip-fp32-correctly-rounded-divide-sqrt  IEEE f32 divide / sqrt
//   f32 denormals are not flushed (gfx9 default)
// Reference paths are relative to the reference checkout.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/kanter_core_amd.h"
#include "preview_walk.h"  // PreviewJob and the index arithmetic of preview.hip / preview.cpp (namespace kc; compiles without HIP too)

namespace kc {

#include "chain_program.h"  // ChainCode, ChainStepRec / ChainStepPair, ChainProgram
#include "upsample.h"       // UpAxis, UpsampleArgs

// The A/B and tuning switches, one field per row of the option table (c_api.cpp, kOptions).  Their defaults, accepted values
// and meaning are listed at kc_set_option (include/kanter_core_amd.h).  Context owns the instance; options() reads it.
struct Options {
    int chain1, replay, join, wide, fusion, down2, down2_by_rows, poly2, poly2_min_ratio, resize_mode, resize_tile_w, resize_tile_h;
    int poly_rows, poly2_xcd, down2_xcd, h2n_tiled, cache_policy, cache_budget_mb, nt_force, chain_unroll, max_blocks, tune_cap;
    int upload_ring, link_gbps, hbm_gbps;
};
Options option_defaults();
const Options &options();

// Per-axis tap table of the separable resampler, resident in HBM.
struct TapsDev {
    const uint32_t *left;
    const uint32_t *count;
    const float *w;
    uint32_t stride;
};

// Pointwise operand: a pitched plane or a broadcast constant.
struct Operand {
    const float *ptr;  // nullptr => constant
    uint32_t pitch;    // in floats
    float c;
};

// ---- kernel launchers, by the unit that defines them.  All enqueue on `s` and return hipGetLastError(). ----
// -- chain.hip --
// What launch_chain launched (runtime.cpp counts it: kc_stats_counter): chain_kernel<k, u, mode, nt>, or
// chain_kernel_k0<mode> for k = 0; k < 0: nothing (an empty plane)
struct ChainVariant {
    int k = -1, u = 0, mode = 0;
    bool nt = false;
};
// mode: 0 = {+, -, *} only, 1 = + divide, 2 = + pow
hipError_t launch_chain(const ChainProgram &p, int batch, int mode, int max_blocks, int unroll, hipStream_t s, ChainVariant *var);
inline uint32_t chain_op_word(uint8_t code, int src) { return (uint32_t)code | ((uint32_t)(src + 1) << 8); }
hipError_t launch_fill(float *dst, uint32_t pitch_floats, uint32_t w, uint32_t h, float v, hipStream_t s);
// -- chain1.hip --
// A one-step program for the ahead-of-time kernels of chain1.hip: result = op(start, operand), each a plane (pointer,
// pitch in float4) or a broadcast constant (pointer null); c = the constant of the fused "c - ..." codes.
struct Chain1Args {
    const float *start[KC_CHAIN_MAX_BATCH], *operand[KC_CHAIN_MAX_BATCH];
    float *out[KC_CHAIN_MAX_BATCH];
    uint32_t start_pitch[KC_CHAIN_MAX_BATCH], operand_pitch[KC_CHAIN_MAX_BATCH], out_pitch[KC_CHAIN_MAX_BATCH];
    float start_c[KC_CHAIN_MAX_BATCH], operand_c[KC_CHAIN_MAX_BATCH], c[KC_CHAIN_MAX_BATCH];
    uint32_t row_units, rows;
};
// nt: bit 0 = the start plane, bit 1 = the operand plane, bit 2 = the result carry the nontemporal hint.
// *launched_nt: the bits of the instantiation launched (left alone when nothing is launched: an empty plane)
hipError_t launch_chain1(const Chain1Args &a, int batch, int code, unsigned nt, hipStream_t s, unsigned *launched_nt);
// -- the resamplers: LDS sizes, the kernels' job tables and the plan that the launchers of resize_tile.hip, resize_down.hip,
// down2.hip and upsample.hip take --
// Tiled single-pass resample.  ncp = LDS pitch in floats of the vertical-pass intermediate: a multiple
// of 4 that covers the widest 4-aligned source window any tile needs (from the host).  The 8 spare
// floats absorb the register-tap form's reads past a short window (discarded, see resize_out_row);
// the tile rows' vertical tap table follows.
// Windows of more than KC_RESIZE_REG_TAPS horizontal taps also keep the tile's horizontal tap table there.
constexpr uint32_t KC_RESIZE_REG_TAPS = 8;
inline size_t resize_lds_bytes(uint32_t tile_h, uint32_t ncp, uint32_t v_stride, uint32_t tile_w, uint32_t h_stride)
{
    // the wide form pads its intermediate rows (one float after every 32, see resize_wide_kernel)
    const size_t row = h_stride > KC_RESIZE_REG_TAPS ? (size_t)ncp + (ncp >> 5) + 1u : ncp;
    size_t n = (size_t)tile_h * row + 8u + 2u * tile_h + (size_t)tile_h * v_stride;
    if (h_stride > KC_RESIZE_REG_TAPS) n += 2u * tile_w + (size_t)tile_w * h_stride;
    return n * sizeof(float);
}
// resize_down_kernel / resize_poly_kernel: intermediate rows of a fixed pitch (a window of at most 256 floats, one float of
// padding after every 32), then the tile's horizontal taps at an odd pitch
#define KC_DOWN_ROW_FLOATS 265u
inline size_t resize_down_lds_bytes(uint32_t tile_h, uint32_t ncp, uint32_t tile_w, uint32_t h_stride)
{
    (void)ncp;  // <= 256 (host-checked)
    return ((size_t)tile_h * KC_DOWN_ROW_FLOATS + 2u * tile_w + (size_t)tile_w * (h_stride | 1u)) * sizeof(float);
}
// Up to 4 planes of equal size (the planes of one image) resampled by one launch, blockIdx.z = plane.
struct ResizePlanes {
    const float *src[4];
    float *dst[4];
    uint32_t spitch[4], dpitch[4];  // in floats
};
// resize_down2_kernel (down2.hip): the wave-private form of down-sampling on both axes.
//   vrec     per group of 4 output rows `nc` records of KC_DOWN2_REC dwords: [0] first source row of the chunk, [1], [2] presence
//            mask of tap (source row u, output row k) at bit 4 u + k, [3] the group's last window row (loads are clamped to
//            it), [4] chunks this group uses, [5] the same in half chunks of 8 rows, [8 + 4 u + k] the weight (resize.cpp, down2_build)
//   hw       the horizontal table's weights, rows padded to hstride (a multiple of 4) floats
//   strips   per strip of tile_w output columns: its first source column rounded down to a multiple of 4, and the width of its
//            source window in column quads (<= 64: one per lane of the vertical pass)
constexpr uint32_t KC_DOWN2_REC = 72, KC_DOWN2_MAX_CHUNKS = 4, KC_DOWN2_SLOTS = 256 + 32;
struct Down2Args {
    const uint32_t *vrec;
    const uint32_t *hleft, *hcount, *strips;
    const float *hw;
    uint32_t nc, hstride;
    uint32_t tile_w, dw, dh;
    // XCD-aware tile order (down2.hip): xcd_per != 0 makes the grid one-dimensional (xcd_per = 0: plain 2-D grid)
    uint32_t xcd_per, n_tiles, gy, gy_magic;
    // by_rows != 0: a workgroup's four waves are four neighbouring STRIPS of one row group and XCD k works through the k-th eighth
    // of the jobs row by row (xcd_per workgroups each; gy / gy_magic then divide by the number of strips): see resize_poly_kernel
    uint32_t by_rows;
};
// output columns per lane of the horizontal pass: its weights live in registers (at most 9 quads per lane)
inline uint32_t down2_cols_per_lane(uint32_t weight_quads) { return weight_quads <= 3 ? 3u : weight_quads == 4 ? 2u : 1u; }
// Tiles in XCD order (as resize_down2_kernel's): with per != 0 the grid is one-dimensional, workgroup id % 8 is the XCD and XCD k
// works through the k-th eighth of the gx x gy tiles in column-major order (tile = (id % 8) * per + id / 8; x = tile / gy), so
// that vertically adjacent tiles, which share source rows, meet in one L2.
struct XcdOrder {
    uint32_t per, n, gy, magic;
};
inline XcdOrder xcd_order(uint32_t gx, uint32_t gy, bool want)
{
    XcdOrder o{ 0, 0, 0, 0 };
    if (!want || gy < 2) return o;
    const uint64_t n = (uint64_t)gx * gy, magic = ((1ull << 32) + gy - 1) / gy;
    // tile / gy == (tile * magic) >> 32 for every tile < n when n * (magic * gy - 2^32) < 2^32
    if (n >= (1u << 24) || n * (magic * gy - (1ull << 32)) >= (1ull << 32)) return o;
    o.per = (uint32_t)((n + 7) / 8);
    o.n = (uint32_t)n;
    o.gy = gy;
    o.magic = (uint32_t)magic;
    return o;
}
// LDS floats of one band wave of resize_poly_kernel (resize_down.hip, resize_down_stage_wave)
inline uint32_t resize_down_wave_floats(uint32_t tile_w, uint32_t hstride) { return (4u * KC_DOWN_ROW_FLOATS + 2u * tile_w + tile_w * (hstride | 1u) + 3u) / 4u * 4u; }
// resize_poly_kernel's jobs (resize_down.hip)
struct PolyBands {
    uint32_t ya, yb;    // regular rows handled as bands: [ya, yb), yb - ya a multiple of 4
    uint32_t rows;      // rows per band (a multiple of 4; the last band may be shorter)
    uint32_t n_bands;
    uint32_t ty0[4], th[4];  // general tiles: first row, rows (<= 16)
    // A workgroup's four waves are four neighbouring STRIPS of one band (each with its taps staged by itself); the grid is
    // one-dimensional and XCD k (workgroup id % 8) works through the k-th eighth of the band workgroups band by band; the
    // border tiles follow.  n_sq strip quads per band, n_band_wgs = n_bands * n_sq, xper = ceil(n_band_wgs / 8), gx strips,
    // wave_floats of LDS per wave.
    uint32_t n_sq, n_band_wgs, xper, gx, wave_floats;
};
// resize_poly2_kernel's jobs (resize_down.hip)
struct Poly2Bands {
    uint32_t ya, yb, rows, n_bands;
    uint32_t tw, n_strips;     // band path: output columns per strip (its source window is at most 256 columns), strips per row
    uint32_t n_wgx;            // workgroups per band (two strips each)
    uint32_t n_band_wgs;       // n_wgx * n_bands; the general tiles follow
    uint32_t gen_tw, gen_gx, gen_ncp;  // general tiles: resize_down_kernel's strip width, strips per row, padded window
    uint32_t n_gen;
    uint32_t ty0[6], th[6];
};
#define KC_POLY2_RING_PITCH 265u  // 256 columns + one pad per 32, odd

// How one resample runs, as plan_resample (resize.cpp) decides it on the host from the two tap tables, the sizes and the
// options: the form, and everything its launcher needs besides the planes (or the chain program), the tables' device pointers
// and the stream.
// Form X runs X_kernel or resize_X_kernel; none: a fused request that is not eligible (the resample runs on its own); two_pass:
// launch_resize_vertical, then launch_resize_horizontal through an HBM intermediate, plane by plane.
enum class ResizeForm { none, upsample, upsample_chain, resize_chain, poly2, down2, poly, down, lds, wide, two_pass };
struct ResizePlan {
    ResizeForm form = ResizeForm::none;
    uint32_t sw = 0, sh = 0, dw = 0, dh = 0;   // source and result size
    int planes = 0;                            // planes (the chain's batch) of the launch: blockIdx.z
    uint32_t tile_w = 0, tile_h = 0, ncp = 0;  // the tiled forms' tile (poly2: the border tiles')
    uint32_t mint = 0, maxt = 0;               // lds: resize_lds_kernel<MINT, MAXT>
    uint32_t ages = 0, ratio = 0;              // poly, poly2: <A, RT>
    uint32_t n_border = 0;                     // poly, poly2: border tiles the rows take (more than the bands hold: refused)
    PolyBands poly{};
    Poly2Bands poly2{};
    uint32_t pair_floats = 0;  // poly2: LDS floats of a pair of waves
    XcdOrder xcd{};            // poly2: the job order
    Down2Args d2{};            // down2: all but the table pointers
    UpsampleArgs up{};         // upsample, upsample_chain
    bool nt = false;           // upsample: nontemporal stores of the results (cache_policy_mask)
    size_t lds = 0;            // dynamic LDS bytes
    dim3 grid{};
};
// The launchers of the planned forms: they check the plan and pick the kernel template, nothing else.
// -- resize_tile.hip --
hipError_t launch_resize_lds(const ResizePlan &r, const ResizePlanes &p, TapsDev v, TapsDev h, hipStream_t s);  // lds, wide
// Fused resample + chain: input slot n_in - 1 of the program is produced by the resampler.
hipError_t launch_resize_chain(const ResizePlan &r, const ChainProgram &p, TapsDev v, TapsDev h, hipStream_t s);
// The two-pass form, one plane per call.
hipError_t launch_resize_vertical(const float *src, uint32_t spitch, uint32_t sw, float *tmp, uint32_t tpitch,
                                  uint32_t dh, TapsDev v, hipStream_t s);
hipError_t launch_resize_horizontal(const float *tmp, uint32_t tpitch, float *dst, uint32_t dpitch, uint32_t dw,
                                    uint32_t dh, TapsDev h, hipStream_t s);
// -- resize_down.hip --
hipError_t launch_resize_down(const ResizePlan &r, const ResizePlanes &p, TapsDev v, TapsDev h, hipStream_t s);
hipError_t launch_resize_poly(const ResizePlan &r, const ResizePlanes &p, TapsDev v, TapsDev h, hipStream_t s);
// The same ranges with two waves to a band's strip (8-byte lanes, a shared ring, the horizontal pass split by pixels)
hipError_t launch_resize_poly2(const ResizePlan &r, const ResizePlanes &p, TapsDev v, TapsDev h, hipStream_t s);
// -- down2.hip --
// a: the plan's d2 with the tables' pointers
hipError_t launch_resize_down2(const ResizePlan &r, const ResizePlanes &p, const Down2Args &a, hipStream_t s);
// -- upsample.hip --
// Integer-ratio up-sampling (upsample.h).  A workgroup's tile: tile_w columns x KC_UPSAMPLE_ROWS * (1024 / tile_w) rows
// (every thread 4 columns x KC_UPSAMPLE_ROWS rows, one trip).  LDS: the tile's intermediate, then the H quad classes.
#ifdef KC_UP_RU  // tuning builds (tools/build_variant.sh)
constexpr uint32_t KC_UPSAMPLE_ROWS = KC_UP_RU;
#else
constexpr uint32_t KC_UPSAMPLE_ROWS = 4;
#endif
inline uint32_t upsample_tile_rows(const UpsampleArgs &u) { return KC_UPSAMPLE_ROWS * (1024u / u.tile_w); }
inline size_t upsample_lds_bytes(const UpsampleArgs &u)
{
    return ((size_t)upsample_tile_rows(u) * u.ncp + (size_t)(std::max(u.H.ratio >> 2, 1u) + u.H.qb_lo + u.H.qb_hi) * 4u * u.H.taps) * sizeof(float);
}
inline bool upsample_args_ok(const UpsampleArgs &u, int batch)
{
    if (batch < 1 || batch > 4) return false;
    if (u.tile_w % 4 != 0 || u.tile_w == 0 || u.tile_w > 1024 || 256u % (u.tile_w / 4) != 0) return false;
    const uint32_t tile_h = upsample_tile_rows(u);
    if (u.chunk == 0 || tile_h % u.chunk != 0 || u.V.ratio % u.chunk != 0) return false;
    if (u.H.ratio % 4 != 0 && !(u.H.ratio == 2 && u.H.n_out % 4 == 0)) return false;
    if (u.H.taps != u.V.taps || u.ncp % 4 != 0 || !u.H.qcls || !u.V.cls) return false;
    if (u.H.n_out > 65535 || u.V.n_out > 65535) return false;  // up_div
    if (u.ncp / 4 > 257 || (std::max(u.H.ratio >> 2, 1u) + u.H.qb_lo + u.H.qb_hi) * u.H.taps > 256) return false;
    return upsample_lds_bytes(u) <= 64 * 1024;
}
inline dim3 upsample_grid(const UpsampleArgs &u, int batch)
{
    const uint32_t tile_h = upsample_tile_rows(u);
    return dim3((u.H.n_out + u.tile_w - 1) / u.tile_w, (u.V.n_out + tile_h - 1) / tile_h, batch);
}
// The plane members of ChainProgram that the plain up-sampling kernel reads (K = 1: no resident inputs).
struct UpsamplePlanes {
    const float *samp_src[4];
    unsigned int samp_pitch[4];  // floats
    float *out[4];
    unsigned int out_pitch[4];  // float4 units
    const float *in[4][1];
    unsigned int in_pitch[4][1];
    unsigned int nt_mask;  // bit 8: nontemporal stores (ChainProgram::nt_mask)
};
hipError_t launch_upsample_chain(const ChainProgram &p, int batch, const UpsampleArgs &u, hipStream_t s);
hipError_t launch_upsample(const UpsamplePlanes &p, int batch, const UpsampleArgs &u, hipStream_t s);
// -- h2n.hip --
// What launch_height_to_normal launched (ops.cpp counts it: kc_stats_counter): height_to_normal_kernel<band, nt, tq != 0>
// with tiles of 2^tq quads (tq = 0: the plain mapping); launched = false: nothing (an empty plane)
struct H2nVariant {
    bool launched = false, band = false, nt = false;
    uint32_t tq = 0;
};
// nt_mask: the launch's cache policy as cache_policy_mask() returns it (bits 0-7: inputs, bit 8: results)
hipError_t launch_height_to_normal(const float *hgt, uint32_t hpitch, uint32_t w, uint32_t h, uint32_t full_h, int band,
                                   float *nx, float *ny, float *nz, uint32_t opitch, uint32_t nt_mask, hipStream_t s, H2nVariant *var);
// -- u8.hip --
// *launched_nt (here and in devimage.hip's launchers): whether the instantiation launched is the nontemporal one (left alone
// when nothing is launched: an empty image)
hipError_t launch_to_u8(Operand r, Operand g, Operand b, Operand a, int gray, int srgb, uint32_t w, uint32_t h,
                        uint8_t *dst, uint32_t nt_mask, hipStream_t s, bool *launched_nt);
hipError_t launch_from_u8(const uint8_t *src, int channels, uint32_t w, uint32_t h, float *const planes[4],
                          uint32_t pitch, uint32_t nt_mask, hipStream_t s, bool *launched_nt);
// -- chain_pack.hip --
// The pack pass of one tier (chain_pack.h): `quads` float4 of the dense plane `src` into `dst`, pack_bytes_per_quad(tier) each;
// *flag (device memory, cleared by the caller) is set to 1 if any sample does not decode back to its own bit pattern.
hipError_t launch_pack_plane(uint32_t tier, const float *src, void *dst, uint64_t quads, uint32_t *flag, hipStream_t s);
// -- devimage.hip --
// Device-memory images (devimage.hip / devimage.cpp): a validated kc_device_image as the kernels take it.  vec != 0: the pointer
// and the pitches are aligned for the widest access of a whole pixel quad (devimage.cpp, devimage_vec).
struct DevImageArgs {
    const char *ptr;
    uint64_t row_pitch, channel_pitch;  // bytes
    uint32_t w, h;
    int channels, layout;  // 1..4, kc_layout
    int vec;
};
// image_import_kernel: the first `channels` planes of `planes` are written (pitch in floats); nt_mask bit 8: nontemporal stores
hipError_t launch_image_import(int dtype, const DevImageArgs &a, float *const planes[4], uint32_t ppitch, uint32_t nt_mask, hipStream_t s,
                               bool *launched_nt);
// image_export_kernel: channel c of the output is op[c]; gray != 0: op[0] stands for R, G and B (read once); nt_mask bits 0-7:
// nontemporal plane loads; srgb: U8 only
hipError_t launch_image_export(int dtype, int srgb, const Operand op[4], int gray, const DevImageArgs &a, uint32_t nt_mask, hipStream_t s,
                               bool *launched_nt);
// -- stats.hip --
// Per-channel statistics (stats.hip / stats.cpp): the n distinct resident planes ("slots") of one image.  Bit s of srgb: slot
// s bins with the sRGB quantiser.  partials: one record of rec_words u32 per workgroup (stats.hip has the layout); result:
// rec_words u64, initialised by the launch itself.
struct StatsArgs {
    const float *ptr[4];
    uint32_t pitch[4];  // floats
    uint32_t w, h, n, srgb;
    uint32_t *partials;
    uint32_t rec_words;
    unsigned long long *result;
};
// channel_stats_kernel<nt, hist, srgb> on `groups` workgroups, then channel_stats_combine_kernel: two launches
hipError_t launch_channel_stats(const StatsArgs &a, bool hist, bool srgb, bool nt, uint32_t groups, hipStream_t s);
// workgroups of that launch for a w x h image on a device of `cus` CUs (>= 1)
uint32_t channel_stats_groups(uint32_t w, uint32_t h, bool hist, bool srgb, uint32_t cus);
// -- bc.hip --
// The launchers of the block-compression units.  The host calls them through bc.cpp's bc_launch_encode / _decode / _compare, which
// pick the unit of a format; the units share their loops through bc_blocks.h.
// Block compression (bc.hip / bc.cpp): bc_encode_kernel<fmt, srgb, nt> writes the ceil(w/4) x ceil(h/4) blocks of format `fmt`
// (kc_bc_format) at dst, block rows row_pitch bytes apart; channel c is op[c]; gray != 0: op[0] stands for R, G and B (read
// once); nt_mask bits 0-7: nontemporal plane loads; srgb: BC1 and BC3 only
hipError_t launch_bc_encode(int fmt, int srgb, const Operand op[4], int gray, char *dst, uint64_t row_pitch, uint32_t w, uint32_t h,
                            uint32_t nt_mask, hipStream_t s);
// -- bc1a.hip --
// KC_BC_PUNCH_THROUGH: bc1a_encode_kernel<srgb, nt>, BC1 blocks of an RGBA image whose texels with an alpha byte below `ref`
// (1..255) decode transparent; bc1a_compare_kernel<srgb, nt> then bc_combine_kernel, launch_bc_compare's record under the flag
hipError_t launch_bc1a_encode(int srgb, const Operand op[4], uint32_t ref, char *dst, uint64_t row_pitch, uint32_t w, uint32_t h, uint32_t nt_mask,
                              hipStream_t s);
hipError_t launch_bc1a_compare(int srgb, const Operand op[4], uint32_t ref, const char *blocks, uint64_t row_pitch, uint32_t w, uint32_t h,
                               uint32_t nt_mask, uint32_t groups, unsigned long long *partials, unsigned long long *result, hipStream_t s);
// -- bc7.hip --
// bc7_encode_kernel<srgb, nt>: the same for KC_BC7 (16-byte blocks, all four channels)
hipError_t launch_bc7_encode(int srgb, const Operand op[4], int gray, char *dst, uint64_t row_pitch, uint32_t w, uint32_t h, uint32_t nt_mask,
                             hipStream_t s);
// -- bc_decode.hip --
// Block decode and the error of an encoding (bc_decode.hip / bc_decode.cpp).  bc_decode_kernel<fmt, nt, count> reads the
// ceil(w/4) x ceil(h/4) blocks at src, block rows row_pitch bytes apart, and writes the planes the format holds (BC4: dst[0];
// BC5: dst[0..1]; the others dst[0..3]), dst_pitch floats between their rows, rows 16-byte aligned; nt_mask bit 8: nontemporal.
struct BcDecodeArgs {
    const char *src;
    uint64_t row_pitch;  // bytes between block rows
    float *dst[4];
    uint32_t dst_pitch;  // floats
    uint32_t w, h, bx, by;
    unsigned long long *partials, *result;  // count: one word per workgroup, and the sum (bc_combine_kernel: a second launch)
};
// count: result[0] = the blocks of the modes that are not decoded, by a second launch (bc_combine_kernel).  Of this unit's formats
// only KC_BC7 has such modes (the partitioned ones) and takes count; the host asks for a count where its format table says the
// format counts, that is for KC_BC7 here and for KC_BC6H through launch_bc6h_decode
hipError_t launch_bc_decode(int fmt, const BcDecodeArgs &a, bool count, uint32_t nt_mask, uint32_t groups, hipStream_t s);
uint32_t bc_decode_groups(uint32_t w, uint32_t h, bool count);
// bc_compare_kernel<fmt, srgb, nt> on `groups` workgroups, then bc_combine_kernel: two launches.  The image's channels as
// launch_bc_encode takes them against the blocks at `blocks`; partials: groups records of KC_BC_REC_WORDS u64 (bc_decode.hip has
// the layout); result: one record, every word written.
constexpr uint32_t KC_BC_REC_WORDS = 17;
hipError_t launch_bc_compare(int fmt, int srgb, const Operand op[4], int gray, const char *blocks, uint64_t row_pitch, uint32_t w, uint32_t h,
                             uint32_t nt_mask, uint32_t groups, unsigned long long *partials, unsigned long long *result, hipStream_t s);
uint32_t bc_compare_groups(uint32_t w, uint32_t h);
// bc_combine_kernel alone, for the records of another unit's kernels: result[col] = the sum (max_cols bit col set: the maximum)
// of word col of the `groups` records of rec_words words
hipError_t launch_bc_combine(const unsigned long long *partials, uint32_t groups, uint32_t rec_words, uint32_t max_cols,
                             unsigned long long *result, hipStream_t s);
// -- bc6h.hip --
// KC_BC6H (16-byte blocks; R, G, B as half bit patterns, alpha never read).  bc6h_encode_kernel<nt>: launch_bc7_encode's arguments
// without the sRGB form.  bc6h_decode_kernel<nt, count>: launch_bc_decode's arguments, dst[0..2] written; count: result[0] = the
// blocks of the two-subset modes, which are not decoded (a second launch).  bc6h_compare_kernel<nt>, then bc_combine_kernel:
// launch_bc_compare's arguments and record, the differences taken over the half bit patterns.
hipError_t launch_bc6h_encode(const Operand op[4], int gray, char *dst, uint64_t row_pitch, uint32_t w, uint32_t h, uint32_t nt_mask,
                              hipStream_t s);
hipError_t launch_bc6h_decode(const BcDecodeArgs &a, bool count, uint32_t nt_mask, uint32_t groups, hipStream_t s);
hipError_t launch_bc6h_compare(const Operand op[4], int gray, const char *blocks, uint64_t row_pitch, uint32_t w, uint32_t h, uint32_t nt_mask,
                               uint32_t groups, unsigned long long *partials, unsigned long long *result, hipStream_t s);
// -- bc_modes.hip --
// KC_BC_ALL_MODES for KC_BC7 and KC_BC6H: every mode of the two formats, partition tables included (bc_modes.h has the decoders).
// bc7_modes_decode_kernel<nt> / bc6h_modes_decode_kernel<nt>: launch_bc_decode's arguments; nothing is undecoded, so there is no
// count and no second launch (a.partials and a.result are not used).  bc7_modes_compare_kernel<srgb, nt> /
// bc6h_modes_compare_kernel<nt>, then bc_combine_kernel: launch_bc_compare's arguments and record, word 8 always 0.
hipError_t launch_bc_modes_decode(int fmt, const BcDecodeArgs &a, uint32_t nt_mask, uint32_t groups, hipStream_t s);
hipError_t launch_bc_modes_compare(int fmt, int srgb, const Operand op[4], int gray, const char *blocks, uint64_t row_pitch, uint32_t w,
                                   uint32_t h, uint32_t nt_mask, uint32_t groups, unsigned long long *partials, unsigned long long *result,
                                   hipStream_t s);
// -- mip.hip --
// Mip chains (mip.hip / mip.cpp): the 2 x 2 box of the header on the n_planes distinct resident planes of one image.  The device
// steps of this family, of mip_normals.hip, of mip_roughness.hip, of mip_alpha.hip and of preview.hip's reduction are one copy, mip_steps.h, with
// the launch checks of the eight launch functions below.
// mip_pyramid_kernel<nt>: levels 1..n (1 <= n <= 6, both of w >> n and h >> n still >= 1) of the w x h source planes, one
// workgroup per 64 x 64 tile; dst[p][k - 1] is level k of plane p, dst_pitch[k - 1] floats between its rows.
struct MipPyramidArgs {
    const float *src[4];
    uint32_t src_pitch[4];  // floats
    float *dst[4][6];
    uint32_t dst_pitch[6];  // floats
    uint32_t w, h, n;
};
hipError_t launch_mip_pyramid(const MipPyramidArgs &a, uint32_t n_planes, bool nt, hipStream_t s);
// mip_level_kernel<nt>: the one level below a w x h source (not 1 x 1), max(1, w >> 1) x max(1, h >> 1), with the clamps; dst rows
// start 16-byte aligned
struct MipLevelArgs {
    const float *src[4];
    uint32_t src_pitch[4];  // floats
    float *dst[4];
    uint32_t dst_pitch;  // floats
    uint32_t w, h;
};
hipError_t launch_mip_level(const MipLevelArgs &a, uint32_t n_planes, bool nt, hipStream_t s);
// -- mip_normals.hip --
// Normal-map chains (KC_MIP_NORMALS): the same two walks (mip_steps.h) with R, G, B coupled in one thread -- the box of each
// channel, then the header's renormalisation of the three, at every level.  Channel c is a resident plane (src[c], src_pitch[c]), the constant
// cval[c] (bit c of const_mask; src[c] is not looked at) or the loads of an earlier channel that aliases it (bits 2c, 2c + 1 of
// `from` = that channel, c itself otherwise).  Every level has three resident planes of its own: dst[c][k - 1] is level k of
// channel c in normal_pyramid_kernel<nt> (n, the tiles and the pitches as in MipPyramidArgs), dst[c] the one level of
// normal_level_kernel<nt> (as MipLevelArgs).
struct NormalPyramidArgs {
    const float *src[3];
    uint32_t src_pitch[3];  // floats
    float cval[3];
    uint32_t const_mask, from;
    float *dst[3][6];
    uint32_t dst_pitch[6];  // floats
    uint32_t w, h, n;
};
hipError_t launch_normal_pyramid(const NormalPyramidArgs &a, bool nt, hipStream_t s);
struct NormalLevelArgs {
    const float *src[3];
    uint32_t src_pitch[3];  // floats
    float cval[3];
    uint32_t const_mask, from;
    float *dst[3];
    uint32_t dst_pitch;  // floats
    uint32_t w, h;
};
hipError_t launch_normal_level(const NormalLevelArgs &a, bool nt, hipStream_t s);
// -- mip_roughness.hip --
// Roughness chains (kc_image_build_roughness_mips): the same two walks with four channels coupled in one thread -- the vector of
// the normals (0..2) and the roughness (3), each down the plain rule -- and the header's rough() of the four boxes as the one
// plane a level stores.  `first`: the sources are level 0, X, Y, Z of the normal map as stored (decoded to unit vectors texel by
// texel right after the loads) and the roughness plane; channel c is then a resident plane (src[c], src_pitch[c]; channels that
// alias carry the same pointer) or the constant cval[c] (bit c of const_mask; src[c] is not looked at).  Otherwise the sources
// are the four state planes of the level read, m_x, m_y, m_z, r, and const_mask is 0.  dst[k - 1] is the stored plane of level
// k in roughness_pyramid_kernel<nt, first> (n, the tiles and the pitches as in MipPyramidArgs), dst the one level of
// roughness_level_kernel<nt, first> (as MipLevelArgs).  state: where more levels follow, the four plain boxes of the last level
// written (level n; the one level) go to these planes, rows as far apart as that level's dst rows; all NULL when none follows.
struct RoughnessPyramidArgs {
    const float *src[4];
    uint32_t src_pitch[4];  // floats
    float cval[4];
    uint32_t const_mask;
    float power;
    float *dst[6];
    uint32_t dst_pitch[6];  // floats
    float *state[4];
    uint32_t w, h, n;
};
hipError_t launch_roughness_pyramid(const RoughnessPyramidArgs &a, bool first, bool nt, hipStream_t s);
struct RoughnessLevelArgs {
    const float *src[4];
    uint32_t src_pitch[4];  // floats
    float cval[4];
    uint32_t const_mask;
    float power;
    float *dst;
    uint32_t dst_pitch;  // floats
    float *state[4];
    uint32_t w, h;
};
hipError_t launch_roughness_level(const RoughnessLevelArgs &a, bool first, bool nt, hipStream_t s);
// -- mip_alpha.hip --
// Alpha-weighted chains (KC_MIP_ALPHA_WEIGHT): the same two walks with four channels coupled in one thread -- the premultiplied
// colour p_r, p_g, p_b (0..2) and the weight w (3), each down the plain rule -- then one push launch over all levels.  `first`:
// the sources are level 0, R, G, B and alpha as stored, each a resident plane (src[c], src_pitch[c]; channels that alias carry
// the same pointer) or the constant cval[c] (bit c of const_mask; src[c] is not looked at); the weight and the premultiplication
// are applied right after the loads, and the thread stores its level-0 colour texels (c where w0 > 0, else 0) to dst0[c], rows
// dst0_pitch floats apart.  Otherwise the sources are the three state planes P_r, P_g, P_b and the weight plane of the level
// read, and const_mask is 0.  Every level k the launch finishes stores W > 0 ? P_c / W : 0 to dst[c][k - 1] and W to
// wdst[k - 1] (alpha_pull_pyramid_kernel<nt, first>: n, the tiles and the pitches as in MipPyramidArgs; alpha_pull_level_kernel
// <nt, first>: the one level, as MipLevelArgs).  state: where more levels follow, P_c of the last level written go to these three
// planes, rows as far apart as that level's dst rows (its W is wdst's plane); all NULL when none follows.  A first one-level
// launch on a 1 x 1 image has no level to write (dst, wdst NULL): it stores level 0's colour alone.
struct AlphaPullPyramidArgs {
    const float *src[4];
    uint32_t src_pitch[4];  // floats
    float cval[4];
    uint32_t const_mask;
    float *dst0[3];
    uint32_t dst0_pitch;  // floats
    float *dst[3][6];
    float *wdst[6];
    uint32_t dst_pitch[6];  // floats
    float *state[3];
    uint32_t w, h, n;
};
hipError_t launch_alpha_pull_pyramid(const AlphaPullPyramidArgs &a, bool first, bool nt, hipStream_t s);
struct AlphaPullLevelArgs {
    const float *src[4];
    uint32_t src_pitch[4];  // floats
    float cval[4];
    uint32_t const_mask;
    float *dst0[3];
    uint32_t dst0_pitch;  // floats
    float *dst[3];
    float *wdst;
    uint32_t dst_pitch;  // floats
    float *state[3];
    uint32_t w, h;
};
hipError_t launch_alpha_pull_level(const AlphaPullLevelArgs &a, bool first, bool nt, hipStream_t s);
// alpha_push_kernel: one thread per quad of every level, level 0 included, through a job table in the launch's arguments (one
// AlphaPushJob per level, as CoverageJob: nothing is uploaded).  known: level 0's alpha (a > 0), or W_k (> 0) of a level below
// it; wsrc NULL: every texel of the level is known (a constant alpha of positive weight).  A thread stores, for each unknown
// texel of its quad, the three colours of the nearest ancestor whose weight is positive; known texels and the weights are
// never written, so the launch has no race.  Workgroups first_wg .. first_wg + wgs - 1 work on the level.
constexpr uint32_t KC_ALPHA_MAX_LEVELS = 32;  // a chain has at most 32 levels
struct AlphaPushJob {
    float *dst[3];      // the level's colour planes
    const float *wsrc;  // level 0: the image's alpha; below: the level's weight plane
    uint32_t dst_pitch, w_pitch;  // floats
    uint32_t w, h;
    uint32_t first_wg, wgs;
};
struct AlphaPushArgs {
    AlphaPushJob jobs[KC_ALPHA_MAX_LEVELS + 3];  // three spare entries: level j's kernel code names entries j + 1 .. j + 3
    uint32_t levels;
};
inline uint32_t alpha_push_job_wgs(uint32_t w, uint32_t h) { return (uint32_t)(((uint64_t)((w + 3) / 4) * h + 255) / 256); }
hipError_t launch_alpha_push(const AlphaPushArgs &a, uint32_t wgs, hipStream_t s);
// -- mip_coverage.hip --
// Alpha-test coverage (KC_MIP_COVERAGE): an exact k-th-largest selection over the alpha plane of every level of a chain -- a
// radix select on the 30 significant bits of the header's key, 10 bits (KC_COVERAGE_BINS bins) per pass -- and the scale of
// every level.  Everything the selection computes is an integer count, so no result depends on the launch shape or the order
// of the atomics.  One table of CoverageJob, one per level; it is small (a chain has at most 32 levels) and travels in the
// launches' arguments, so that nothing is uploaded and kc_image_build_mips never waits for a staging buffer.  Workgroup first_wg ..
// first_wg + wgs - 1 of a count or scale launch works on that level (level 0 takes part in the first count launch only).
constexpr uint32_t KC_COVERAGE_BINS = 1024, KC_COVERAGE_MAX_LEVELS = 32;
struct CoverageJob {
    const float *src;  // the plain rule's alpha of the level, p_k
    float *dst;        // the stored alpha, d_k (levels >= 1 of a chain; nullptr for the query, which does not scale)
    uint32_t src_pitch, dst_pitch;  // floats
    uint32_t w, h;
    uint32_t first_wg, wgs;
};
// Per level in device memory, zeroed before the first launch: the public kc_mip_coverage_level, then the state of the select --
// the key bits found so far, the rank that remains among the texels with that prefix, done != 0 once the scale is known.
struct CoverageRecord {
    unsigned long long texels, target, plain_covered;
    float v, scale;
    uint32_t prefix, rank, done, unused;
};
struct CoverageArgs {
    CoverageJob jobs[KC_COVERAGE_MAX_LEVELS];
    CoverageRecord *rec;
    uint32_t *hist;  // levels x KC_COVERAGE_BINS, zeroed before the first launch; a pick leaves its level's bins zero again
    uint32_t levels;
    uint32_t ref;    // B
    float r_b;       // (float)B / 255.0f
};
// workgroups of a level's job: few, every thread of 256 sixteen quads where the level has them and 1024 workgroups at the most --
// every workgroup of a level ends with atomics on that level's one histogram, and their depth per address is what a count costs
inline uint32_t coverage_job_wgs(uint32_t w, uint32_t h)
{
    const uint64_t quads = (uint64_t)((w + 3) / 4) * h;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((quads + 4095) / 4096, 1), 1024);
}
// coverage_count_kernel, pass 0 .. 2: the histogram of the pass's 10 key bits over the texels whose higher bits equal the
// level's prefix, for every level >= 1 that is not done; pass 0 also counts the covered texels of every level, level 0
// included.  coverage_pick_kernel, one workgroup per level, after each count: pass 0 sets the targets and finishes the levels
// that keep the plain alpha, every pass finds the bin that holds the rank, pass 2 ends with v and the scale.
// coverage_scale_kernel: d_k = p_k * s_k for every level >= 1, a copy where s_k == 1.
hipError_t launch_coverage_count(const CoverageArgs &a, uint32_t pass, uint32_t first_wg, uint32_t wgs, hipStream_t s);
hipError_t launch_coverage_pick(const CoverageArgs &a, uint32_t pass, hipStream_t s);
hipError_t launch_coverage_scale(const CoverageArgs &a, uint32_t first_wg, uint32_t wgs, hipStream_t s);
// -- preview.hip --
// Previews (preview.hip / preview.cpp): preview_kernel<srgb, nt> on `workgroups` workgroups, one pass of a batch (the tile
// reduction is mip_steps.h's).  jobs: `count`
// PreviewJob (preview_walk.h) in device memory; prefix: count + 1 words, prefix[j] = the first workgroup of job j, prefix[count] =
// workgroups.  srgb: R, G, B (Gray: the value) of the jobs that store RGBA8 go through quant_u8_srgb.
hipError_t launch_preview(const PreviewJob *jobs, const uint32_t *prefix, uint32_t count, uint32_t workgroups, bool srgb, bool nt, hipStream_t s);
// -- sdf.hip --
// Signed distance fields (sdf.hip / sdf.cpp): the header's rule as a separable exact transform with windows of radius `spread`.
// mid: one 16-bit word per texel, rows w words apart -- bits 0-7 the distance along the column to the nearest texel of the
// other class, capped at spread + 1 (1..255: a texel is its own class), bit 8 the class (1: inside).
// sdf_columns_kernel<nt, wrap>: src -> mid, one thread per column of a band of KC_SDF_BAND rows, one workgroup per KC_SDF_SEG
// columns of a band.  sdf_rows_kernel<nt, wrap>: mid -> dst, one workgroup per KC_SDF_SEG columns of KC_SDF_ROWS rows.  Both
// grids are one-dimensional.  nt: the source loads of the first, the result stores of the second.
constexpr uint32_t KC_SDF_BAND = 64, KC_SDF_SEG = 256, KC_SDF_ROWS = 4;
struct SdfArgs {
    const float *src;
    uint32_t src_pitch;  // floats
    uint16_t *mid;
    float *dst;
    uint32_t dst_pitch;  // floats
    uint32_t w, h, ref, spread;  // ref: B, 1..255; spread: S, 1..KC_SDF_MAX_SPREAD
};
inline uint64_t sdf_columns_groups(uint32_t w, uint32_t h) { return (uint64_t)((w + KC_SDF_SEG - 1) / KC_SDF_SEG) * ((h + KC_SDF_BAND - 1) / KC_SDF_BAND); }
inline uint64_t sdf_rows_groups(uint32_t w, uint32_t h) { return (uint64_t)((w + KC_SDF_SEG - 1) / KC_SDF_SEG) * ((h + KC_SDF_ROWS - 1) / KC_SDF_ROWS); }
hipError_t launch_sdf_columns(const SdfArgs &a, bool wrap, bool nt, hipStream_t s);
hipError_t launch_sdf_rows(const SdfArgs &a, bool wrap, bool nt, hipStream_t s);
// -- blur.hip --
// Separable Gaussian blur (blur.hip / blur.cpp): the header's texel rule along one axis of `planes` planes per launch; the plane
// index is blockIdx.y, the pointers, pitches (floats, multiples of 4; rows start 16-byte aligned) and the R + 1 weights travel
// in the argument block.  blur_rows_kernel<nt, wrap>: one workgroup per KC_BLUR_SEG columns of KC_BLUR_ROWS rows, a wave per
// row, a lane per four adjacent texels.  blur_columns_kernel<nt, wrap>: one workgroup per KC_BLUR_COLS columns of a band of
// KC_BLUR_BAND rows, a lane per four adjacent columns of four adjacent rows; its LDS is (KC_BLUR_BAND + 2 R) rows of
// KC_BLUR_COLS floats, sized by the launch.  nt: the source loads of the rows kernel, the result stores of the columns kernel.
constexpr uint32_t KC_BLUR_SEG = 256, KC_BLUR_ROWS = 4, KC_BLUR_COLS = 64, KC_BLUR_BAND = 64;
struct BlurArgs {
    const float *src[4];
    float *dst[4];
    uint32_t src_pitch[4], dst_pitch[4];  // floats
    uint32_t w, h, radius, planes;        // radius: R, 1..KC_BLUR_MAX_RADIUS; planes: 1..4
    float weights[KC_BLUR_MAX_RADIUS + 1];
};
inline uint64_t blur_rows_groups(uint32_t w, uint32_t h) { return (uint64_t)((w + KC_BLUR_SEG - 1) / KC_BLUR_SEG) * ((h + KC_BLUR_ROWS - 1) / KC_BLUR_ROWS); }
inline uint64_t blur_columns_groups(uint32_t w, uint32_t h) { return (uint64_t)((w + KC_BLUR_COLS - 1) / KC_BLUR_COLS) * ((h + KC_BLUR_BAND - 1) / KC_BLUR_BAND); }
inline size_t blur_columns_lds(uint32_t radius) { return (size_t)(KC_BLUR_BAND + 2u * radius) * KC_BLUR_COLS * sizeof(float); }
hipError_t launch_blur_rows(const BlurArgs &a, bool wrap, bool nt, hipStream_t s);
hipError_t launch_blur_columns(const BlurArgs &a, bool wrap, bool nt, hipStream_t s);

}  // namespace kc
