// The one copy of the mip steps that mip.hip, mip_normals.hip, mip_roughness.hip, mip_alpha.hip and preview.hip share: the box, the reduction of
// a 64 x 64 tile by a 16 x 16 workgroup, the tile's loads and stores, the one-level step, where a channel of a normal map comes
// from, and the two launch checks.  C channels (1, 3, or the 4 of a roughness chain -- the normals' vector and the roughness -- and of
// an alpha-weighted one -- the premultiplied colour and the weight) go
// down together; a unit supplies its rule, rule(float (&b)[C]), called with the C boxes of one texel before they are stored or
// passed on (nothing for the plain chain, the previews and the roughness chain's state, normal_texel for normal maps), and says
// what happens to a finished level: the tile walk's `done`, the one-level walk's `sink` -- a roughness chain stores one plane
// that is none of the four it passes on.  The fused form equals the level-by-level one, a preview equals to_u8 of the chain and a
// normal map's alpha equals the plain rule because all of them run these additions in this order;
// tests/host/preview_walk_check.cpp keeps a copy of its own (lanes_reduce): the host's check stays independent of this header.
// Included inside namespace kc after streaming.h; every definition is static, each unit keeps its own copy.
#pragma once

typedef float mip_f4 __attribute__((ext_vector_type(4)));
typedef float mip_f2 __attribute__((ext_vector_type(2)));
struct MipRows {  // a thread's 4 x 4 texels of one channel of the tile
    mip_f4 r[4];
};

static __device__ __forceinline__ float mip_box(float a, float b, float c, float d) { return ((a + b) + (c + d)) * 0.25f; }

static __device__ __forceinline__ mip_f4 mip_splat(float v) { return mip_f4{ v, v, v, v }; }

// What the one-level walk stores: a whole quad under the launch's cache policy, a texel of a row's tail plainly.
template <bool NT>
static __device__ __forceinline__ void mip_level_store(float *p, mip_f4 v) { st_policy<NT>(reinterpret_cast<mip_f4 *>(p), v); }
template <bool NT>
static __device__ __forceinline__ void mip_level_store(float *p, float v) { *p = v; }

// The plain rule: the boxes are the texel.
struct MipPlainRule {
    template <int C>
    __device__ __forceinline__ void operator()(float (&)[C]) const {}
};

// ---------------------------------------------------------------- where the channels of a launch come from
// Every channel its own plane: load(c, v[c]).
struct MipOwnPlanes {
    template <class T, int C, class Const, class Load>
    __device__ __forceinline__ void operator()(T (&v)[C], Const, Load load) const
    {
#pragma unroll
        for (int c = 0; c < C; ++c) load(c, v[c]);
    }
};

static constexpr uint32_t kNormalOwnPlanes = 0u | 1u << 2 | 2u << 4;  // `from` when every channel reads its own plane

// R, G, B of a normal-map launch (a: NormalPyramidArgs or NormalLevelArgs): channel c is the constant a.cval[c]
// (of_const(a.cval[c], v[c]); its pointer is never formed), what an earlier channel that aliases it has loaded, or its own plane
// (load(c, v[c])).  All three are uniform over the launch.
template <class Args, class T, class Const, class Load>
static __device__ __forceinline__ void normal_channels(const Args &a, T (&v)[3], Const of_const, Load load)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t from = (a.from >> (2 * c)) & 3u;
        if ((a.const_mask >> c) & 1u) of_const(a.cval[c], v[c]);
        else if (c >= 1 && from == 0u) v[c] = v[0];
        else if (c == 2 && from == 1u) v[c] = v[1];
        else load(c, v[c]);
    }
}

// ---------------------------------------------------------------- the tile: thread (tx, ty) of 16 x 16 = threadIdx.x & 15, >> 4
// Thread (tx, ty) holds rows 4 ty .. 4 ty + 3, columns 4 tx .. 4 tx + 3 of the tile (blockIdx.x, blockIdx.y) of a w x h plane: four
// 16-byte loads.  Rows are readable in whole float4 quads up to 4 ceil(w / 4) floats and no further (kc_plane_wrap), so the quad
// index is clamped to the last whole quad and the rows to h - 1: what the out-of-image lanes hold never reaches a stored texel.
template <bool NT>
static __device__ __forceinline__ void mip_tile_load(const float *src, uint32_t sp, uint32_t w, uint32_t h, uint32_t tx, uint32_t ty, MipRows &p)
{
    const uint32_t q = min(blockIdx.x * 16u + tx, (w + 3u) / 4u - 1u);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t r = min(blockIdx.y * 64u + 4u * ty + (uint32_t)i, h - 1u);
        p.r[i] = ld_policy<NT>(reinterpret_cast<const mip_f4 *>(src + (size_t)r * sp + 4u * q));
    }
}

// Levels 1 to 4 of the tile.  Levels 1 and 2 are in-lane (a 2 x 2 patch, then one value); a wave holds four ty rows, so levels 3
// and 4 are exchanges between its lanes (tx ^ 1, ty ^ 1, then tx ^ 2, ty ^ 2: lanes ^ 1, ^ 16, ^ 2, ^ 32).  f32 addition commutes
// bit for bit, so the lanes of an exchange group hold bit-equal sums, apply the rule to their own copy and stay bit-equal.  Every
// lane takes part, in range or not: the exchanges need all 64 lanes of a wave.  done(k, v) takes level k as the thread holds it
// (level 1: v[c][0..3], the patch row-major; levels 2 to 4: v[c][0], one texel per 2^(k-2) x 2^(k-2) threads, the same in all of
// them) and returns true when nothing below level k is wanted.  After level 4 the 4 x 4 level-4 values go to l4[c] for
// mip_tile_tail, which runs behind a barrier that the calling kernel places.
template <int C, class Rule, class Done>
static __device__ __forceinline__ void mip_tile_reduce(const MipRows (&p)[C], uint32_t tx, uint32_t ty, float (*l4)[16], Rule rule, Done done)
{
    float v1[C][4], v[C][4], b[C];  // level 1, then the levels below it in v[c][0]
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int c = 0; c < C; ++c)
                b[c] = mip_box(p[c].r[2 * r][2 * j], p[c].r[2 * r][2 * j + 1], p[c].r[2 * r + 1][2 * j], p[c].r[2 * r + 1][2 * j + 1]);
            rule(b);
#pragma unroll
            for (int c = 0; c < C; ++c) v1[c][2 * r + j] = b[c];
        }
    if (done(1u, v1)) return;
#pragma unroll
    for (int c = 0; c < C; ++c) b[c] = mip_box(v1[c][0], v1[c][1], v1[c][2], v1[c][3]);
    rule(b);
#pragma unroll
    for (int c = 0; c < C; ++c) v[c][0] = b[c];
    if (done(2u, v)) return;
#pragma unroll
    for (uint32_t k = 3u; k <= 4u; ++k) {
        const int m = 1 << (k - 3u);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float hs = v[c][0] + __shfl_xor(v[c][0], m, 64);
            b[c] = (hs + __shfl_xor(hs, 16 * m, 64)) * 0.25f;
        }
        rule(b);
#pragma unroll
        for (int c = 0; c < C; ++c) v[c][0] = b[c];
        if (done(k, v)) return;
    }
    if (!(tx & 3u) && !(ty & 3u)) {
#pragma unroll
        for (int c = 0; c < C; ++c) l4[c][(ty >> 2) * 4u + (tx >> 2)] = v[c][0];
    }
}

// Levels 5 and 6 from l4, behind the barrier.  five: threads 0 .. 3 make the tile's 2 x 2 level 5, thread t texel (t & 1, t >> 1);
// six: thread 0 makes the one texel of level 6.  Each goes to done(k, v) in v[c][0].
template <int C, class Rule, class Done>
static __device__ __forceinline__ void mip_tile_tail(const float (*l4)[16], bool five, bool six, uint32_t t, Rule rule, Done done)
{
    auto level5 = [&](uint32_t cx, uint32_t cy, float (&o)[C]) __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float *s = l4[c] + 8u * cy + 2u * cx;
            o[c] = mip_box(s[0], s[1], s[4], s[5]);
        }
        rule(o);
    };
    float v[C][4], b[C];
    if (five && t < 4u) {
        level5(t & 1u, t >> 1, b);
#pragma unroll
        for (int c = 0; c < C; ++c) v[c][0] = b[c];
        done(5u, v);
    }
    if (six && t == 0u) {
        float v5[4][C];
#pragma unroll
        for (int k = 0; k < 4; ++k) level5((uint32_t)(k & 1), (uint32_t)(k >> 1), v5[k]);
#pragma unroll
        for (int c = 0; c < C; ++c) b[c] = mip_box(v5[0][c], v5[1][c], v5[2][c], v5[3][c]);
        rule(b);
#pragma unroll
        for (int c = 0; c < C; ++c) v[c][0] = b[c];
        done(6u, v);
    }
}

// What the chain kernels do with a finished level (the body of their `done`): level k <= n of channel c goes to dst(c, k), rows
// pitch[k - 1] floats apart, where the thread's texel lies inside the level, (w >> k) x (h >> k).  NT: the level-1 stores are
// nontemporal.
template <bool NT, int C, class Dst>
static __device__ __forceinline__ void mip_tile_store(uint32_t k, const float (&v)[C][4], uint32_t n, uint32_t w, uint32_t h, uint32_t tx, uint32_t ty,
                                                      Dst dst, const uint32_t *pitch)
{
    if (k == 1u) {
        const uint32_t W = w >> 1, H = h >> 1, x = blockIdx.x * 32u + 2u * tx;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float *d = dst(c, 1u);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const uint32_t y = blockIdx.y * 32u + 2u * ty + (uint32_t)r;
                float *o = d + (size_t)y * pitch[0] + x;
                if (y < H && x + 1u < W) st_policy<NT>(reinterpret_cast<mip_f2 *>(o), mip_f2{ v[c][2 * r], v[c][2 * r + 1] });
                else if (y < H && x < W) *o = v[c][2 * r];
            }
        }
        return;
    }
    // levels 2 to 4: one thread of 2^(k-2) x 2^(k-2) stores; levels 5 and 6: mip_tile_tail's threads, (tx, 0) with tx < 4
    const uint32_t low = k <= 4u ? (1u << (k - 2u)) - 1u : 0u;
    const uint32_t lx = k <= 4u ? tx >> (k - 2u) : tx & 1u, ly = k <= 4u ? ty >> (k - 2u) : tx >> 1;
    if (n >= k && !(tx & low) && !(ty & low)) {
        const uint32_t x = blockIdx.x * (64u >> k) + lx, y = blockIdx.y * (64u >> k) + ly;
        if (x < (w >> k) && y < (h >> k)) {
#pragma unroll
            for (int c = 0; c < C; ++c) dst(c, k)[(size_t)y * pitch[k - 1u] + x] = v[c][0];
        }
    }
}

// ---------------------------------------------------------------- one level of any size, with the clamps
// The four source texels under one output texel (T = float: the scalar tail) or the 2 x 8 under a quad of them (T = mip_f4: t0,
// t1 the upper row's columns 0 .. 3 and 4 .. 7, b0, b1 the lower row's), of one channel, as loaded.
template <class T>
struct MipSrc {
    T t0, t1, b0, b1;
};
static __device__ __forceinline__ MipSrc<float> mip_src_const(float cv, const float &) { return MipSrc<float>{ cv, cv, cv, cv }; }
static __device__ __forceinline__ MipSrc<mip_f4> mip_src_const(float cv, const mip_f4 &)
{
    return MipSrc<mip_f4>{ mip_splat(cv), mip_splat(cv), mip_splat(cv), mip_splat(cv) };
}
static __device__ __forceinline__ float mip_src_box(const MipSrc<float> &s) { return mip_box(s.t0, s.t1, s.b0, s.b1); }
static __device__ __forceinline__ mip_f4 mip_src_box(const MipSrc<mip_f4> &s)
{
    return mip_f4{ mip_box(s.t0[0], s.t0[1], s.b0[0], s.b0[1]), mip_box(s.t0[2], s.t0[3], s.b0[2], s.b0[3]),
                   mip_box(s.t1[0], s.t1[1], s.b1[0], s.b1[1]), mip_box(s.t1[2], s.t1[3], s.b1[2], s.b1[3]) };
}
// Nothing happens to the source texels before the box (every unit but the first launches of mip_roughness.hip and mip_alpha.hip).
struct MipNoDecode {
    static constexpr bool kNone = true;
};

// The C boxes of one output position (T = mip_f4: a quad of texels; float: one): fetch(c, s) loads the source texels of channel
// c, channels(v, of_const, load) says where the channels come from (MipOwnPlanes, normal_channels).  Without a decode every
// channel is boxed as it arrives.  A decode (kNone == false; decode(s) on MipSrc<T> (&s)[C]) couples the channels before the
// box, so the source texels of all C are held first.
template <int C, class T, class Channels, class Decode, class Fetch>
static __device__ __forceinline__ void mip_level_boxes(T (&b)[C], Channels channels, Decode decode, Fetch fetch)
{
    if constexpr (Decode::kNone) {
        channels(
            b, [](float cv, T &o) __attribute__((always_inline)) { o = mip_src_box(mip_src_const(cv, o)); },
            [&](int c, T &o) __attribute__((always_inline)) {
                MipSrc<T> s;
                fetch(c, s);
                o = mip_src_box(s);
            });
    } else {
        MipSrc<T> s[C];
        channels(s, [](float cv, MipSrc<T> &o) __attribute__((always_inline)) { o = mip_src_const(cv, o.t0); }, fetch);
        decode(s);
#pragma unroll
        for (int c = 0; c < C; ++c) b[c] = mip_src_box(s[c]);
    }
}

// One thread per quad of output texels, rows in order.  A whole quad (4 q + 3 < W, hence source columns up to 8 q + 7 <= w - 1)
// is two 16-byte loads per source row and channel and one 16-byte value per channel; the tail of a row is scalar, with the
// column clamp.  channels and decode: mip_level_boxes; rule(v) is applied to the C boxes of every texel, and sink(o, v) takes
// them: a quad (v: mip_f4[C]) or one texel (v: float[C]) that starts o floats into a plane whose rows are dst_pitch floats apart.
template <bool NT, int C, class Channels, class Decode, class Rule, class Sink>
static __device__ __forceinline__ void mip_level_walk(const float *const *src, const uint32_t *src_pitch, uint32_t w, uint32_t h, uint32_t dst_pitch,
                                                      Channels channels, Decode decode, Rule rule, Sink sink)
{
    const uint32_t W = max(w >> 1, 1u), H = max(h >> 1, 1u), quads = (W + 3u) / 4u;
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= quads * H) return;
    const uint32_t y = idx / quads, q = idx - y * quads;
    const uint32_t y0 = 2u * y, y1 = min(2u * y + 1u, h - 1u);
    const size_t o = (size_t)y * dst_pitch + 4u * q;
    if (4u * q + 3u < W) {
        mip_f4 b[C];
        mip_level_boxes(b, channels, decode, [&](int c, MipSrc<mip_f4> &s) __attribute__((always_inline)) {
            const float *r0 = src[c] + (size_t)y0 * src_pitch[c], *r1 = src[c] + (size_t)y1 * src_pitch[c];
            s.t0 = ld_policy<NT>(reinterpret_cast<const mip_f4 *>(r0 + 8u * q));
            s.t1 = ld_policy<NT>(reinterpret_cast<const mip_f4 *>(r0 + 8u * q + 4u));
            s.b0 = ld_policy<NT>(reinterpret_cast<const mip_f4 *>(r1 + 8u * q));
            s.b1 = ld_policy<NT>(reinterpret_cast<const mip_f4 *>(r1 + 8u * q + 4u));
        });
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v[C];
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = b[c][j];
            rule(v);
#pragma unroll
            for (int c = 0; c < C; ++c) b[c][j] = v[c];
        }
        sink(o, b);
        return;
    }
    for (uint32_t x = 4u * q; x < W; ++x) {
        const uint32_t x0 = 2u * x, x1 = min(2u * x + 1u, w - 1u);
        float v[C];
        mip_level_boxes(v, channels, decode, [&](int c, MipSrc<float> &s) __attribute__((always_inline)) {
            const float *r0 = src[c] + (size_t)y0 * src_pitch[c], *r1 = src[c] + (size_t)y1 * src_pitch[c];
            s = MipSrc<float>{ r0[x0], r0[x1], r1[x0], r1[x1] };
        });
        rule(v);
        sink(o + (x - 4u * q), v);
    }
}

// The walk for the units that store what the rule leaves: channel c of the level goes to dst[c].
template <bool NT, int C, class Rule, class Channels>
static __device__ __forceinline__ void mip_level_step(const float *const *src, const uint32_t *src_pitch, uint32_t w, uint32_t h, float *const *dst,
                                                      uint32_t dst_pitch, Rule rule, Channels channels)
{
    mip_level_walk<NT, C>(src, src_pitch, w, h, dst_pitch, channels, MipNoDecode(), rule, [&](size_t o, const auto (&v)[C]) __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < C; ++c) mip_level_store<NT>(dst[c] + o, v[c]);
    });
}

// ---------------------------------------------------------------- the launch checks (host)
// A pyramid launch of n levels on `planes` planes of w x h: 1 <= n <= 6, both extents halve n times, one workgroup per tile
[[maybe_unused]] static bool mip_pyramid_grid(uint32_t w, uint32_t h, uint32_t n, uint32_t planes, dim3 *grid)
{
    if (w < 2 || h < 2 || n < 1 || n > 6 || planes < 1 || planes > 4) return false;
    if ((w >> n) == 0 || (h >> n) == 0) return false;
    const uint64_t gx = ((uint64_t)w + 63) / 64, gy = ((uint64_t)h + 63) / 64;
    if (gx > 0x7fffffffull || gy > 65535ull) return false;
    *grid = dim3((unsigned)gx, (unsigned)gy, planes);
    return true;
}

// A one-level launch below `planes` planes of w x h (not 1 x 1): one thread per quad of the level
[[maybe_unused]] static bool mip_level_grid(uint32_t w, uint32_t h, uint32_t planes, dim3 *grid)
{
    if (w == 0 || h == 0 || (w == 1 && h == 1) || planes < 1 || planes > 4) return false;
    const uint64_t W = w > 1 ? w >> 1 : 1, H = h > 1 ? h >> 1 : 1;
    const uint64_t total = (W + 3) / 4 * H;
    if (total > (1ull << 31)) return false;  // the kernel's quad index is 32-bit
    *grid = dim3((unsigned)((total + 255) / 256), planes);
    return true;
}
