// How many float4 per lane should a compiled chain kernel (csrc/specialize.cpp, generate) keep in flight when one of its
// inputs is served by the Infinity Cache?  Not part of the product.
//
// The traffic is config #1's and the headline's (profiles/tilecopy.hip, add2): 201 MB + 201 MB read, 201 MB written, as three
// 3-plane buffers; input A nontemporal, input B plain, the result nontemporal and alternating between two buffers (cache
// policy mask 0x101).  The body is R dependent records "c - (acc op b)", op alternating + and *, packed exactly as the
// generator packs them (the text of kPackedF4; the constants arrive in scalar registers from the argument block).
//   U      float4 per lane; quad u of a lane is at base + u * 256, so a workgroup touches one contiguous run per plane
//   form   straight: all 2 U loads, then U bodies, each followed by its store
//          rolled:   all 2 U loads, then ONE body in a loop that is not unrolled and rotates the next quad's registers in
//          late:     all 2 U loads, then U bodies, then U stores (the compiler waits for EVERYTHING outstanding, a store
//                    included, before the second body of the straight form: vmcnt(0); here no store lies between the bodies)
//   warm   the same A and B every launch (B resident);   cold   three sets of A and B in rotation (1.2 GB of inputs)
// Every row: 20 launches to warm up, then 100 back to back between two events.  Before the timing every form is run once on
// a unit count that is no multiple of anything and compared byte for byte with U = 1.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math profiles/chain_inflight.hip -o /tmp/chain_inflight
//   for i in 1 2 3 4; do /tmp/chain_inflight; done
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CK(x)                                                                      \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                    \
            std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

typedef float raw4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef unsigned long long rec64;
static __device__ __forceinline__ f2 pk_sub(f2 a, f2 b)
{
    f2 d;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
struct kconst {
    rec64 rec;  // { word, c }
    __device__ __forceinline__ f2 minus(f2 b) const
    {
        f2 d;
        asm("v_pk_add_f32 %0, %1, %2 op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "s"(rec >> 32), "v"(b));
        return d;
    }
};
struct f4 {
    f2 lo, hi;
    f4() = default;
    __device__ __forceinline__ f4(f2 l, f2 h) : lo(l), hi(h) {}
    __device__ __forceinline__ f4(raw4 v) : lo(v.xy), hi(v.zw) {}
    __device__ __forceinline__ raw4 raw() const { return raw4{ lo.x, lo.y, hi.x, hi.y }; }
};
static __device__ __forceinline__ f4 operator+(f4 a, f4 b) { return f4(a.lo + b.lo, a.hi + b.hi); }
static __device__ __forceinline__ f4 operator*(f4 a, f4 b) { return f4(a.lo * b.lo, a.hi * b.hi); }
static __device__ __forceinline__ f4 operator-(kconst c, f4 b) { return f4(c.minus(b.lo), c.minus(b.hi)); }

struct Recs {
    rec64 rec[16];
};

template <int R>
static __device__ __forceinline__ f4 body(f4 acc, f4 y, const Recs &P)
{
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const kconst c{ P.rec[i] };
        acc = (i & 1) ? c - (acc * y) : c - (acc + y);
    }
    return acc;
}

enum { STRAIGHT = 0, ROLLED = 1, LATE = 2 };

// loads are clamped to the last unit (always in bounds), stores are guarded: the unit count need not be a multiple of U * 256
template <int U, int R, int FORM>
__global__ __launch_bounds__(256) void chain(const raw4 *__restrict__ a, const raw4 *__restrict__ b, raw4 *__restrict__ o, unsigned int n,
                                             const Recs P)
{
    unsigned int idx = blockIdx.x * (U * 256u) + threadIdx.x;
    f4 x[U], y[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned int i = min(idx + u * 256u, n - 1u);
        x[u] = __builtin_nontemporal_load(&a[i]);
        y[u] = b[i];
    }
    if (FORM == STRAIGHT) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const f4 acc = body<R>(x[u], y[u], P);
            if (idx + u * 256u < n) __builtin_nontemporal_store(acc.raw(), &o[idx + u * 256u]);
        }
    } else if (FORM == LATE) {
        f4 acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = body<R>(x[u], y[u], P);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (idx + u * 256u < n) __builtin_nontemporal_store(acc[u].raw(), &o[idx + u * 256u]);
    } else {
#pragma nounroll
        for (int u = 0; u < U; ++u) {
            const f4 acc = body<R>(x[0], y[0], P);
            if (idx < n) __builtin_nontemporal_store(acc.raw(), &o[idx]);
            idx += 256u;
#pragma unroll
            for (int k = 0; k + 1 < U; ++k) {
                x[k] = x[k + 1];
                y[k] = y[k + 1];
            }
        }
    }
}

struct Set {
    raw4 *a, *b;
};

int main()
{
    const size_t plane = (size_t)4096 * 4096 * 4, big = 3 * plane;
    const unsigned int n = (unsigned int)(big / 16);
    Set in[3];
    raw4 *out[2];
    for (auto &s : in) {
        CK(hipMalloc((void **)&s.a, big));
        CK(hipMalloc((void **)&s.b, big));
        CK(hipMemset(s.a, 0x3c, big));
        CK(hipMemset(s.b, 0x3c, big));
    }
    for (auto &p : out) CK(hipMalloc((void **)&p, big));
    Recs P;
    for (int i = 0; i < 16; ++i) {
        const float c = 1.0f - 0.03125f * i;
        unsigned int bits;
        std::memcpy(&bits, &c, 4);
        P.rec[i] = ((rec64)bits << 32) | (unsigned int)((i & 1 ? 13 : 10) | (2u << 8));
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));

    struct Row {
        const char *name;
        int U, R;
        void (*kernel)(const raw4 *, const raw4 *, raw4 *, unsigned int, const Recs);
    };
#define ROW(U, R, FORM) { "U=" #U " " #FORM, U, R, chain<U, R, FORM> }
    const Row table[] = { ROW(1, 1, STRAIGHT),  ROW(2, 1, STRAIGHT),  ROW(2, 1, ROLLED),  ROW(2, 1, LATE),
                          ROW(4, 1, STRAIGHT),  ROW(4, 1, ROLLED),    ROW(4, 1, LATE),
                          ROW(1, 16, STRAIGHT), ROW(2, 16, STRAIGHT), ROW(2, 16, ROLLED), ROW(2, 16, LATE),
                          ROW(4, 16, STRAIGHT), ROW(4, 16, ROLLED),   ROW(4, 16, LATE) };
    auto launch = [&](const Row &r, const Set &s, raw4 *o, unsigned int units) {
        const unsigned int per = r.U * 256u;
        r.kernel<<<(units + per - 1) / per, 256>>>(s.a, s.b, o, units, P);
    };

    // every form against U = 1 of the same R, on a unit count that straddles the guards; the tail must stay untouched
    {
        const unsigned int units = n - 3u;
        std::vector<char> ref(big), got(big);
        for (const Row &r : table) {
            CK(hipMemset(out[0], 0, big));
            launch(r, in[0], out[0], units);
            CK(hipDeviceSynchronize());
            CK(hipMemcpy(r.U == 1 ? ref.data() : got.data(), out[0], big, hipMemcpyDeviceToHost));
            if (r.U != 1 && std::memcmp(ref.data(), got.data(), big) != 0) {
                std::fprintf(stderr, "%s R=%d differs from U=1\n", r.name, r.R);
                return 1;
            }
        }
        std::printf("all forms byte-identical to U=1 on %u units\n", units);
    }

    auto run = [&](const Row &r, bool cold) {
        int flip = 0, rot = 0;
        auto one = [&] { launch(r, in[cold ? rot++ % 3 : 0], out[flip++ & 1], n); };
        for (int i = 0; i < 20; ++i) one();
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(e0));
        for (int i = 0; i < 100; ++i) one();
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        CK(hipGetLastError());
        return ms * 10.f;  // us per launch
    };
    for (const Row &r : table) {
        const float warm = run(r, false), cold = run(r, true);
        std::printf("R=%-2d %-14s warm %6.2f us  cold %6.2f us\n", r.R, r.name, warm, cold);
    }
    return 0;
}
