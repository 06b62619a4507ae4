// Run-time specialisation of the fused chain kernel: hiprtc, the registry of compiled kernels with its worker thread, and
// the launches.  What a kernel is and what its text says: chain_codegen.cpp; its file on disk: kernel_cache.cpp.
#include <dlfcn.h>

#include <condition_variable>
#include <cstdlib>
#include <thread>

#include "chain_codegen.h"

namespace kc {

namespace {

// ---- hiprtc, bound at first use (the library loads without it; the specialiser then stays off) ----
typedef struct _hiprtcProgram *hiprtcProgram;
struct Rtc {
    void *lib = nullptr;
    int (*create)(hiprtcProgram *, const char *, const char *, int, const char **, const char **) = nullptr;
    int (*compile)(hiprtcProgram, int, const char **) = nullptr;
    int (*log_size)(hiprtcProgram, size_t *) = nullptr;
    int (*log)(hiprtcProgram, char *) = nullptr;
    int (*code_size)(hiprtcProgram, size_t *) = nullptr;
    int (*code)(hiprtcProgram, char *) = nullptr;
    int (*destroy)(hiprtcProgram *) = nullptr;
    int (*version)(int *, int *) = nullptr;
    bool ok = false;
};

void specialize_stop_at_exit();

Rtc &rtc()
{
    // bound once; the worker thread and a launch in "compile at once" mode can get here at the same time
    static Rtc r;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char *name : { "libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so" }) {
            r.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (r.lib) break;
        }
        if (!r.lib) return;
#define KC_RTC_SYM(field, sym) *(void **)(&r.field) = dlsym(r.lib, sym)
        KC_RTC_SYM(create, "hiprtcCreateProgram");
        KC_RTC_SYM(compile, "hiprtcCompileProgram");
        KC_RTC_SYM(log_size, "hiprtcGetProgramLogSize");
        KC_RTC_SYM(log, "hiprtcGetProgramLog");
        KC_RTC_SYM(code_size, "hiprtcGetCodeSize");
        KC_RTC_SYM(code, "hiprtcGetCode");
        KC_RTC_SYM(destroy, "hiprtcDestroyProgram");
        KC_RTC_SYM(version, "hiprtcVersion");
#undef KC_RTC_SYM
        r.ok = r.create && r.compile && r.log_size && r.log && r.code_size && r.code && r.destroy;
        // At process exit the worker must be gone BEFORE libhiprtc / comgr / LLVM run their own exit handlers (a
        // compile in flight while those are torn down hangs the process).  Handlers run in reverse order of
        // registration and theirs were registered by the dlopen above, so this one, registered now, runs first.
        if (r.ok) std::atexit(specialize_stop_at_exit);
    });
    return r;
}

// the parity flags of the offline build (kanter_core_amd/build.py)
const char *const kCompileOpts[] = { "--gpu-architecture=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math",
                                     "-fhip-fp32-correctly-rounded-divide-sqrt" };
constexpr int kNumCompileOpts = (int)(sizeof kCompileOpts / sizeof *kCompileOpts);

}  // namespace

const CompilerId &compiler_id()
{
    static const CompilerId id = [] {
        CompilerId c{ kCompileOpts, kNumCompileOpts, { 0, 0 } };
        if (rtc().version) (void)rtc().version(&c.version[0], &c.version[1]);
        return c;
    }();
    return id;
}

// Source -> code object with hiprtc (works without a device).  KC_ERR_UNSUPPORTED: no libhiprtc.
int rtc_compile(const std::string &src, std::vector<char> &code, std::string *log)
{
    Rtc &r = rtc();
    if (!r.ok) {
        *log = "libhiprtc not available";
        return KC_ERR_UNSUPPORTED;
    }
    hiprtcProgram prog = nullptr;
    if (r.create(&prog, src.c_str(), "kc_chain_spec.hip", 0, nullptr, nullptr) != 0) {
        *log = "hiprtcCreateProgram failed";
        return KC_ERR_GENERIC;
    }
    const int rc = r.compile(prog, kNumCompileOpts, const_cast<const char **>(kCompileOpts));
    size_t n = 0;
    r.log_size(prog, &n);
    log->assign(n, '\0');
    if (n) r.log(prog, &(*log)[0]);
    if (rc == 0) {
        n = 0;
        r.code_size(prog, &n);
        code.resize(n);
        r.code(prog, code.data());
    }
    r.destroy(&prog);
    return rc == 0 ? KC_OK : KC_ERR_GENERIC;
}

namespace {

// ---- registry + worker ----
struct Entry {
    enum State { COUNTING, QUEUED, READY, FAILED } state = COUNTING;
    uint32_t sightings = 0;
    hipModule_t module = nullptr;
    hipFunction_t fn = nullptr;
};

struct Spec {
    std::mutex mu;
    std::condition_variable cv, idle_cv;
    std::unordered_map<Signature, Entry, SignatureHash> cache;
    std::deque<Signature> queue;
    std::thread worker;
    bool worker_running = false, stopping = false;
    int busy = 0;
    std::atomic<int> mode{ 1 };  // 0 off, 1 compile in the background, 2 compile at once (the launch waits); read without the lock by launches
    uint32_t after = 2;  // sightings of a program before it is worth a compile (mode 1)
    int device = -1;
    uint64_t compiled = 0, failed = 0, launches = 0, loaded_from_disk = 0;
    std::string last_log;

    // Drops what is queued, waits for the compile in flight (if any) and ends the worker.  Programs that were
    // waiting go back to "not seen yet", so a later mode change can pick them up again.
    void stop()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            stopping = true;
            for (auto &sig : queue) {
                auto it = cache.find(sig);
                if (it != cache.end() && it->second.state == Entry::QUEUED) it->second = Entry{};
            }
            queue.clear();
        }
        cv.notify_all();
        idle_cv.notify_all();
        if (worker.joinable()) worker.join();
        std::lock_guard<std::mutex> lk(mu);
        worker_running = false;
        stopping = false;
    }
};

Spec &spec()
{
    static Spec *s = new Spec();  // never destroyed: stopped explicitly (kc_shutdown, exit handler), see rtc()
    return *s;
}

void specialize_stop_at_exit() { spec().stop(); }

// How make_ready came by a kernel.
struct Ready {
    enum How { FAILED, FROM_DISK, COMPILED } how = FAILED;
    hipModule_t module = nullptr;
    hipFunction_t fn = nullptr;
    std::string log;
};

bool load_code(const Signature &sig, const std::vector<char> &code, Ready &r)
{
    if (hipModuleLoadData(&r.module, code.data()) != hipSuccess) {
        (void)hipGetLastError();
        r.log = "hipModuleLoadData failed";
        return false;
    }
    if (hipModuleGetFunction(&r.fn, r.module, kernel_name(sig).c_str()) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipModuleUnload(r.module);
        r.module = nullptr;
        r.log = "hipModuleGetFunction failed";
        return false;
    }
    return true;
}

// The kernel of one signature on the bound device: from the directories if a trustworthy code object is there, else
// compiled (and written there).  `disk_only`: never compile.
Ready make_ready(const Signature &sig, bool disk_only)
{
    Ready r;
    const std::string src = generate(sig);
    if (src.empty()) {
        r.log = "unknown step code";
        return r;
    }
    std::vector<char> code;
    if (disk_load(sig, src, compiler_id(), code)) {
        if (load_code(sig, code, r)) {
            r.how = Ready::FROM_DISK;
            return r;
        }
        disk_load_refused();  // compile
    }
    if (disk_only) {
        r.log = "not in the kernel cache";
        return r;
    }
    if (rtc_compile(src, code, &r.log) != KC_OK || !load_code(sig, code, r)) return r;
    disk_store(sig, src, compiler_id(), code);
    r.how = Ready::COMPILED;
    return r;
}

// Books what make_ready brought (S.mu held); the kernel, if there is one.
hipFunction_t finish(Spec &S, const Signature &sig, const Ready &r)
{
    auto it = S.cache.find(sig);
    if (it == S.cache.end()) {
        if (r.module) (void)hipModuleUnload(r.module);
        return nullptr;
    }
    Entry &e = it->second;
    if (r.how == Ready::FAILED) {
        e.state = Entry::FAILED;
        S.failed++;
        S.last_log = r.log;
        return nullptr;
    }
    e.module = r.module;
    e.fn = r.fn;
    e.state = Entry::READY;
    (r.how == Ready::FROM_DISK ? S.loaded_from_disk : S.compiled)++;
    return e.fn;
}

void worker_main()
{
    Spec &S = spec();
    if (S.device >= 0) (void)hipSetDevice(S.device);
    std::unique_lock<std::mutex> lk(S.mu);
    for (;;) {
        S.cv.wait(lk, [&] { return S.stopping || !S.queue.empty(); });
        if (S.stopping) return;
        const Signature sig = S.queue.front();
        S.queue.pop_front();
        S.busy++;
        lk.unlock();
        const Ready r = make_ready(sig, /*disk_only=*/false);
        lk.lock();
        S.busy--;
        finish(S, sig, r);
        S.idle_cv.notify_all();  // specialize_wait() waits for "nothing pending", mode-2 launches for one entry
    }
}

// The specialised kernel for this program if there is one; otherwise nullptr (and, depending on the mode,
// a compile is started).  Called with the context lock held.  A launch that finds its kernel READY takes the
// registry lock once and allocates nothing.
hipFunction_t spec_lookup(const Signature &sig)
{
    Spec &S = spec();
    if (S.mode.load(std::memory_order_relaxed) == 0) return nullptr;
    std::unique_lock<std::mutex> lk(S.mu);
    auto it = S.cache.find(sig);
    if (it != S.cache.end() && it->second.state == Entry::READY) return it->second.fn;
    // "compile at once": a compile of this program that is already queued in the background is waited for
    if (S.mode == 2 && it != S.cache.end() && it->second.state == Entry::QUEUED)
        S.idle_cv.wait(lk, [&] {
            auto w = S.cache.find(sig);
            return w == S.cache.end() || w->second.state != Entry::QUEUED || !S.worker_running;
        });
    Entry &e = S.cache[sig];
    if (e.state == Entry::READY) return e.fn;
    if (e.state != Entry::COUNTING) return nullptr;
    e.sightings++;
    if (e.sightings == 1 && S.mode == 1) {
        // first sighting in this process: a code object from an earlier process (or from the build) is loaded on the spot
        const Ready r = make_ready(sig, /*disk_only=*/true);
        if (r.how != Ready::FAILED) return finish(S, sig, r);
    }
    if (S.mode == 1 && e.sightings < S.after) return nullptr;
    e.state = Entry::QUEUED;
    if (S.mode == 2) {
        lk.unlock();
        const Ready r = make_ready(sig, /*disk_only=*/false);
        lk.lock();
        return finish(S, sig, r);
    }
    S.queue.push_back(sig);
    if (!S.worker_running) {
        S.device = ctx().device;
        S.stopping = false;
        S.worker = std::thread(worker_main);
        S.worker_running = true;
    }
    lk.unlock();
    S.cv.notify_one();
    return nullptr;
}

void count_launch()
{
    std::lock_guard<std::mutex> lk(spec().mu);
    spec().launches++;
}

}  // namespace

// Launches the specialised kernel for P if one is ready.  *launched tells the caller whether it still has to
// run the interpreter; *nt_mask (optional) receives the cache-policy bits the launched kernel was compiled with.
hipError_t launch_chain_specialized(const ChainProgram &P, int batch, hipStream_t s, bool *launched, uint32_t *nt_mask, uint32_t *quads)
{
    *launched = false;
    if (P.n_ops < 1 || P.n_ops > (uint32_t)KC_CHAIN_MAX_OPS || P.n_in > (uint32_t)KC_CHAIN_MAX_IN) return hipSuccess;
    const uint64_t total = (uint64_t)P.rows * P.row_units;
    if (total == 0 || total > 0xFFFFFFFFull) return hipSuccess;
    const Signature sig = signature_of(P);
    hipFunction_t fn = spec_lookup(sig);
    if (!fn) return hipSuccess;
    size_t size = sizeof(ChainProgram);
    const int SPEC_WG = spec_wg();
    void *extra[] = { HIP_LAUNCH_PARAM_BUFFER_POINTER, (void *)&P, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END };
    const uint64_t per_block = (uint64_t)SPEC_WG * sig.quads;  // the generator's own count (chain_codegen.cpp, emit_quads)
    const unsigned gx = (unsigned)((total + per_block - 1) / per_block);
    hipError_t e = hipModuleLaunchKernel(fn, gx, (unsigned)batch, 1, SPEC_WG, 1, 1, 0, s, nullptr, extra);
    if (e == hipSuccess) {
        *launched = true;
        if (nt_mask) *nt_mask = sig.nt_mask;
        if (quads) *quads = sig.quads;
        count_launch();
    }
    return e;
}

// The same for a program that runs inside the integer-ratio up-sampling kernel (resize.cpp, chain_resize_launch).
hipError_t launch_upsample_chain_specialized(const ChainProgram &P, int batch, const UpsampleArgs &U, hipStream_t s, bool *launched)
{
    *launched = false;
    if (P.n_ops < 1 || P.n_ops > (uint32_t)KC_CHAIN_MAX_OPS || P.n_in < 1 || P.n_in > (uint32_t)KC_CHAIN_INTERP_IN) return hipSuccess;
    if (!upsample_args_ok(U, batch) || (U.H.taps != 1 && U.H.taps != 3)) return hipSuccess;
    if (U.H.ratio == 2) return hipSuccess;  // the half-quad form exists ahead of time only (upsample_chain_kernel<.., true>)
    hipFunction_t fn = spec_lookup(signature_of(P, &U));
    if (!fn) return hipSuccess;
    struct alignas(16) Params {
        ChainProgram P;
        UpsampleArgs U;
    };
    static_assert(sizeof(ChainProgram) % alignof(UpsampleArgs) == 0, "the second kernel argument follows the first without padding");
    static thread_local Params params;
    params.P = P;
    params.U = U;
    size_t size = sizeof(Params);
    void *extra[] = { HIP_LAUNCH_PARAM_BUFFER_POINTER, (void *)&params, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END };
    const dim3 grid = upsample_grid(U, batch);
    hipError_t e = hipModuleLaunchKernel(fn, grid.x, grid.y, grid.z, 256, 1, 1, (unsigned)upsample_lds_bytes(U), s, nullptr, extra);
    if (e == hipSuccess) {
        *launched = true;
        count_launch();
    }
    return e;
}

int specialize_set_mode(int mode, int after)
{
    Spec &S = spec();
    if (mode < 0 || mode > 2) return KC_ERR_INVALID_ARG;
    {
        std::lock_guard<std::mutex> lk(S.mu);
        S.mode.store(mode);
        if (after >= 1) S.after = (uint32_t)after;
    }
    if (mode == 0) S.stop();  // off: nothing stays queued, no thread stays behind
    return KC_OK;
}

int specialize_get_mode() { return spec().mode.load(); }

// Blocks until every queued compile has landed.
void specialize_wait()
{
    Spec &S = spec();
    std::unique_lock<std::mutex> lk(S.mu);
    S.idle_cv.wait(lk, [&] { return S.stopping || (S.queue.empty() && S.busy == 0); });
}

void specialize_stats(uint64_t *compiled, uint64_t *failed, uint64_t *launches, uint64_t *pending)
{
    Spec &S = spec();
    std::lock_guard<std::mutex> lk(S.mu);
    if (compiled) *compiled = S.compiled;
    if (failed) *failed = S.failed;
    if (launches) *launches = S.launches;
    if (pending) *pending = S.queue.size() + (uint64_t)S.busy;
}

void kernel_cache_stats(uint64_t *hits, uint64_t *rejected, uint64_t *written, uint64_t *kernels_loaded)
{
    disk_counters(hits, rejected, written);
    Spec &S = spec();
    std::lock_guard<std::mutex> lk(S.mu);
    if (kernels_loaded) *kernels_loaded = S.loaded_from_disk;
}

std::string specialize_last_log()
{
    Spec &S = spec();
    std::lock_guard<std::mutex> lk(S.mu);
    return S.last_log;
}

// kc_shutdown: the worker is stopped and every module unloaded before the device goes away.
void specialize_shutdown()
{
    Spec &S = spec();
    S.stop();
    std::lock_guard<std::mutex> lk(S.mu);
    for (auto &kv : S.cache)
        if (kv.second.module) (void)hipModuleUnload(kv.second.module);
    S.cache.clear();
}

// Compiles without loading: lets the CPU-only test suite check that every generated program builds for
// gfx950 with the parity flags (hiprtc cross-compiles without a device).
int specialize_compile_only(const std::string &src, std::string *log)
{
    std::vector<char> code;
    return src.empty() ? KC_ERR_GENERIC : rtc_compile(src, code, log);
}

}  // namespace kc
