// ---- code objects that outlive the process ----
// hiprtc takes about two seconds for the first program of a process and the interpreter runs meanwhile; a batch job that
// evaluates one graph once per process (the reference's own usage, tests/integration_tests.rs:47-49) would never reach the
// kernel its program deserves.  So every code object the compiler produces is also written to a directory, and a program's
// FIRST sighting in a later process loads it from there (a file read and hipModuleLoadData: ~0.3 ms).
//   where   KC_KERNEL_CACHE_DIR (kc_set_kernel_cache_dir), default $XDG_CACHE_HOME/kanter_core_amd or ~/.cache/kanter_core_amd;
//           "off" disables.  Read-only second place: kernel_cache/ next to the library, which the build fills with the
//           BASELINE programs (kanter_core_amd/build.py, baseline_programs.jsonl), so that a fresh machine has them too.
//   file    <kernel name>-<hash of the signature>.kcco = header, the signature's key, the code object.
//   trust   a file is used only if its key equals the signature's byte for byte, the hash of what the generator emits TODAY for
//           that signature (source text, compiler options, hiprtc version) equals the one stored, and the code's checksum
//           holds.  Anything else -- a truncated or edited file, a file from another version of the library or of ROCm -- is
//           ignored and replaced by a fresh compile; never a wrong kernel.
//   writes  to a temporary name in the same directory, then rename(): readers see whole files only.
#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "chain_codegen.h"

namespace kc {
namespace {

uint64_t fnv64(const void *data, size_t n, uint64_t h = 1469598103934665603ull)
{
    const unsigned char *p = (const unsigned char *)data;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

struct CacheHeader {
    char magic[8];  // "KCCO0001"
    uint64_t key_len, source_hash, code_len, code_hash;
};

struct DiskCache {
    std::mutex mu;
    bool resolved = false;
    std::string write_dir;              // empty: nothing is written
    std::vector<std::string> read_dirs; // write_dir first, then the packaged directory
    uint64_t hits = 0, rejected = 0, written = 0;
};

DiskCache &disk()
{
    static DiskCache d;
    return d;
}

bool make_dirs(const std::string &path)
{
    for (size_t i = 1; i <= path.size(); ++i)
        if (i == path.size() || path[i] == '/') {
            const std::string part = path.substr(0, i);
            if (mkdir(part.c_str(), 0755) != 0 && errno != EEXIST) return false;
        }
    return true;
}

void resolve_dirs_locked(DiskCache &d, const char *forced)
{
    d.resolved = true;
    d.write_dir.clear();
    d.read_dirs.clear();
    std::string dir;
    if (forced) dir = forced;
    else if (const char *e = std::getenv("KC_KERNEL_CACHE_DIR")) dir = e;
    else if (const char *x = std::getenv("XDG_CACHE_HOME")) dir = *x ? std::string(x) + "/kanter_core_amd" : "";
    else if (const char *h = std::getenv("HOME")) dir = *h ? std::string(h) + "/.cache/kanter_core_amd" : "";
    if (dir == "off" || dir == "0") return;  // no cache at all
    if (!dir.empty() && make_dirs(dir) && access(dir.c_str(), W_OK) == 0) {
        d.write_dir = dir;
        d.read_dirs.push_back(dir);
    } else if (!dir.empty()) {
        d.read_dirs.push_back(dir);  // readable perhaps, even if it cannot be written
    }
    Dl_info info;
    if (dladdr((const void *)&disk, &info) && info.dli_fname) {
        std::string lib = info.dli_fname;
        const size_t slash = lib.rfind('/');
        d.read_dirs.push_back((slash == std::string::npos ? std::string(".") : lib.substr(0, slash)) + "/kernel_cache");
    }
}

std::string cache_file_name(const Signature &sig, const std::string &key)
{
    char buf[64];
    std::snprintf(buf, sizeof buf, "-%016llx.kcco", (unsigned long long)fnv64(key.data(), key.size()));
    return kernel_name(sig) + buf;
}

// What today's generator and compiler would make of this signature, as a hash.
uint64_t source_hash_of(const std::string &src, const CompilerId &cc)
{
    uint64_t h = fnv64(src.data(), src.size());
    for (int i = 0; i < cc.n_opts; ++i) h = fnv64(cc.opts[i], std::strlen(cc.opts[i]) + 1, h);
    return fnv64(cc.version, sizeof cc.version, h);
}

bool disk_store_in(const std::string &dir, const Signature &sig, const std::string &src, const CompilerId &cc, const std::vector<char> &code)
{
    const std::string key = sig.key(), final_name = dir + "/" + cache_file_name(sig, key);
    char tmp_suffix[48];
    std::snprintf(tmp_suffix, sizeof tmp_suffix, ".tmp.%d.%llx", (int)getpid(), (unsigned long long)fnv64(&code, sizeof(void *)));
    const std::string tmp = final_name + tmp_suffix;
    FILE *f = std::fopen(tmp.c_str(), "wb");
    if (!f) return false;
    CacheHeader h{};
    std::memcpy(h.magic, "KCCO0001", 8);
    h.key_len = key.size();
    h.source_hash = source_hash_of(src, cc);
    h.code_len = code.size();
    h.code_hash = fnv64(code.data(), code.size());
    bool ok = std::fwrite(&h, sizeof h, 1, f) == 1 && std::fwrite(key.data(), 1, key.size(), f) == key.size() &&
              std::fwrite(code.data(), 1, code.size(), f) == code.size();
    ok = std::fclose(f) == 0 && ok;
    if (ok) ok = std::rename(tmp.c_str(), final_name.c_str()) == 0;
    if (!ok) (void)std::remove(tmp.c_str());
    return ok;
}

void mark_populated(const std::string &dir)
{
    if (FILE *f = std::fopen((dir + "/.populated").c_str(), "w")) std::fclose(f);
}

}  // namespace

// The code object of `sig` from the directories, if a trustworthy one is there.
bool disk_load(const Signature &sig, const std::string &src, const CompilerId &cc, std::vector<char> &code)
{
    DiskCache &d = disk();
    std::vector<std::string> dirs;
    {
        std::lock_guard<std::mutex> lk(d.mu);
        if (!d.resolved) resolve_dirs_locked(d, nullptr);
        dirs = d.read_dirs;
    }
    if (dirs.empty()) return false;
    const std::string key = sig.key(), name = cache_file_name(sig, key);
    const uint64_t want = source_hash_of(src, cc);
    for (auto &dir : dirs) {
        FILE *f = std::fopen((dir + "/" + name).c_str(), "rb");
        if (!f) continue;
        CacheHeader h{};
        bool ok = std::fread(&h, sizeof h, 1, f) == 1 && std::memcmp(h.magic, "KCCO0001", 8) == 0 && h.key_len == key.size() &&
                  h.source_hash == want && h.code_len > 0 && h.code_len < (64u << 20);
        std::string fkey;
        if (ok) {
            fkey.resize(h.key_len);
            code.resize(h.code_len);
            ok = std::fread(&fkey[0], 1, fkey.size(), f) == fkey.size() && fkey == key &&
                 std::fread(code.data(), 1, code.size(), f) == code.size() && std::fgetc(f) == EOF &&
                 fnv64(code.data(), code.size()) == h.code_hash;
        }
        std::fclose(f);
        std::lock_guard<std::mutex> lk(d.mu);
        if (ok) {
            d.hits++;
            return true;
        }
        d.rejected++;
    }
    code.clear();
    return false;
}

// The file disk_load accepted passed every check and the driver still refuses its code.
void disk_load_refused()
{
    std::lock_guard<std::mutex> lk(disk().mu);
    disk().hits--;
    disk().rejected++;
}

// After a compile: the code object into the directory that is written, and the program onto the list of what this run compiled
// where KC_KERNEL_CACHE_MANIFEST names one (tools/dump_baseline_programs.sh).
void disk_store(const Signature &sig, const std::string &src, const CompilerId &cc, const std::vector<char> &code)
{
    DiskCache &d = disk();
    std::string dir;
    {
        std::lock_guard<std::mutex> lk(d.mu);
        if (!d.resolved) resolve_dirs_locked(d, nullptr);
        dir = d.write_dir;
    }
    if (!dir.empty() && disk_store_in(dir, sig, src, cc, code)) {
        std::lock_guard<std::mutex> lk(d.mu);
        if (d.written++ == 0) mark_populated(dir);
    }
    const char *m = std::getenv("KC_KERNEL_CACHE_MANIFEST");
    FILE *f = m ? std::fopen(m, "a") : nullptr;
    if (!f) return;
    std::fprintf(f, "{\"name\": \"%s\", \"n_in\": %u, \"start_src\": %d, \"flat\": %d, \"nt_mask\": %u, \"up_taps\": %u, \"up_wide\": %d, \"words\": [",
                 kernel_name(sig).c_str(), sig.n_in, sig.start_src, sig.flat ? 1 : 0, sig.nt_mask, sig.up_taps, sig.up_wide ? 1 : 0);
    for (uint32_t k = 0; k < sig.n_ops; ++k) std::fprintf(f, "%s%u", k ? ", " : "", sig.word[k]);
    if (sig.in_tiers) std::fprintf(f, "], \"in_tiers\": %u}\n", sig.in_tiers);  // (optional field: packed inputs, chain_pack.h)
    else std::fprintf(f, "]}\n");
    std::fclose(f);
}

void disk_counters(uint64_t *hits, uint64_t *rejected, uint64_t *written)
{
    DiskCache &d = disk();
    std::lock_guard<std::mutex> lk(d.mu);
    if (hits) *hits = d.hits;
    if (rejected) *rejected = d.rejected;
    if (written) *written = d.written;
}

// ---- the kernel cache from outside ----
// nullptr / "": back to the environment's choice; "off": no cache.
int kernel_cache_set_dir(const char *dir)
{
    DiskCache &d = disk();
    std::lock_guard<std::mutex> lk(d.mu);
    resolve_dirs_locked(d, dir && *dir ? dir : nullptr);
    return KC_OK;
}

// Is there anything a first evaluation could find?  (graph.cpp: whether a graph's first walk builds the wide / joined programs.)
bool kernel_cache_populated()
{
    DiskCache &d = disk();
    std::vector<std::string> dirs;
    {
        std::lock_guard<std::mutex> lk(d.mu);
        if (!d.resolved) resolve_dirs_locked(d, nullptr);
        dirs = d.read_dirs;
        if (dirs.empty()) return false;  // "off"
        if (d.hits) return true;
    }
    static std::map<std::string, bool> seen;  // per directory, asked once (callers hold the context lock)
    for (auto &dir : dirs) {
        auto it = seen.find(dir);
        if (it == seen.end()) it = seen.emplace(dir, access((dir + "/.populated").c_str(), R_OK) == 0).first;
        if (it->second) return true;
    }
    return false;
}

// Compiles the program of a signature given by value (no device needed) and writes its code object into `dir`: how the build
// pre-populates kernel_cache/ next to the library.
int kernel_cache_precompile(const uint32_t *words, uint32_t n_ops, uint32_t n_in, int32_t start_src, bool flat, uint32_t nt_mask, uint32_t in_tiers,
                            uint32_t up_taps, bool up_wide, const char *dir, std::string *log)
{
    if (!words || n_ops < 1 || n_ops > (uint32_t)KC_CHAIN_MAX_OPS || n_in > (uint32_t)KC_CHAIN_MAX_IN || !dir || !*dir) return KC_ERR_INVALID_ARG;
    if (in_tiers && (!flat || up_taps || (n_in < 16 && in_tiers >> (2 * n_in)))) return KC_ERR_INVALID_ARG;
    for (uint32_t k = 0; k < n_in; ++k)
        if (KC_CHAIN_TIER(in_tiers, k) == 3u) return KC_ERR_INVALID_ARG;
    const Signature sig = make_signature(words, n_ops, n_in, start_src, flat, nt_mask, in_tiers, up_taps, up_wide);
    const std::string src = generate(sig);
    if (src.empty()) {
        *log = "unknown step code";
        return KC_ERR_INVALID_ARG;
    }
    std::vector<char> code;
    if (const int rc = rtc_compile(src, code, log)) return rc;
    if (!make_dirs(dir) || !disk_store_in(dir, sig, src, compiler_id(), code)) {
        *log = std::string("cannot write into ") + dir;
        return KC_ERR_IO;
    }
    mark_populated(dir);
    return KC_OK;
}

}  // namespace kc
