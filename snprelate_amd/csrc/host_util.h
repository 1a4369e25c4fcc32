// Host layer of the one-shot C ABI calls (ld.hip, ld_prune.hip, ibd.hip, pop.hip, qc.hip): what every such call does around
// its kernels -- refuse bad arguments before any HIP call, open a stream on the caller's device, own device buffers for the
// length of the call, stream the genotype rows through a staging buffer, time phases with HIP events, hand results back.
// A new entry point is a kernel file, its launch declarations and one function written with these pieces.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "snpgpu_internal.h"

namespace snpgpu {

inline int fail(const char *fn, const std::string &msg) { set_error(std::string(fn) + ": " + msg); return 1; }

// a size from the environment (staging bytes, a forced block size): the variable's value when it is positive, else `fallback`
inline size_t env_bytes(const char *name, size_t fallback)
{
    const char *e = getenv(name);
    return e && atoll(e) > 0 ? (size_t)atoll(e) : fallback;
}

// ---- argument checks (no HIP call) -------------------------------------------------------------------------------------------
// The ranges a call accepts: n_samp in [samp_min, samp_end), n_snp in [1, snp_end); samp_msg states the sample range.
struct GenoLimits {
    int64_t samp_min, samp_end, snp_end;
    bool packed2_only;
    const char *samp_msg;
};
constexpr int64_t NO_LIMIT = INT64_MAX;
// the LD table kernels: int sample / SNP indices, 24-bit counters per table cell
constexpr GenoLimits LD_GENO = {1, int64_t(1) << 24, int64_t(1) << 30, false, "invalid number of samples (1 ... 2^24 - 1)"};

inline int check_dims(const char *fn, int64_t n_snp, int64_t n_samp, const GenoLimits &lim)
{
    if (n_snp < 1) return fail(fn, "invalid number of SNPs: no SNP in the working dataset");
    if (n_snp >= lim.snp_end)
        return fail(fn, "invalid number of SNPs: too many SNPs (< 2^" + std::to_string(63 - __builtin_clzll((unsigned long long)lim.snp_end)) + ")");
    if (n_samp < lim.samp_min || n_samp >= lim.samp_end) return fail(fn, lim.samp_msg);
    return 0;
}

inline int check_geno(const char *fn, const void *geno, int64_t n_snp, int64_t n_samp, int format, int mem, const GenoLimits &lim)
{
    if (!geno) return fail(fn, "NULL argument: geno is NULL");
    if (check_dims(fn, n_snp, n_samp, lim)) return 1;
    if (lim.packed2_only && format != SNPGPU_GENO_PACKED2)
        return fail(fn, "invalid genotype format: genotypes must be SNPGPU_GENO_PACKED2 rows");
    if (format != SNPGPU_GENO_U8 && format != SNPGPU_GENO_PACKED2) return fail(fn, "invalid genotype format");
    if (mem != SNPGPU_HOST && mem != SNPGPU_DEVICE) return fail(fn, "invalid memory kind");
    return 0;
}

// ---- device, stream ----------------------------------------------------------------------------------------------------------
// makes `device` the calling thread's current device
inline int use_device(const char *fn, int device)
{
    int ndev = 0;
    SNPGPU_HIP_CHECK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(fn, "no HIP device (the GPU path has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(fn, "invalid device ordinal");
    SNPGPU_HIP_CHECK(hipSetDevice(device));
    return 0;
}

// The stream of one call (or of one streaming object): the caller's, or a non-blocking one that is synchronised and destroyed
// with this object.  Declare it before the DevArena of the call, so that the buffers go first.
struct CallStream {
    hipStream_t s = nullptr;
    bool own = false;
    CallStream() = default;
    CallStream(const CallStream &) = delete;
    CallStream &operator=(const CallStream &) = delete;
    ~CallStream()
    {
        if (!own) return;
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    int open(const char *fn, int device, void *user_stream = nullptr)
    {
        if (use_device(fn, device)) return 1;
        if (user_stream) { s = (hipStream_t)user_stream; return 0; }
        const hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (e != hipSuccess) { s = nullptr; return fail(fn, std::string("hipStreamCreate failed: ") + hipGetErrorString(e)); }
        own = true;
        return 0;
    }
};

// ---- device buffers of one call ----------------------------------------------------------------------------------------------
struct DevArena {
    std::vector<DevBuf *> all;
    DevArena() = default;
    DevArena(const DevArena &) = delete;
    DevArena &operator=(const DevArena &) = delete;
    ~DevArena() { for (DevBuf *b : all) delete b; }
    // A buffer of `bytes`, or nullptr with rc set: when this allocation fails, or when rc was set already (so a run of get()s
    // needs one test of rc after it -- and nothing of the run may be dereferenced before that test).
    DevBuf *get(size_t bytes, int &rc)
    {
        if (rc) return nullptr;
        DevBuf *b = new DevBuf;
        all.push_back(b);
        rc = b->alloc(bytes);
        return rc ? nullptr : b;
    }
};

// A device view of a caller's array: the caller's pointer when it is device memory (or NULL), else a temporary from the arena
// that close() copies back.  keep: the temporary starts as a copy of the caller's array (inputs, partly written outputs).
struct HostOut {
    void *user = nullptr, *dev = nullptr;
    size_t bytes = 0;
    int mem = 0;
    int open(DevArena &arena, void *u, size_t b, int m, bool keep, hipStream_t s)
    {
        user = u; bytes = b; mem = m;
        if (!u) return 0;
        if (m == SNPGPU_DEVICE) { dev = u; return 0; }
        int rc = 0;
        DevBuf *tmp = arena.get(b, rc);
        if (rc) return 1;
        dev = tmp->p;
        if (keep) SNPGPU_HIP_CHECK(hipMemcpyAsync(dev, u, b, hipMemcpyHostToDevice, s));
        return 0;
    }
    int close(hipStream_t s)
    {
        if (user && mem != SNPGPU_DEVICE) SNPGPU_HIP_CHECK(hipMemcpyAsync(user, dev, bytes, hipMemcpyDeviceToHost, s));
        return 0;
    }
};

// ---- phase timing with HIP events --------------------------------------------------------------------------------------------
// begin(phase) ... end() around work on one stream; events exist only while `on`.  The sums want the stream synchronised.
struct EventLog {
    struct Span { int phase; hipEvent_t a, b; };
    bool on = false;
    std::vector<Span> spans;
    EventLog() = default;
    EventLog(const EventLog &) = delete;
    EventLog &operator=(const EventLog &) = delete;
    ~EventLog() { clear(); }
    void clear()
    {
        for (Span &e : spans) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
        spans.clear();
    }
    int begin(int phase, hipStream_t s)
    {
        if (!on) return 0;
        hipEvent_t a, b;
        SNPGPU_HIP_CHECK(hipEventCreate(&a));
        if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); set_error("hipEventCreate failed"); return 1; }
        spans.push_back({phase, a, b});
        SNPGPU_HIP_CHECK(hipEventRecord(a, s));
        return 0;
    }
    int end(hipStream_t s)
    {
        if (on) SNPGPU_HIP_CHECK(hipEventRecord(spans.back().b, s));
        return 0;
    }
    // waits for the span that was ended last and adds its time to *ms (the per-block statistics of pop.hip and qc.hip)
    int wait_last(double *ms)
    {
        float t = 0;
        SNPGPU_HIP_CHECK(hipEventSynchronize(spans.back().b));
        SNPGPU_HIP_CHECK(hipEventElapsedTime(&t, spans.back().a, spans.back().b));
        *ms += t;
        return 0;
    }
    int sum_ms(int phase, double *ms) const
    {
        double sum = 0;
        for (const Span &e : spans) {
            if (e.phase != phase) continue;
            float t = 0;
            SNPGPU_HIP_CHECK(hipEventElapsedTime(&t, e.a, e.b));
            sum += t;
        }
        *ms = sum;
        return 0;
    }
    int64_t count(int phase) const
    {
        int64_t n = 0;
        for (const Span &e : spans) n += e.phase == phase;
        return n;
    }
};

// What a one-shot call holds from its argument checks to its return; destroyed in the order timer, buffers, stream.
struct Call {
    CallStream st;
    DevArena bufs;
    EventLog log;
    int open(const char *fn, int device, bool timed, void *user_stream = nullptr)
    {
        log.on = timed;
        return st.open(fn, device, user_stream);
    }
    // open() with timing, then the checks that need the runtime: the caller's stream and every pointer of dev_ptrs that is
    // device memory (NULL and what the runtime does not know are skipped) belong to `device`
    int open_on(const char *fn, int device, void *user_stream, const std::vector<const void *> &dev_ptrs)
    {
        if (open(fn, device, true, user_stream)) return 1;
        if (user_stream) {
            hipDevice_t d = -1;
            if (hipStreamGetDevice(st.s, &d) == hipSuccess && (int)d != device) return fail(fn, "the stream belongs to another device");
        }
        for (const void *p : dev_ptrs) {
            hipPointerAttribute_t a;
            if (!p) continue;
            if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); continue; }
            if (a.type == hipMemoryTypeDevice && a.device != device) return fail(fn, "a device pointer of another device");
        }
        return 0;
    }
};

// ---- genotype rows in SNP blocks ---------------------------------------------------------------------------------------------
// Streams n_snp caller rows to a per-block function as 2-bit rows of `rb` bytes in device memory: 2-bit device rows where they
// lie (one block unless a block size is forced), host rows through one staging buffer of stage_bytes, one-byte genotypes
// through launch_repack.  Blocks are multiples of 16 SNPs (whole 16-byte lines of 2-bit words: every block starts on the same
// line offset), at most max_block_snps; the environment variable `env_name` forces a block size for every input kind (e.g. to
// test the streaming).
struct RowBlocks {
    const uint8_t *geno = nullptr;
    int64_t n_snp = 0, N = 0, rb_in = 0, rb = 0, B = 0;
    int format = 0;
    DevBuf *raw = nullptr, *packed = nullptr;
    int open(DevArena &arena, const void *g, int64_t n_snp_, int64_t n_samp, int format_, int mem, size_t stage_bytes,
             int64_t max_block_snps, const char *env_name)
    {
        geno = (const uint8_t *)g; n_snp = n_snp_; N = n_samp; format = format_;
        const bool repack = format == SNPGPU_GENO_U8;
        rb_in = repack ? N : (N + 3) / 4;
        rb = repack ? (N + 255) / 256 * 64 : rb_in;
        B = (mem == SNPGPU_DEVICE && !repack) ? (n_snp + 15) / 16 * 16 : (int64_t)(stage_bytes / (size_t)rb_in);
        B = (int64_t)env_bytes(env_name, (size_t)B);
        B = std::min(B, max_block_snps);
        B = std::max<int64_t>(16, B / 16 * 16);
        B = std::min(B, (n_snp + 15) / 16 * 16);
        int rc = 0;
        if (mem == SNPGPU_HOST) raw = arena.get((size_t)(B * rb_in) + 32, rc);
        if (repack) packed = arena.get((size_t)(B * rb) + 32, rc);
        return rc;
    }
    // where fn will read the first block (every block of a staged input)
    const uint8_t *first() const { return packed ? (const uint8_t *)packed->p : raw ? (const uint8_t *)raw->p : geno; }
    // fn(src, rb, i0, nb): nb rows from SNP i0 at src, valid on stream s until fn's work on s is complete
    template <class F> int for_each(hipStream_t s, F &&fn)
    {
        for (int64_t i0 = 0; i0 < n_snp; i0 += B) {
            const int64_t nb = std::min(B, n_snp - i0);
            const uint8_t *src = geno + i0 * rb_in;
            if (raw) {
                SNPGPU_HIP_CHECK(hipMemcpyAsync(raw->p, src, (size_t)(nb * rb_in), hipMemcpyHostToDevice, s));
                src = (const uint8_t *)raw->p;
            }
            if (packed) {
                if (launch_repack(s, src, format, nb, N, (uint8_t *)packed->p, rb)) return 1;
                src = (const uint8_t *)packed->p;
            }
            if (fn(src, rb, i0, nb)) return 1;
            SNPGPU_HIP_CHECK(hipStreamSynchronize(s));                // the staging buffers are reused by the next block
        }
        return 0;
    }
};

// ---- LD staging rows ---------------------------------------------------------------------------------------------------------
constexpr size_t LD_RAW_BYTES = size_t(64) << 20;      // host rows go to the device in copies of at most this

// n caller rows at src -> staging rows of rbp bytes at dst (kernels_ld.hip).  Host memory goes through `raw`, at most
// LD_RAW_BYTES per copy (allocated on the first host call, sized by the rows actually given).  Nothing waits for the stream.
inline int stage_ld_rows(hipStream_t s, DevBuf &raw, const uint8_t *src, int64_t n, int64_t n_samp, int64_t rbp, int format, int mem,
                         uint8_t *dst)
{
    if (mem == SNPGPU_DEVICE) return launch_ld_stage(s, src, format, n, n_samp, rbp, dst);
    const int64_t irb = format == SNPGPU_GENO_U8 ? n_samp : (n_samp + 3) / 4;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)LD_RAW_BYTES / irb));
    if (raw.bytes < (size_t)(chunk * irb)) {
        SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
        raw.release();
        if (raw.alloc((size_t)(chunk * irb))) return 1;
    }
    for (int64_t o = 0; o < n; o += chunk) {
        const int64_t m = std::min(chunk, n - o);
        SNPGPU_HIP_CHECK(hipMemcpyAsync(raw.p, src + o * irb, (size_t)(m * irb), hipMemcpyHostToDevice, s));
        if (launch_ld_stage(s, raw.p, format, m, n_samp, rbp, dst + o * rbp)) return 1;
    }
    return 0;
}

}  // namespace snpgpu
