// Diagnostics behind include/snpgpu.h (no reference counterpart): what THIS device's matrix pipe sustains right now.
//
// The SYRK / pair-counter kernels run against the socket power cap, not against the 2.4 GHz peak: a register-only
// MFMA stream with operands shaped like theirs settles at 1.7 - 1.85 GHz, one with zero operands at 2.39 GHz, and the figure moves
// by a few per cent from box to box.  bench.py therefore measures it in the run it reports (roofline.sustained_peak_measured)
// instead of quoting a constant: snpgpu_diag_mfma_rate streams one MFMA instruction from registers -- 8 independent accumulators
// per wave, 2 waves per SIMD, so the pipe never waits -- for `seconds` and returns the rate over the second half of that time.
#include "ctx_plan.h"

#include <chrono>
#include <cstring>
#include <sstream>
#include <vector>

namespace snpgpu {
namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef int v8i __attribute__((ext_vector_type(8)));

constexpr int DIAG_NT = 8, DIAG_ITERS = 2048;

__global__ __launch_bounds__(256, 2) void diag_f16_kernel(const h8 *__restrict__ src, float *__restrict__ out)
{
    h8 a[4], b[4];
    for (int i = 0; i < 4; i++) {
        a[i] = src[(threadIdx.x + 256 * i) & 1023];
        b[i] = src[1024 + ((threadIdx.x + 256 * i + 77) & 1023)];
    }
    f16v acc[DIAG_NT];
    for (int t = 0; t < DIAG_NT; t++)
        for (int r = 0; r < 16; r++) acc[t][r] = 0.f;
    for (int it = 0; it < DIAG_ITERS; it++) {
#pragma unroll
        for (int t = 0; t < DIAG_NT; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[t & 3], b[(t >> 1) & 3], acc[t], 0, 0, 0);
    }
    float s = 0;
    for (int t = 0; t < DIAG_NT; t++)
        for (int r = 0; r < 16; r++) s += acc[t][r];
    if (s == 1.2345f) out[0] = s;
}

// the same flops through v_mfma_f32_16x16x32_f16 (a quarter of the accumulator registers per instruction, half the cycles)
typedef float f4v __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256, 2) void diag_f16_16x16x32_kernel(const h8 *__restrict__ src, float *__restrict__ out)
{
    h8 a[4], b[4];
    for (int i = 0; i < 4; i++) {
        a[i] = src[(threadIdx.x + 256 * i) & 1023];
        b[i] = src[1024 + ((threadIdx.x + 256 * i + 77) & 1023)];
    }
    f4v acc[2 * DIAG_NT];
    for (int t = 0; t < 2 * DIAG_NT; t++)
        for (int r = 0; r < 4; r++) acc[t][r] = 0.f;
    for (int it = 0; it < DIAG_ITERS; it++) {
#pragma unroll
        for (int t = 0; t < 2 * DIAG_NT; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[t & 3], b[(t >> 2) & 3], acc[t], 0, 0, 0);
    }
    float s = 0;
    for (int t = 0; t < 2 * DIAG_NT; t++)
        for (int r = 0; r < 4; r++) s += acc[t][r];
    if (s == 1.2345f) out[0] = s;
}

__global__ __launch_bounds__(256, 2) void diag_fp4_kernel(const v8i *__restrict__ src, float *__restrict__ out)
{
    v8i a[4], b[4];
    for (int i = 0; i < 4; i++) {
        a[i] = src[(threadIdx.x + 256 * i) & 1023];
        b[i] = src[1024 + ((threadIdx.x + 256 * i + 77) & 1023)];
    }
    f16v acc[DIAG_NT];
    for (int t = 0; t < DIAG_NT; t++)
        for (int r = 0; r < 16; r++) acc[t][r] = 0.f;
    for (int it = 0; it < DIAG_ITERS; it++) {
#pragma unroll
        for (int t = 0; t < DIAG_NT; t++)
            acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[t & 3], b[(t >> 1) & 3], acc[t], 4, 4, 0, 127, 0, 127);
    }
    float s = 0;
    for (int t = 0; t < DIAG_NT; t++)
        for (int r = 0; r < 16; r++) s += acc[t][r];
    if (s == 1.2345f) out[0] = s;
}

__global__ __launch_bounds__(256, 2) void diag_fp4_16x16x128_kernel(const v8i *__restrict__ src, float *__restrict__ out)
{
    v8i a[4], b[4];
    for (int i = 0; i < 4; i++) {
        a[i] = src[(threadIdx.x + 256 * i) & 1023];
        b[i] = src[1024 + ((threadIdx.x + 256 * i + 77) & 1023)];
    }
    f4v acc[2 * DIAG_NT];
    for (int t = 0; t < 2 * DIAG_NT; t++)
        for (int r = 0; r < 4; r++) acc[t][r] = 0.f;
    for (int it = 0; it < DIAG_ITERS; it++) {
#pragma unroll
        for (int t = 0; t < 2 * DIAG_NT; t++)
            acc[t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[t & 3], b[(t >> 2) & 3], acc[t], 4, 4, 0, 127, 0, 127);
    }
    float s = 0;
    for (int t = 0; t < 2 * DIAG_NT; t++)
        for (int r = 0; r < 4; r++) s += acc[t][r];
    if (s == 1.2345f) out[0] = s;
}

uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

}  // namespace

// fp64 vector stream: 8 independent v_fma_f64 chains per lane, operands that never leave registers
constexpr int FP64_CHAINS = 8, FP64_ITERS = 4096;
__global__ __launch_bounds__(256) void diag_fp64_kernel(const double *__restrict__ src, double *__restrict__ out)
{
    double a[FP64_CHAINS];
    const double b = src[threadIdx.x & 63], c = src[64 + (threadIdx.x & 63)];
    for (int t = 0; t < FP64_CHAINS; t++) a[t] = src[128 + t];
    for (int it = 0; it < FP64_ITERS; it++) {
#pragma unroll
        for (int t = 0; t < FP64_CHAINS; t++) a[t] = fma(a[t], b, c);
    }
    double s = 0;
    for (int t = 0; t < FP64_CHAINS; t++) s += a[t];
    if (s == 1.2345) out[0] = s;
}

}  // namespace snpgpu

using namespace snpgpu;

extern "C" int snpgpu_diag_mfma_rate(int device, int mode, double seconds, double *tflops, double *implied_mhz)
{
    if (!tflops || !(seconds > 0.0) || seconds > 30.0 || mode < 0 || mode > SNPGPU_DIAG_F16_EXACT_ROW_16X16X32) {
        set_error("snpgpu_diag_mfma_rate: invalid arguments");
        return 1;
    }
    SNPGPU_HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    SNPGPU_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
        set_error(std::string("snpgpu_diag_mfma_rate: device is ") + prop.gcnArchName + ", this library is built for gfx950 (MI355X) only");
        return 1;
    }
    // operand images: entries 0..1023 = a registers, 1024..2047 = b registers (16 bytes for fp16 x 8, 32 bytes for 64 nibbles padded)
    const bool fp4 = mode == SNPGPU_DIAG_FP4 || mode == SNPGPU_DIAG_FP4_16X16X128;
    const size_t entry = fp4 ? 32 : 16;
    std::vector<uint8_t> h(2048 * entry, 0);
    uint32_t s = 7u;
    if (mode == SNPGPU_DIAG_F16_EXACT_ROW || mode == SNPGPU_DIAG_F16_UV || mode == SNPGPU_DIAG_F16_UV_16X16X32 || mode == SNPGPU_DIAG_F16_EXACT_ROW_16X16X32) {
        _Float16 *p = (_Float16 *)h.data();
        for (int e = 0; e < 2048; e++) {
            // single-product kernel (SNPGPU_DIAG_F16_UV): both operands (g - c) x an fp16 factor of the SNP weight, g in {0,1,2},
            // c in {0,1,2}; exact-row kernel: row operand (g - c), column operand a real number y^2 (g - avg) (hi part)
            for (int k = 0; k < 8; k++) {
                const int gg = (int)(lcg(s) % 3u), cc = (int)(lcg(s) % 3u);
                const float g = (float)(gg - cc);
                const float f = 0.75f + (float)(lcg(s) % 1024u) / 1024.0f;
                const bool row = e < 1024;
                float v;
                if (mode != SNPGPU_DIAG_F16_EXACT_ROW && mode != SNPGPU_DIAG_F16_EXACT_ROW_16X16X32) v = g * f;
                else v = row ? g : ((float)(lcg(s) % 2001u) - 1000.0f) / 400.0f;
                p[e * 8 + k] = (_Float16)v;
            }
        }
    } else if (fp4) {
        uint32_t *p = (uint32_t *)h.data();
        for (int e = 0; e < 2048; e++)
            for (int w = 0; w < 4; w++) {        // 32 nibbles used per lane (the upper four dwords of the operand are ignored for fp4)
                uint32_t x = 0;
                for (int k = 0; k < 8; k++) {
                    // e2m1 codes of the counter kernels' value types: a in {0, 1/2, 1} (nibble of g / 2), b in {0, +-1}
                    const uint32_t g = lcg(s) % 3u;
                    const uint32_t code = e < 1024 ? g : (g == 0 ? 0u : g == 1 ? 2u : 0xAu);
                    x |= code << (4 * k);
                }
                p[e * 8 + w] = x;
            }
    }
    void *d_src = nullptr, *d_out = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    int rc = 1;
    do {
        if (hipMalloc(&d_src, h.size()) != hipSuccess || hipMalloc(&d_out, 64) != hipSuccess) { set_error("snpgpu_diag_mfma_rate: hipMalloc failed"); break; }
        if (hipMemcpy(d_src, h.data(), h.size(), hipMemcpyHostToDevice) != hipSuccess) { set_error("snpgpu_diag_mfma_rate: copy failed"); break; }
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { set_error("snpgpu_diag_mfma_rate: stream"); break; }
        bool ok = true;
        for (auto &e : ev) ok = ok && hipEventCreate(&e) == hipSuccess;
        if (!ok) { set_error("snpgpu_diag_mfma_rate: events"); break; }
        const int cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        const int blocks = cus * 2 * 4;       // 2 workgroups of 4 waves per CU resident, 4 rounds per launch (~3 ms)
        auto launch = [&]() {
            if (mode == SNPGPU_DIAG_FP4_16X16X128)
                hipLaunchKernelGGL(diag_fp4_16x16x128_kernel, dim3(blocks), dim3(256), 0, st, (const v8i *)d_src, (float *)d_out);
            else if (fp4) hipLaunchKernelGGL(diag_fp4_kernel, dim3(blocks), dim3(256), 0, st, (const v8i *)d_src, (float *)d_out);
            else if (mode == SNPGPU_DIAG_F16_UV_16X16X32 || mode == SNPGPU_DIAG_F16_EXACT_ROW_16X16X32)
                hipLaunchKernelGGL(diag_f16_16x16x32_kernel, dim3(blocks), dim3(256), 0, st, (const h8 *)d_src, (float *)d_out);
            else hipLaunchKernelGGL(diag_f16_kernel, dim3(blocks), dim3(256), 0, st, (const h8 *)d_src, (float *)d_out);
        };
        const double flop_per_launch = 2.0 * (fp4 ? 32.0 * 32 * 64 : 32.0 * 32 * 16) * DIAG_NT * DIAG_ITERS * 4.0 * blocks;
        // first half: the clock settles under the power cap; second half: timed with HIP events on this stream
        auto run_for = [&](double secs, long &n) {
            const auto t0 = std::chrono::steady_clock::now();
            n = 0;
            do {
                for (int i = 0; i < 8; i++) launch();
                n += 8;
                if (hipStreamSynchronize(st) != hipSuccess) return false;
            } while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < secs);
            return true;
        };
        long n1 = 0, n2 = 0;      // n1: launches of the settling half (not timed)
        if (!run_for(seconds * 0.5, n1)) { set_error("snpgpu_diag_mfma_rate: kernel failed"); break; }
        (void)hipEventRecord(ev[0], st);
        if (!run_for(seconds * 0.5, n2)) { set_error("snpgpu_diag_mfma_rate: kernel failed"); break; }
        (void)hipEventRecord(ev[1], st);
        if (hipEventSynchronize(ev[1]) != hipSuccess) { set_error("snpgpu_diag_mfma_rate: sync failed"); break; }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
        if (!(ms > 0.f)) { set_error("snpgpu_diag_mfma_rate: no time measured"); break; }
        const double rate = flop_per_launch * (double)n2 / ((double)ms * 1e-3) / 1e12;
        *tflops = rate;
        // the stream is issue-bound on the matrix pipe: rate / (flop per clock of the whole device) = the shader clock it ran at
        if (implied_mhz) *implied_mhz = rate * 1e12 / ((double)cus * 4.0 * (fp4 ? 4096.0 : 1024.0)) / 1e6;
        rc = 0;
    } while (0);
    for (auto &e : ev) if (e) (void)hipEventDestroy(e);
    if (st) (void)hipStreamDestroy(st);
    if (d_src) (void)hipFree(d_src);
    if (d_out) (void)hipFree(d_out);
    return rc;
}

extern "C" int snpgpu_diag_device_pci(int device, char *buf, int len)
{
    if (!buf || len < 16) { set_error("snpgpu_diag_device_pci: buffer of at least 16 bytes needed"); return 1; }
    SNPGPU_HIP_CHECK(hipDeviceGetPCIBusId(buf, len, device));
    return 0;
}

extern "C" int snpgpu_diag_fp64_rate(int device, double seconds, double *tflops)
{
    if (!tflops || !(seconds > 0.0) || seconds > 30.0) { set_error("snpgpu_diag_fp64_rate: invalid arguments"); return 1; }
    SNPGPU_HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    SNPGPU_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    std::vector<double> h(256);
    for (int i = 0; i < 64; i++) { h[i] = 0.999 + 1e-6 * i; h[64 + i] = 1e-3 * (i % 7); }
    for (int i = 128; i < 256; i++) h[i] = 0.5 + 1e-3 * i;
    void *d_src = nullptr, *d_out = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    int rc = 1;
    do {
        if (hipMalloc(&d_src, h.size() * sizeof(double)) != hipSuccess || hipMalloc(&d_out, 64) != hipSuccess) { set_error("snpgpu_diag_fp64_rate: hipMalloc failed"); break; }
        if (hipMemcpy(d_src, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { set_error("snpgpu_diag_fp64_rate: copy failed"); break; }
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { set_error("snpgpu_diag_fp64_rate: stream"); break; }
        bool ok = true;
        for (auto &e : ev) ok = ok && hipEventCreate(&e) == hipSuccess;
        if (!ok) { set_error("snpgpu_diag_fp64_rate: events"); break; }
        const int cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        const int blocks = cus * 2 * 4;       // 8 waves per CU resident (2 per SIMD), 4 rounds per launch
        const double flop_per_launch = 2.0 * FP64_CHAINS * FP64_ITERS * 256.0 * blocks;
        auto run_for = [&](double secs, long &n) {
            const auto t0 = std::chrono::steady_clock::now();
            n = 0;
            do {
                for (int i = 0; i < 8; i++)
                    hipLaunchKernelGGL(diag_fp64_kernel, dim3(blocks), dim3(256), 0, st, (const double *)d_src, (double *)d_out);
                n += 8;
                if (hipStreamSynchronize(st) != hipSuccess) return false;
            } while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < secs);
            return true;
        };
        long n1 = 0, n2 = 0;
        if (!run_for(seconds * 0.5, n1)) { set_error("snpgpu_diag_fp64_rate: kernel failed"); break; }
        (void)hipEventRecord(ev[0], st);
        if (!run_for(seconds * 0.5, n2)) { set_error("snpgpu_diag_fp64_rate: kernel failed"); break; }
        (void)hipEventRecord(ev[1], st);
        if (hipEventSynchronize(ev[1]) != hipSuccess) { set_error("snpgpu_diag_fp64_rate: sync failed"); break; }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
        if (!(ms > 0.f)) { set_error("snpgpu_diag_fp64_rate: no time measured"); break; }
        *tflops = flop_per_launch * (double)n2 / ((double)ms * 1e-3) / 1e12;
        rc = 0;
    } while (0);
    for (auto &e : ev) if (e) (void)hipEventDestroy(e);
    if (st) (void)hipStreamDestroy(st);
    if (d_src) (void)hipFree(d_src);
    if (d_out) (void)hipFree(d_out);
    return rc;
}

// work items of syrk_uv16c_kernel that found no free slot of the carry scratch since the context was created or the count was last
// reset (they took the per-run atomics instead: slower, never wrong)
extern "C" int snpgpu_diag_carry_fallbacks(snpgpu_ctx *c, int64_t *count, int reset)
{
    if (!c || !count) { set_error("snpgpu_diag_carry_fallbacks: invalid arguments"); return 1; }
    *count = 0;
    if (!c->uvcarry_flags.p) return 0;
    unsigned int n = 0;
    SNPGPU_HIP_CHECK(hipSetDevice(c->device));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(c->stream));
    SNPGPU_HIP_CHECK(hipMemcpy(&n, c->uvcarry_flags.p, sizeof(n), hipMemcpyDeviceToHost));
    if (reset) SNPGPU_HIP_CHECK(hipMemset(c->uvcarry_flags.p, 0, sizeof(n)));
    *count = (int64_t)n;
    return 0;
}

// kernel launches of the SYRK family (launch_syrk, launch_syrk_h3, launch_syrk_uv) since the context was created: host-side count of
// what was enqueued, whichever of two launches of a block the device flag lets work.  (snpgpu_get_timing counts timed SPANS: one
// per table and feed block, however many launches the block's fp32 runs take.)
extern "C" int snpgpu_diag_syrk_launches(snpgpu_ctx *c, int64_t *count)
{
    if (!c || !count) { set_error("snpgpu_diag_syrk_launches: invalid arguments"); return 1; }
    *count = c->syrk_launches;
    return 0;
}

// ---- snpgpu_diag_plan: names of the kernels a block takes under a plan (what launch_pair_i8 / launch_syrk_h3 / launch_syrk_uv run)
static const char *uv_form_kernel(UvForm f)
{
    return f == UvForm::Mfma32x32x16 ? "syrk_uv_kernel" : f == UvForm::Lookup16x16x32 ? "syrk_uv16_kernel" : "syrk_uv16c_kernel";
}
// the pair-counter kernel of a block with / without missing calls ("none": the block needs none)
static const char *plan_counter_kernel(const CtxPlan &p, bool missing)
{
    if (!p.use_pc) return "none";
    if (!p.pc_i8) return (p.pc_mode == PM_GCTA_MISS && !missing) ? "none" : "pair_popcount_kernel";
    if (p.pc_mode == PM_GCTA_MISS) return !missing ? "none" : p.miss_fp4 ? "pair_mfma_fp4_miss_kernel" : "pair_mfma_i8_kernel";
    if (!missing && p.want_het) return p.nomiss_fp4 ? "pair_mfma_fp4_nomiss_kernel" : "pair_mfma_i8_kernel";
    return p.general_fp4 ? "pair_mfma_fp4_kernel" : "pair_mfma_i8_kernel";
}
// the SYRK kernel of table 0 (KING-homo / dissimilarity: of the weight sums)
static const char *plan_syrk_kernel(const CtxPlan &p, bool missing)
{
    if (!p.use_mm) return "none";
    if (p.homo_uv) return missing ? uv_form_kernel(p.homo_form) : "none";
    const bool homo = p.lut_mode[0] == LUT_HOMO_W1;       // (with the two-product counter kernel: blocks with missing calls only)
    if (homo && p.want_het && !missing) return "none";
    if (!p.mm_h3) return "syrk_mfma_kernel";
    if (p.h3_a_kind[0] > 0) return "syrk_h3_kernel<2, false>";
    if (p.h3_a_kind[0] < 0) return "syrk_h3_kernel<3, false>";
    if (!missing && p.uv_enabled) return uv_form_kernel(p.uv_form);
    if (missing && !(p.h3_exact_missing || p.eigmix_x1)) return "syrk_h3_kernel<3, false>";
    return (p.want_x1_list && (missing || !p.uv_eigmix)) ? "syrk_x1_kernel" : "syrk_h3_kernel<2, true>";
}

// the plan of a context as text: every line "key=value", keys stable (tests/test_cpu_plan.py reads them)
extern "C" int snpgpu_diag_plan(int kind, int64_t n_samp, const snpgpu_opts *opts, int64_t block_snps, char *buf, int len)
{
    if (!buf || len <= 0) { set_error("snpgpu_diag_plan: no buffer"); return 1; }
    snpgpu_opts o{};
    if (opts) o = *opts;
    CtxPlan p;
    std::string why;
    if (plan_context(kind, n_samp, o, Switches::from_env(), &p, &why)) { set_error("snpgpu_create: " + why); return 1; }
    static const char *const pair_modes[] = {"ibs", "king_robust", "king_homo", "gcta_miss", "beta", "ibs_nomiss", "homo_nomiss", "diss"};
    static const char *const lut_modes[] = {"gcta", "bayes", "homo_w1", "homo_w2", "eigmix_num", "eigmix_missw"};
    static const char *const uv_forms[] = {"mfma32x32x16", "lookup16x16x32", "converted", "converted_carry"};
    static const char *const layouts[] = {"entry8or16", "entry16", "entry12", "entry12or8", "entry12missing"};
    std::ostringstream t;
    t << "kind=" << p.kind << "\nbayesian=" << p.bayesian << "\nn_samp=" << p.N << "\nrow0=" << p.row0 << "\nrow1=" << p.row1
      << "\ncol0=" << p.col0 << "\nrows_pad=" << p.rows_pad << "\nncols_pad=" << p.ncols_pad << "\nRB=" << p.RB << "\nBmax=" << p.Bmax
      << "\nKWmax=" << p.KWmax << "\nfull=" << p.full << "\nacc_tiles_c=" << p.acc_tiles_c << "\ntail_parts=" << p.tail_parts
      << "\ncounter_mode=" << (p.use_pc ? pair_modes[p.pc_mode] : "none") << "\nn_u32=" << p.n_u32
      << "\ncounter_backend=" << (!p.use_pc ? "none" : p.pc_i8 ? "mfma" : "popcount");
    if (p.use_pc && p.pc_i8)
        t << "\nnomiss_fp4=" << p.nomiss_fp4 << "\ngeneral_fp4=" << p.general_fp4 << "\nmiss_fp4=" << p.miss_fp4
          << "\ncounter_tile=" << p.pc_tile_r << "x" << p.pc_tile_c << "x" << p.pc_wg_per_cu << "\nwant_het=" << p.want_het
          << "\nnomiss_tile=" << p.nm_tile_r << "x" << p.nm_tile_c << "x" << p.nm_wg_per_cu << "\ngcta_sparse=" << p.gcta_sparse
          << "\nsp_max_rate=" << p.sp_max_rate;
    t << "\nn_lut=" << p.n_lut;
    for (int i = 0; i < p.n_lut; i++) t << "\nlut_mode" << i << "=" << lut_modes[p.lut_mode[i]] << "\nh3_a_kind" << i << "=" << p.h3_a_kind[i];
    if (p.use_mm)
        t << "\nsyrk_family=" << (p.mm_h3 ? "split_fp16" : "fp32") << "\nh3_super=" << p.h3_super << "\nx1_super=" << p.x1_super
          << "\nh3_exact_rows=" << p.h3_exact_rows << "\nh3_exact_missing=" << p.h3_exact_missing << "\nh3_w_shift=" << p.h3_w_shift
          << "\nh3_promote=" << p.h3_promote << "\nuv_promote=" << p.uv_promote << "\nwant_x1_list=" << p.want_x1_list
          << "\nuv_enabled=" << p.uv_enabled << "\nuv_eigmix=" << p.uv_eigmix << "\nuv_targets=" << p.uv_targets
          << "\nuv_form=" << uv_forms[(int)p.uv_form]  << "\nuvc_pace=" << p.uvc_pace << "\nuvc_carry_all=" << p.uvc_carry_all
          << "\nuvc_carry_slots=" << p.uvc_carry_slots << "\neigmix_x1=" << p.eigmix_x1
          << "\nsparse_missing=" << p.sparse_missing << "\nx1_short_runs=" << p.x1_short_runs << "\nx1_sparse_mac=" << p.x1_sparse_mac
          << "\nwt_layout=" << layouts[(int)p.wt_layout] << "\nwt_block_flag=" << p.wt_block_flag << "\nhomo_uv=" << p.homo_uv
          << "\nhomo_form=" << uv_forms[(int)p.homo_form] << "\nhomo_weights=" << p.homo_weights;
    t << "\ncounter_kernel_nomiss=" << plan_counter_kernel(p, false) << "\ncounter_kernel_missing=" << plan_counter_kernel(p, true)
      << "\nsyrk_kernel_nomiss=" << plan_syrk_kernel(p, false) << "\nsyrk_kernel_missing=" << plan_syrk_kernel(p, true);
    if (block_snps > 0 && p.use_mm) {
        const BlockRuns b = plan_block(p, block_snps);
        t << "\nblock_snps=" << block_snps << "\nuv_runs=" << b.uv_runs << "\nuv_cpr=" << b.uv_cpr << "\nuv_chunks=" << b.uv_chunks
          << "\nuv_q=" << b.uv_q << "\nn_pad=" << b.n_pad << "\nn_q=" << b.n_q;
    }
    t << "\n";
    const std::string s = t.str();
    if ((int64_t)s.size() + 1 > (int64_t)len) { set_error("snpgpu_diag_plan: buffer too small"); return 1; }
    memcpy(buf, s.c_str(), s.size() + 1);
    return 0;
}
