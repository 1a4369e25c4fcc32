// C ABI of libsnpgpu (include/snpgpu.h): the error slot and the calls that need no context.  The streaming accumulator contexts of
// level (1) are in ctx_life.hip (create, destroy, timing), ctx_feed.hip, ctx_results.hip (finalisers) and ctx_select.hip.
#include <cmath>
#include <string>

#include "snpgpu_internal.h"

namespace snpgpu {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }

}  // namespace snpgpu

using namespace snpgpu;

extern "C" {

int snpgpu_abi_version(void) { return SNPGPU_ABI_VERSION; }
const char *snpgpu_last_error(void) { return g_err.c_str(); }

int snpgpu_device_count(int *count)
{
    int n = 0;
    SNPGPU_HIP_CHECK(hipGetDeviceCount(&n));
    if (count) *count = n;
    return 0;
}

int snpgpu_synth_block(void *dst, int64_t n_samp, int64_t snp_begin, int64_t n_snp, uint32_t seed, double missing,
                       int spectrum, int special, int device, void *stream)
{
    if (!dst || n_samp <= 0 || n_snp < 0 || snp_begin < 0 || !(missing >= 0.0 && missing < 1.0) || spectrum < 0 || spectrum > 4) {
        set_error("snpgpu_synth_block: invalid arguments");
        return 1;
    }
    SNPGPU_HIP_CHECK(hipSetDevice(device));
    const uint32_t miss32 = (uint32_t)std::floor(missing * 4294967296.0);
    // without a stream the block is written on the NULL stream, which does not order itself against the contexts' own
    // (non-blocking) streams: wait for whatever may still read `dst` (an earlier asynchronous snpgpu_feed of the same buffer)
    if (!stream) SNPGPU_HIP_CHECK(hipDeviceSynchronize());
    if (launch_synth_block((hipStream_t)stream, (uint8_t *)dst, n_samp, snp_begin, n_snp, seed, miss32, spectrum, special)) return 1;
    if (!stream) SNPGPU_HIP_CHECK(hipDeviceSynchronize());
    return 0;
}

int snpgpu_host_alloc(size_t bytes, void **out)
{
    if (!out) { set_error("snpgpu_host_alloc: out is NULL"); return 1; }
    SNPGPU_HIP_CHECK(hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocDefault));
    return 0;
}

int snpgpu_host_free(void *p)
{
    if (p) SNPGPU_HIP_CHECK(hipHostFree(p));
    return 0;
}

}  // extern "C"
