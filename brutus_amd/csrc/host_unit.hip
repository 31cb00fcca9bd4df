// host_unit.hip -- translation unit of libbrutus_amd.so: the host state every unit shares (the
// error string, the kernel-timing switch and its last result; declared in host.hpp) with the
// entry points that read it, and the measurement aids that belong to no subsystem
// (calib_kernels.hpp).

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/brutus_amd.h"
#include "../../include/brutus_amd_debug.h"

#include "host.hpp"
#include "common.hpp"
#include "fastmath.hpp"
#include "calib_kernels.hpp"

thread_local std::string g_err;
bool g_timing = false;
thread_local std::vector<TimingEntry> g_last_timing;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" {

int brutus_abi_version(void) { return BRUTUS_ABI_VERSION; }
const char *brutus_last_error(void) { return g_err.c_str(); }

void brutus_enable_timing(int on) { g_timing = on != 0; }

int brutus_last_timing(int *n_entries, const char **names, float *ms, int max_entries) {
    int n = 0;
    for (auto &t : g_last_timing) {
        if (n >= max_entries) break;
        names[n] = t.name.c_str();
        ms[n] = t.ms;
        ++n;
    }
    if (n_entries) *n_entries = n;
    return 0;
}

int brutus_calibrate_traffic(const float *d_in, double *d_out, int64_t n, void *stream) {
    if (!d_in || !d_out || n <= 0) return fail(BRUTUS_EINVAL, "bad calibration arguments");
    hipLaunchKernelGGL(k_calib_stream, dim3(4096), dim3(TILE), 0, (hipStream_t)stream, d_in, d_out, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brutus_calibrate_copy16(const void *d_in, void *d_out, int64_t nbytes, void *stream) {
    if (!d_in || !d_out || nbytes < 16 || (nbytes & 15)) return fail(BRUTUS_EINVAL, "bad calibration arguments");
    const int64_t n = nbytes / 16;
    if ((n + TILE - 1) / TILE > 0x7fffffff) return fail(BRUTUS_EINVAL, "calibration buffer too large");
    hipLaunchKernelGGL(k_calib_copy16, dim3((unsigned)((n + TILE - 1) / TILE)), dim3(TILE), 0,
                       (hipStream_t)stream, (const calib_f4 *)d_in, (calib_f4 *)d_out, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brutus_calibrate_issue(int kind, int iters, int waves_per_simd, float *d_scratch,
                           int64_t scratch_floats, void *stream) {
    if (kind < 0 || kind > 2 || iters <= 0 || waves_per_simd < 1 || waves_per_simd > 8 || !d_scratch)
        return fail(BRUTUS_EINVAL, "bad calibration arguments");
    int dev = 0, ncu = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    const int blocks = ncu * waves_per_simd;       // 256 threads = one wave on each of a CU's four SIMDs
    if (scratch_floats < (int64_t)blocks * 256) return fail(BRUTUS_EINVAL, "calibration scratch too small");
    hipStream_t st = (hipStream_t)stream;
    if (kind == 0) hipLaunchKernelGGL(k_calib_issue<0>, dim3(blocks), dim3(256), 0, st, d_scratch, iters);
    else if (kind == 1) hipLaunchKernelGGL(k_calib_issue<1>, dim3(blocks), dim3(256), 0, st, d_scratch, iters);
    else hipLaunchKernelGGL(k_calib_issue<2>, dim3(blocks), dim3(256), 0, st, d_scratch, iters);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brutus_debug_exp10(const double *d_x, double *d_y, int64_t n, void *stream) {
    if (!d_x || !d_y || n <= 0) return fail(BRUTUS_EINVAL, "bad arguments");
    hipLaunchKernelGGL(k_debug_exp10, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, d_x, d_y, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brutus_debug_math(int which, const double *d_x, double *d_y, int64_t n, void *stream) {
    if (!d_x || !d_y || n <= 0 || which < 0 || which > 10) return fail(BRUTUS_EINVAL, "bad arguments");
    if (which == 10 && n % 64 != 0) return fail(BRUTUS_EINVAL, "wave maximum: n must be a multiple of 64");
    hipLaunchKernelGGL(k_debug_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, which, d_x, d_y, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
