// calib_kernels.hpp -- measurement aids that belong to no subsystem: PMC calibration streams,
// the vector unit's issue rate, and the fastmath.hpp functions evaluated elementwise for the
// tests.  Included by host_unit.hip only; needs common.hpp (TILE) and fastmath.hpp.
#pragma once

#include "common.hpp"
#include "fastmath.hpp"

namespace {

// PMC calibration stream with the fused scan's access widths: 4-byte loads and
// 8-byte stores per lane, a known byte count (see tools/pmc_traffic.py).
__global__ void k_calib_stream(const float *__restrict__ in, double *__restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (double)in[i];
}

// the guide's reference stream: 16 B per lane in, 16 B per lane out.  One element per lane,
// workgroups in address order, non-temporal accesses: the shape that reaches the guide's
// 6.3 TB/s on this pool (profiles/r04_stream_sweep.txt: 6.1 - 6.5 TB/s; the grid-stride loop
// over 8 192 workgroups that rounds 1-3 measured with reaches 4.5 - 5.0 with the same bytes).
typedef float calib_f4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(TILE)
k_calib_copy16(const calib_f4 *__restrict__ in, calib_f4 *__restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * TILE + threadIdx.x;
    if (i < n) __builtin_nontemporal_store(__builtin_nontemporal_load(in + i), out + i);
}

// Measurement aid: the vector unit's issue rate, by kind of instruction.  Every lane runs
// `iters` rounds of 128 independent-enough operations of one kind (8 accumulators), so a launch
// of w x 256 workgroups of 256 threads puts w waves on every SIMD that issue nothing else:
//   kind 0  v_fmac_f32      1  v_fmac_f64      2  v_exp_f32 (transcendental)
// (the same loops as tools/ubench/dpp_rate.hip, which also has the DPP and packed forms).
#define CALIB_REP16(x) x x x x x x x x x x x x x x x x
template <int KIND>
__global__ void __launch_bounds__(256)
k_calib_issue(float *__restrict__ out, int iters) {
    float a0 = threadIdx.x, a1 = 1.f, a2 = 2.f, a3 = 3.f, a4 = 4.f, a5 = 5.f, a6 = 6.f, a7 = 7.f;
    const float r = threadIdx.x * 0.5f, x = 1.0001f;
    double d0 = a0, d1 = a1, d2 = a2, d3 = a3;
    const double dr = r, dx = x;
    for (int i = 0; i < iters; ++i) {
        if constexpr (KIND == 0) {
            CALIB_REP16(asm volatile(
                "v_fmac_f32_e32 %0, %8, %9\n v_fmac_f32_e32 %1, %8, %9\n v_fmac_f32_e32 %2, %8, %9\n"
                "v_fmac_f32_e32 %3, %8, %9\n v_fmac_f32_e32 %4, %8, %9\n v_fmac_f32_e32 %5, %8, %9\n"
                "v_fmac_f32_e32 %6, %8, %9\n v_fmac_f32_e32 %7, %8, %9\n"
                : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                : "v"(r), "v"(x));)
        } else if constexpr (KIND == 1) {
            CALIB_REP16(asm volatile(
                "v_fmac_f64_e32 %0, %4, %5\n v_fmac_f64_e32 %1, %4, %5\n v_fmac_f64_e32 %2, %4, %5\n"
                "v_fmac_f64_e32 %3, %4, %5\n v_fmac_f64_e32 %0, %4, %5\n v_fmac_f64_e32 %1, %4, %5\n"
                "v_fmac_f64_e32 %2, %4, %5\n v_fmac_f64_e32 %3, %4, %5\n"
                : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3) : "v"(dr), "v"(dx));)
        } else {
            CALIB_REP16(asm volatile(
                "v_exp_f32_e32 %0, %0\n v_exp_f32_e32 %1, %1\n v_exp_f32_e32 %2, %2\n v_exp_f32_e32 %3, %3\n"
                "v_exp_f32_e32 %4, %4\n v_exp_f32_e32 %5, %5\n v_exp_f32_e32 %6, %6\n v_exp_f32_e32 %7, %7\n"
                : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));)
        }
    }
    out[(int64_t)blockIdx.x * blockDim.x + threadIdx.x] =
        a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + (float)(d0 + d1 + d2 + d3);
}
#undef CALIB_REP16

__global__ void k_debug_exp10(const double *__restrict__ x, double *__restrict__ y, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = fast_exp10(x[i]);
}
__global__ void k_debug_math(int which, const double *__restrict__ x, double *__restrict__ y,
                             int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    double sq, rsq;
    if (which == 10) {      // (n is a multiple of 64: whole waves come here)
        y[i] = wave_max_dpp(v);
        return;
    }
    switch (which) {
    case 1: y[i] = fast_exp(v); break;
    case 2: y[i] = fast_log(v); break;
    case 3: y[i] = fast_sqrt(v); break;
    case 4: fast_sqrt_rsqrt(v, sq, rsq); y[i] = rsq; break;
    case 5: y[i] = fast_rcp(v); break;
    case 6: y[i] = fast_exp_fin(v, kExp2Tbl); break;
    case 7: y[i] = fast_log_pos(v); break;
    case 8: y[i] = fast_log_r(v); break;
    case 9: y[i] = fast_exp_bf(v, kExp2Tbl); break;
    default: y[i] = fast_exp10(v);
    }
}

}  // namespace
