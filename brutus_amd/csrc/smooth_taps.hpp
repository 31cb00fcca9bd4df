// smooth_taps.hpp -- one axis of scipy.ndimage.gaussian_filter (order 0, mode `reflect`, truncate
// 4) as the kernels that smooth a plane share it: k_binpdf_smooth (binpdf_kernels.hpp, float32
// planes) and k_corner_smooth (corner_kernels.hpp, float64 panels).  The reflected index, the
// weights exp(-k^2 / (2 sigma^2)) / sum in float64 (LDS, made by the workgroup) and the symmetric
// sum of scipy's correlate1d, accumulated in float64 from the far taps inwards.  Every product is
// rounded before it is added (contraction off).
#pragma once

namespace {

constexpr int BP_NT = 256;
constexpr int BP_MAXR = 2047;                       // largest smoothing radius, in bins

__device__ __forceinline__ double bp_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// index j of a line of n values extended by `reflect`: (d c b a | a b c d | d c b a), repeated
__device__ __forceinline__ int bp_reflect(int j, int n) {
    if ((unsigned)j < (unsigned)n) return j;
    const int p = 2 * n;
    int m = j % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// The normalised weights w[0 .. r] of `sigma` (> 1e-15), r = int(4 sigma + 0.5) capped at BP_MAXR,
// made by the BP_NT lanes of the workgroup: w holds BP_MAXR + 1 doubles of LDS, part BP_NT / 64.
// Returns r; ends at a barrier.
__device__ __forceinline__ int bp_gauss_weights(double sigma, double *w, double *part) {
#pragma clang fp contract(off)
    const double r4 = 4. * sigma + 0.5;
    const int r = r4 < (double)BP_MAXR ? (int)r4 : BP_MAXR;
    const double a = -0.5 / (sigma * sigma);
    double s = 0.;
    for (int k = threadIdx.x; k <= r; k += BP_NT) {
        const double v = exp(a * (double)(k * k));
        w[k] = v;
        s += k ? v + v : v;
    }
    s = bp_wave_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    const double tot = (part[0] + part[1]) + (part[2] + part[3]);
    for (int k = threadIdx.x; k <= r; k += BP_NT) w[k] = w[k] / tot;
    __syncthreads();
    return r;
}

// The filtered value at (x, y) of the (nx, ny) plane `src`, element i = x ny + y, along AXIS.
template <int AXIS, class T>
__device__ __forceinline__ double bp_taps(const T *__restrict__ src, int64_t i, int x, int y, int nx, int ny,
                                          int r, const double *w) {
#pragma clang fp contract(off)
    double t = (double)src[i] * w[0];
    if (AXIS == 0) {
        const T *col = src + y;
        for (int k = r; k >= 1; --k)
            t += ((double)col[(int64_t)bp_reflect(x - k, nx) * ny] +
                  (double)col[(int64_t)bp_reflect(x + k, nx) * ny]) * w[k];
    } else {
        const T *row = src + (int64_t)x * ny;
        for (int k = r; k >= 1; --k)
            t += ((double)row[bp_reflect(y - k, ny)] + (double)row[bp_reflect(y + k, ny)]) * w[k];
    }
    return t;
}

}  // namespace
