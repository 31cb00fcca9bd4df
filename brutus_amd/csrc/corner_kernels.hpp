// corner_kernels.hpp -- corner-plot marginals of a catalogue behind brutus_corner_hist1d /
// brutus_corner_hist2d (pdf.PosteriorCorner; reference plotting.py:361-501 and _hist2d,
// plotting.py:1456-1543).  Included by summary_unit.hip alone, after summary_kernels.hpp (the
// sample matrix, the sort) and smooth_taps.hpp (the Gaussian filter's weights and taps).
//
// k_corner_hist<WEIGHTED>: one workgroup per object and panel, laid out as k_summary_quantiles
// lays its object out (T = min(P, 1024) lanes, sample e = m T + t in slot m of lane t).  A sample
// gets its bin by comparison against the edges lo + k step (numpy.linspace: product and sum
// rounded apart, the last edge hi); the keys (bin << 12 | draw) are sorted with summary_sort, and
// the lane that holds the first key of a bin adds that bin's weights one by one, in draw order,
// starting from 0 -- numpy.bincount's order, so the bytes are numpy's.  The workgroup zeroes its
// panel first; no cell is written by two lanes after that.  LDS: 8 P bytes of keys and, WEIGHTED,
// 8 P of weights.
// k_corner_smooth<AXIS>: one axis of the filter on the float64 panels, a lane per cell.
// k_corner_levels: one workgroup per panel on its cells in descending order (a segmented radix
// sort): lane 0 adds them one by one from the largest, as numpy.cumsum does, a tile of LDS at a
// time, and stops at the first zero (what follows adds nothing); then every lane counts, for
// each level, the cells whose share is <= the level -- the share never decreases along the
// cells, so the count is the reference's `Hflat[sm <= v0][-1]` -- with integer atomics only.
// No scratch, no floating-point atomics; nothing depends on another object.
#pragma once

namespace {

constexpr int CORNER_DRAW_BITS = 12;                // 4096 draws
constexpr int CORNER_LEV_T = 256;
constexpr int CORNER_LEV_TILE = 2048;
constexpr int CORNER_MAX_LEVELS = BRUTUS_CORNER_MAX_LEVELS;

static_assert((1 << CORNER_DRAW_BITS) == BRUTUS_SUMMARY_MAX_DRAWS, "a key holds a draw in 12 bits");

__device__ __forceinline__ double corner_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

__device__ __forceinline__ bool corner_span_ok(double lo, double hi) {
    return lo < hi && lo > -INFINITY && hi < INFINITY;
}

// edge k of the n + 1 edges of [lo, hi], step = (hi - lo) / n: numpy.linspace
__device__ __forceinline__ double corner_edge(double lo, double hi, double step, int k, int n) {
#pragma clang fp contract(off)
    return k == n ? hi : lo + (double)k * step;
}

// the bin of v (numpy.histogram, numpy.histogramdd): the division only proposes, the edges
// decide; -1: outside [lo, hi] or NaN
__device__ __forceinline__ int corner_bin(double v, double lo, double hi, int n) {
#pragma clang fp contract(off)
    if (!(v >= lo && v <= hi)) return -1;
    const double step = (hi - lo) / (double)n;
    const double g = (v - lo) / (hi - lo) * (double)n;
    int b = g >= 0. ? (g < (double)(n - 1) ? (int)g : n - 1) : 0;
    while (b > 0 && v < corner_edge(lo, hi, step, b, n)) --b;
    while (b < n - 1 && v >= corner_edge(lo, hi, step, b + 1, n)) ++b;
    return b;
}

// coly < 0: a 1-D panel of column colx (nby = 1)
template <bool WEIGHTED>
__global__ void __launch_bounds__(SUMMARY_MAX_T)
k_corner_hist(int nsamps, int npad, const int32_t *__restrict__ idx, const double *__restrict__ dist,
              const double *__restrict__ red, const double *__restrict__ dred,
              const double *__restrict__ weights, int64_t nmodel, int nlab,
              const double *__restrict__ labels, int colx, int coly, int nbx, int nby,
              const double *__restrict__ spans, double *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char corner_lds[];
    uint64_t *xk = (uint64_t *)corner_lds;                   // (npad) exchange buffer, then sorted keys
    double *sw = (double *)(xk + npad);                      // (npad) WEIGHTED only: the weights by draw

    const int T = (int)blockDim.x, t = (int)threadIdx.x;
    const int E = npad / T;
    const int64_t row = (int64_t)blockIdx.x * nsamps;
    const int cells = nbx * nby;
    double *H = out + (int64_t)blockIdx.x * cells;
    const double *sp = spans + (int64_t)blockIdx.x * (nlab + 4) * 2;
    const double xlo = sp[2 * colx], xhi = sp[2 * colx + 1];
    const double ylo = coly >= 0 ? sp[2 * coly] : 0., yhi = coly >= 0 ? sp[2 * coly + 1] : 1.;
    if (!(corner_span_ok(xlo, xhi) && corner_span_ok(ylo, yhi))) {       // (uniform over the workgroup)
        for (int c = t; c < cells; c += T) H[c] = corner_nan();
        return;
    }
    for (int c = t; c < cells; c += T) H[c] = 0.;

    uint64_t key[SUMMARY_MAX_E];
    uint32_t pos[SUMMARY_MAX_E];
#pragma unroll
    for (int m = 0; m < SUMMARY_MAX_E; ++m) {
        const int e = m * T + t;
        key[m] = ~0ull;
        pos[m] = (uint32_t)e;
        if (m < E && e < nsamps) {
            const int32_t v = idx[row + e];
            const int32_t mi = v >= 0 && v < nmodel ? v : -1;
            int b = corner_bin(summary_sample(colx, nlab, mi, labels, dist, red, dred, row + e), xlo, xhi, nbx);
            if (coly >= 0 && b >= 0) {
                const int by = corner_bin(summary_sample(coly, nlab, mi, labels, dist, red, dred, row + e), ylo,
                                          yhi, nby);
                b = by >= 0 ? b * nby + by : -1;
            }
            if (b >= 0) key[m] = ((uint64_t)b << CORNER_DRAW_BITS) | (uint64_t)e;
            if (WEIGHTED) sw[e] = weights[row + e];
        }
    }
    summary_sort<false>(key, pos, npad, T, t, E, xk, (uint32_t *)nullptr);
#pragma unroll
    for (int m = 0; m < SUMMARY_MAX_E; ++m)
        if (m < E) xk[m * T + t] = key[m];
    __syncthreads();                         // the keys, the weights and the zeroed panel are in place

#pragma unroll
    for (int m = 0; m < SUMMARY_MAX_E; ++m) {
        const int e = m * T + t;
        if (m < E && key[m] != ~0ull) {
            const uint64_t bin = key[m] >> CORNER_DRAW_BITS;
            if (e == 0 || (xk[e - 1] >> CORNER_DRAW_BITS) != bin) {      // the first draw of its bin
                double s = 0.;
                for (int i = e; i < npad; ++i) {
                    const uint64_t ki = xk[i];
                    if ((ki >> CORNER_DRAW_BITS) != bin) break;
                    s += WEIGHTED ? sw[ki & ((1u << CORNER_DRAW_BITS) - 1)] : 1.;
                }
                H[bin] = s;
            }
        }
    }
}

// One axis of the filter on the (nx, ny) float64 panels of all objects: nblk = ceil(panel / 256)
// workgroups per object, objects along grid.x.
template <int AXIS>
__global__ void __launch_bounds__(BP_NT)
k_corner_smooth(int nx, int ny, int nblk, double sigma, const double *__restrict__ in, double *__restrict__ out) {
    __shared__ double w[BP_MAXR + 1];
    __shared__ double part[BP_NT / 64];
    const int plane = nx * ny;
    const int64_t o = blockIdx.x / (unsigned)nblk;
    const int blk = (int)(blockIdx.x - (unsigned)o * (unsigned)nblk);
    const double *src = in + o * plane;
    double *dst = out + o * plane;
    const int i = blk * BP_NT + (int)threadIdx.x;
    const int r = bp_gauss_weights(sigma, w, part);
    if (i >= plane) return;
    const int x = i / ny, y = i - x * ny;
    dst[i] = bp_taps<AXIS>(src, (int64_t)i, x, y, nx, ny, r, w);
}

// sorted (npanel, cells): every panel's cells in descending order; sm (npanel, cells): room for
// the cumulative sums; out (npanel, nlev).  A panel that holds a NaN (it sorts first) gets NaN levels.
__global__ void __launch_bounds__(CORNER_LEV_T)
k_corner_levels(int cells, const double *__restrict__ sorted, double *__restrict__ sm, int nlev,
                const double *__restrict__ levels, double *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double tile[CORNER_LEV_TILE];
    __shared__ double vals[CORNER_MAX_LEVELS];
    __shared__ double lev[CORNER_MAX_LEVELS];
    __shared__ double run;
    __shared__ int filled, cnt[CORNER_MAX_LEVELS];
    const double *src = sorted + (int64_t)blockIdx.x * cells;
    double *dst = sm + (int64_t)blockIdx.x * cells;
    const int t = (int)threadIdx.x;
    const double top = src[0];
    if (top != top) {                        // (uniform over the workgroup)
        if (t < nlev) out[(int64_t)blockIdx.x * nlev + t] = corner_nan();
        return;
    }
    if (t == 0) run = 0.;
    if (t < CORNER_MAX_LEVELS) {
        cnt[t] = 0;
        lev[t] = t < nlev ? levels[t] : 0.;
    }
    __syncthreads();

    // ---- the cumulative sum, sequential like numpy's, up to the first cell that is not > 0 ----
    int nscan = 0;
    for (int base = 0; base < cells; base += CORNER_LEV_TILE) {
        const int n = cells - base < CORNER_LEV_TILE ? cells - base : CORNER_LEV_TILE;
        for (int k = t; k < n; k += CORNER_LEV_T) tile[k] = src[base + k];
        __syncthreads();
        if (t == 0) {
            double s = run;
            int k = 0;
            for (; k + 8 <= n && tile[k + 7] > 0.; k += 8) {         // (descending: all eight are > 0)
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = tile[k + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    s += v[u];
                    tile[k + u] = s;
                }
            }
            for (; k < n && tile[k] > 0.; ++k) {
                s += tile[k];
                tile[k] = s;
            }
            run = s;
            filled = k;
        }
        __syncthreads();
        const int f = filled;
        for (int k = t; k < f; k += CORNER_LEV_T) dst[base + k] = tile[k];
        nscan = base + f;
        __syncthreads();                     // the tile is free again
        if (f < n) break;                    // (uniform)
    }

    // ---- per level: how many cells have a share <= the level (a lane re-reads its own stores) ----
    const double tot = run;
    int c[CORNER_MAX_LEVELS];
#pragma unroll
    for (int l = 0; l < CORNER_MAX_LEVELS; ++l) c[l] = 0;
    for (int base = 0; base < nscan; base += CORNER_LEV_TILE) {
        const int n = nscan - base < CORNER_LEV_TILE ? nscan - base : CORNER_LEV_TILE;
        for (int k = t; k < n; k += CORNER_LEV_T) {
            const double share = dst[base + k] / tot;
#pragma unroll
            for (int l = 0; l < CORNER_MAX_LEVELS; ++l) c[l] += share <= lev[l] ? 1 : 0;
        }
    }
    if (t == 0 && nscan < cells) {           // the zero cells: their share is tot / tot (0 / 0: none)
        const double share = tot / tot;
#pragma unroll
        for (int l = 0; l < CORNER_MAX_LEVELS; ++l) c[l] += share <= lev[l] ? cells - nscan : 0;
    }
#pragma unroll
    for (int l = 0; l < CORNER_MAX_LEVELS; ++l) {
        int v = c[l];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((t & 63) == 0 && l < nlev) atomicAdd(&cnt[l], v);
    }
    __syncthreads();
    if (t < nlev) vals[t] = cnt[t] > 0 ? src[cnt[t] - 1] : top;
    __syncthreads();
    if (t == 0) {                            // ascending, as the reference's V.sort()
        for (int a = 1; a < nlev; ++a) {
            const double v = vals[a];
            int b = a - 1;
            for (; b >= 0 && vals[b] > v; --b) vals[b + 1] = vals[b];
            vals[b + 1] = v;
        }
        for (int l = 0; l < nlev; ++l) out[(int64_t)blockIdx.x * nlev + l] = vals[l];
    }
}

}  // namespace
