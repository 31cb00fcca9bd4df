// summary_kernels.hpp -- per-object posterior summaries: weighted quantiles of every column of an
// object's sample matrix (reference plotting.py:249-322 with utils.py:718-762).  Included by
// summary_unit.hip alone.
//
// k_summary_quantiles<WEIGHTED>: one workgroup per object, objects along grid.x.  The workgroup has
// T = min(P, 1024) lanes, P = the draw count padded to a power of two (64 at the least), and lane
// t owns the samples e = m T + t, m < P / T <= 4, in registers for the whole object: their model
// indices are read once, then the columns are walked.  Per column (summary_column, which
// k_predictive_quantiles of predictive_kernels.hpp calls too):
//   - the sample becomes an order-preserving 64-bit key (NaNs made canonical first, so a NaN of
//     either sign sorts last; -0 becomes +0, numpy sorts them as equal; the padding is the
//     all-ones key, above every NaN);
//   - a bitonic sort of (key, position): compare-exchange passes with a partner closer than 64
//     stay inside the wave (shuffles), the others go through LDS -- every lane writes its own
//     8-byte slot and reads its partner's, consecutive lanes consecutive slots, which is free of
//     bank conflicts for ds_read_b64 (64 banks, 32-lane groups) and ds_write_b64 alike.  The
//     position breaks ties, so the order is numpy's stable argsort and does not depend on the
//     network; without weights the order of equal keys cannot matter and keys travel alone;
//   - WEIGHTED: the weight of every sorted sample is fetched by its position (the object's row,
//     at most 32 KiB, is cache-resident) and scanned inclusively: shuffles in the wave, wave
//     totals through LDS, summed in a fixed order;
//   - one lane per q searches the knots c_j = S_j / S_{n-1} (S_j = the first j sorted weights;
//     the last sorted weight is never used, the reference's rule) and interpolates as
//     numpy.interp does, in float64.  Without weights c_j = j / (n - 1), no scan.
// LDS: 8 P bytes (sorted samples; the exchange buffer during the sort) and, WEIGHTED, 8 P more
// (the scan; positions during the sort): sized by the draw count, 64 KiB at 4096 draws.  No
// scratch, no atomics; nothing depends on another object, so an object gives the same bytes in
// any batch.
#pragma once

namespace {

constexpr int SUMMARY_MAX_E = 4;          // samples per lane: 4096 draws over 1024 lanes
constexpr int SUMMARY_MAX_T = 1024;

__device__ __forceinline__ uint64_t summary_key(double x) {
    uint64_t u = (uint64_t)__double_as_longlong(x);
    if (x != x) u = 0x7ff8000000000000ull;
    if (x == 0.) u = 0;
    return u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
}

__device__ __forceinline__ double summary_unkey(uint64_t k) {
    return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull)));
}

// what the element at `e` keeps of itself and its partner at e ^ j in the pass (k, j)
template <bool WEIGHTED>
__device__ __forceinline__ void summary_keep(int e, int k, int j, uint64_t &key, uint32_t &pos, uint64_t okey,
                                             uint32_t opos) {
    const bool want_min = ((e & j) == 0) == ((e & k) == 0);
    const bool mine_less = WEIGHTED ? (key < okey || (key == okey && pos < opos)) : key < okey;
    if (mine_less != want_min) {
        key = okey;
        if (WEIGHTED) pos = opos;
    }
}

// c_j of the weighted form: S_j / S_{n-1}, S_0 = 0 (sinc: the inclusive scan)
__device__ __forceinline__ double summary_knot(const double *sinc, int j, double norm) {
    return j ? sinc[j - 1] / norm : 0.;
}

// The bitonic sort of (key, pos), ascending, as the head of this file has it: sample e = m T + t
// in slot m of lane t, npad samples in all; xk (npad) and, WEIGHTED, xp (npad) are the exchange
// buffers.  Every pass that touched LDS ends at a barrier.  Called by every lane of the workgroup
// (summary_column; k_corner_hist of corner_kernels.hpp sorts its bin keys with it).
template <bool WEIGHTED>
__device__ __forceinline__ void summary_sort(uint64_t (&key)[SUMMARY_MAX_E], uint32_t (&pos)[SUMMARY_MAX_E],
                                             int npad, int T, int t, int E, uint64_t *xk, uint32_t *xp) {
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j < 64) {
#pragma unroll
                for (int m = 0; m < SUMMARY_MAX_E; ++m)
                    if (m < E) {
                        const uint64_t ok = (uint64_t)__shfl_xor((unsigned long long)key[m], j);
                        const uint32_t op = WEIGHTED ? (uint32_t)__shfl_xor((int)pos[m], j) : 0u;
                        summary_keep<WEIGHTED>(m * T + t, k, j, key[m], pos[m], ok, op);
                    }
            } else {
#pragma unroll
                for (int m = 0; m < SUMMARY_MAX_E; ++m)
                    if (m < E) {
                        xk[m * T + t] = key[m];
                        if (WEIGHTED) xp[m * T + t] = pos[m];
                    }
                __syncthreads();
#pragma unroll
                for (int m = 0; m < SUMMARY_MAX_E; ++m)
                    if (m < E) {
                        const int e = m * T + t;
                        const uint64_t ok = xk[e ^ j];
                        const uint32_t op = WEIGHTED ? xp[e ^ j] : 0u;
                        summary_keep<WEIGHTED>(e, k, j, key[m], pos[m], ok, op);
                    }
                __syncthreads();
            }
        }
    }
}

// One column of one object, from the lanes' keys to its nq quantiles: `key` / `pos` hold the
// column (sample e = m T + t in slot m, the padding as the all-ones key), `wrow` the object's
// weights, `dst` the column's nq results.  Sort, scan, knot search, interpolation and store as
// the head of this file has them; ends at a barrier, after which xk / sinc are free again.
// Called by every lane of the workgroup (k_summary_quantiles, k_predictive_quantiles).
template <bool WEIGHTED>
__device__ __forceinline__ void summary_column(uint64_t (&key)[SUMMARY_MAX_E], uint32_t (&pos)[SUMMARY_MAX_E],
                                               int nsamps, int npad, int T, int t, int E, uint64_t *xk,
                                               double *sinc, uint32_t *xp, const double *__restrict__ wrow,
                                               int nq, const double *__restrict__ qs,
                                               double *__restrict__ dst) {
    summary_sort<WEIGHTED>(key, pos, npad, T, t, E, xk, xp);
#pragma unroll
    for (int m = 0; m < SUMMARY_MAX_E; ++m)
        if (m < E) xk[m * T + t] = key[m];

    // ---- WEIGHTED: inclusive scan of the sorted weights, in the order e = 0 .. npad - 1 ----
    if (WEIGHTED) {
        const int lane = t & 63, wv = t >> 6, nw = (T + 63) >> 6;
        double inc[SUMMARY_MAX_E];
#pragma unroll
        for (int m = 0; m < SUMMARY_MAX_E; ++m) {
            inc[m] = 0.;
            if (m < E) {
                double w = (m * T + t) < nsamps && pos[m] < (uint32_t)nsamps ? wrow[pos[m]] : 0.;
                for (int d = 1; d < 64; d <<= 1) {
                    const double up = __shfl_up(w, d);
                    if (lane >= d) w += up;
                }
                inc[m] = w;
            }
        }
        // (every pass of the sort that read xp ended at a barrier: its place is free)
#pragma unroll
        for (int m = 0; m < SUMMARY_MAX_E; ++m)
            if (m < E && lane == 63) sinc[m * nw + wv] = inc[m];
        __syncthreads();
        double before[SUMMARY_MAX_E];
#pragma unroll
        for (int m = 0; m < SUMMARY_MAX_E; ++m) {
            before[m] = 0.;
            if (m < E)
                for (int i = 0; i < m * nw + wv; ++i) before[m] += sinc[i];
        }
        __syncthreads();                     // the wave totals are read: their place is the scan's
#pragma unroll
        for (int m = 0; m < SUMMARY_MAX_E; ++m)
            if (m < E) sinc[m * T + t] = before[m] + inc[m];
    }
    __syncthreads();

    // ---- one lane per q: the knot search and the interpolation of numpy.interp ----
    if (t < nq) {
        const double q = qs[t];
        const int last = nsamps - 1;
        const double norm = WEIGHTED ? sinc[nsamps - 2] : (double)last;
        int j;
        if (WEIGHTED) {
            int lo = 0, hi = last;           // the rightmost knot <= q (c_0 = 0)
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (summary_knot(sinc, mid, norm) <= q)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            j = lo;
        } else {
            const double g = q * norm;
            j = g >= 0. ? (g < (double)last ? (int)g : last) : 0;
            while (j < last && (double)(j + 1) / norm <= q) ++j;
            while (j > 0 && (double)j / norm > q) --j;
        }
        double r;
        if (WEIGHTED && !(norm > 0.)) {
            r = __longlong_as_double(0x7ff8000000000000ll);
        } else if (j == last) {
            r = summary_unkey(xk[last]);
        } else {
            const double cj = WEIGHTED ? summary_knot(sinc, j, norm) : (double)j / norm;
            const double cn = WEIGHTED ? summary_knot(sinc, j + 1, norm) : (double)(j + 1) / norm;
            const double x0 = summary_unkey(xk[j]), x1 = summary_unkey(xk[j + 1]);
            if (cj == q) {
                r = x0;
            } else {
                const double slope = (x1 - x0) / (cn - cj);
                r = slope * (q - cj) + x0;
                if (r != r) {
                    r = slope * (q - cn) + x1;
                    if (r != r && x0 == x1) r = x0;
                }
            }
        }
        dst[t] = r;
    }
    __syncthreads();                         // the next column overwrites xk / sinc
}

// sample `i` (object row + draw) of column c: the labels of model `mi` (-1: outside the table,
// NaN) in table order, then Av, Rv, parallax = 1 / distance, distance
__device__ __forceinline__ double summary_sample(int c, int nlab, int32_t mi, const double *__restrict__ labels,
                                                 const double *__restrict__ dist, const double *__restrict__ red,
                                                 const double *__restrict__ dred, int64_t i) {
    if (c < nlab) return mi >= 0 ? labels[(int64_t)mi * nlab + c] : __longlong_as_double(0x7ff8000000000000ll);
    if (c == nlab) return red[i];
    if (c == nlab + 1) return dred[i];
    if (c == nlab + 2) return 1. / dist[i];
    return dist[i];
}

template <bool WEIGHTED>
__global__ void __launch_bounds__(SUMMARY_MAX_T)
k_summary_quantiles(int nsamps, int npad, const int32_t *__restrict__ idx, const double *__restrict__ dist,
                    const double *__restrict__ red, const double *__restrict__ dred,
                    const double *__restrict__ weights, int64_t nmodel, int nlab,
                    const double *__restrict__ labels, int nq, const double *__restrict__ qs,
                    double *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char summary_lds[];
    uint64_t *xk = (uint64_t *)summary_lds;                  // (npad) exchange buffer, then sorted keys
    double *sinc = (double *)(xk + npad);                    // (npad) WEIGHTED only: the scan ...
    uint32_t *xp = (uint32_t *)sinc;                         // ... and, during the sort, positions

    const int T = (int)blockDim.x, t = (int)threadIdx.x;
    const int E = npad / T;
    const int64_t row = (int64_t)blockIdx.x * nsamps;
    const int ncol = nlab + 4;

    int32_t mi[SUMMARY_MAX_E];                               // model index, -1: outside the table
#pragma unroll
    for (int m = 0; m < SUMMARY_MAX_E; ++m) {
        const int e = m * T + t;
        mi[m] = -1;
        if (m < E && e < nsamps) {
            const int32_t v = idx[row + e];
            if (v >= 0 && v < nmodel) mi[m] = v;
        }
    }

    for (int c = 0; c < ncol; ++c) {
        uint64_t key[SUMMARY_MAX_E];
        uint32_t pos[SUMMARY_MAX_E];
#pragma unroll
        for (int m = 0; m < SUMMARY_MAX_E; ++m) {
            const int e = m * T + t;
            key[m] = ~0ull;
            pos[m] = (uint32_t)e;
            if (m < E && e < nsamps) {
                const double x = summary_sample(c, nlab, mi[m], labels, dist, red, dred, row + e);
                key[m] = summary_key(x);
            }
        }

        summary_column<WEIGHTED>(key, pos, nsamps, npad, T, t, E, xk, sinc, xp,
                                 WEIGHTED ? weights + row : nullptr, nq, qs,
                                 out + ((int64_t)blockIdx.x * ncol + c) * nq);
    }
}

}  // namespace
