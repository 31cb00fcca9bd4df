// offdiag_kernels.hpp -- photometric-offset residual maps: the computing half of reference
// plotting.photometric_offsets (plotting.py:1073-1134) and photometric_offsets_2d
// (plotting.py:1297-1363).  Included by summary_unit.hip alone, after predictive_kernels.hpp,
// whose predictive_value<false> and predictive_row form every predicted magnitude here.
//
//   k_od_residuals       one workgroup per object, the draws strided over the lanes.  A lane
//                        gathers its draw's grid row once (12 Nfilt contiguous bytes, see the head
//                        of predictive_kernels.hpp), forms every band's magnitude, stores
//                        dm = mpred - magobs and keeps the chi-square terms of the masked bands in
//                        its own LDS column (an array indexed by band, out of the registers).  For
//                        each band the object is used in it sums the OTHER bands' terms in band
//                        order (never total minus one term: that cancels) and parks ln L in the
//                        wt array; then, per band, a workgroup max and three sums over the draws,
//                        every one a fixed tree, give logsumexp, the normalised weights and their
//                        sum.  lgamma and the Gaussian normaliser are formed once per workgroup.
//   k_od_pool, k_od_bin, k_od_cell_keys, k_od_cell_of, k_od_cell_gather
//                        lane = pooled sample: what the sorts of summary_unit.hip take and give.
//   k_od_bin_sums        one wave per bin: the run of the bin in the sorted keys, summed by lane
//                        stride and a fixed shuffle tree.
//   k_od_run_quantiles   one workgroup per run of sorted (value, weight) pairs: utils.quantile's
//                        rule over a run of ANY length, walked twice in tiles of
//                        OD_RUN_T * OD_RUN_E samples with a carried prefix (the first walk finds
//                        the normaliser, the second the knots).  The pooled quantiles of a band
//                        are one run, the cell medians one run per cell.
// No atomics anywhere: a sum is a fixed tree over a fixed order, so every byte repeats.  Nothing
// in k_od_residuals depends on another object.
#pragma once

namespace {

constexpr int OD_POOL_T = 256;
constexpr int OD_RUN_T = 512, OD_RUN_E = 8;
constexpr int OD_MAX_Q = BRUTUS_OFFDIAG_MAX_Q;
constexpr int OD_BINS_PER_BLOCK = 4;      // k_od_bin_sums: 4 waves

__device__ __forceinline__ double od_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
// a sort key: one NaN (positive, so it sorts last), -0 as +0 (numpy sorts them as equal)
__device__ __forceinline__ double od_canon(double x) { return x != x ? od_nan() : x + 0.; }

// max or sum of `v` over the workgroup (T a power of two), a fixed tree; all lanes get it
template <bool MAX>
__device__ __forceinline__ double od_reduce(double v, double *buf, int t, int T) {
    buf[t] = v;
    __syncthreads();
    for (int s = T >> 1; s > 0; s >>= 1) {
        if (t < s) buf[t] = MAX ? fmax(buf[t], buf[t + s]) : buf[t] + buf[t + s];
        __syncthreads();
    }
    const double r = buf[0];
    __syncthreads();
    return r;
}

// LDS of k_od_residuals for `T` lanes and `nfilt` bands
inline size_t od_residuals_lds(int T, int nfilt) {
    return sizeof(double) * ((size_t)nfilt * T + T + 5 * (size_t)nfilt) + sizeof(int) * 2 * (size_t)nfilt;
}

__global__ void __launch_bounds__(256)
k_od_residuals(int64_t nobj, int nsamps, const int32_t *__restrict__ idx, const double *__restrict__ dist,
               const double *__restrict__ red, const double *__restrict__ dred,
               const double *__restrict__ weights, int64_t nmodel, int nfilt, const float *__restrict__ models,
               const double *__restrict__ magobs, const double *__restrict__ mageobs,
               const uint8_t *__restrict__ mask, int dim_prior, double *__restrict__ dm, double *__restrict__ wt,
               uint8_t *__restrict__ use) {
    // (every product and quotient rounded on its own, as numpy rounds it)
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char od_lds[];
    const int T = (int)blockDim.x, t = (int)threadIdx.x;
    double *term = (double *)od_lds;          // (nfilt, T): lane t owns column t
    double *buf = term + (size_t)nfilt * T;   // (T) reductions
    double *mo = buf + T;                     // (nfilt) magobs, mageobs^2, the two constants of ln L, a - 1
    double *var = mo + nfilt;
    double *c1 = var + nfilt;
    double *c2 = c1 + nfilt;
    double *am1 = c2 + nfilt;
    int *msk = (int *)(am1 + nfilt);          // (nfilt) masked in; used in this band
    int *usef = msk + nfilt;

    const int64_t o = blockIdx.x, row = o * nsamps;
    int bad = 0;
    if (t < nfilt) {
        const double m = magobs[o * nfilt + t], e = mageobs[o * nfilt + t];
        mo[t] = m;
        var[t] = e * e;
        msk[t] = mask[o * nfilt + t] != 0;
        if (!(fabs(m) <= 1.7976931348623157e308)) bad = 1;
    }
    for (int e = t; e < nsamps; e += T) {
        const int32_t v = idx[row + e];
        if (v < 0 || v >= nmodel) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (t < nfilt) {
        int n = 0;
        double slv = 0.;
        for (int b = 0; b < nfilt; ++b)
            if (b != t && msk[b]) {
                ++n;
                slv += log(var[b]);
            }
        usef[t] = !bad && msk[t] && n > 3;
        const double a = 0.5 * (double)(n - 3);
        am1[t] = a - 1.;
        if (dim_prior) {
            c1[t] = n > 3 ? lgamma(a) : 0.;
            c2[t] = log(2.) * a;
        } else {
            c1[t] = 0.5 * ((double)n * log(2. * 3.141592653589793) + slv);
            c2[t] = 0.;
        }
    }
    __syncthreads();

    // ---- per draw: the residuals, and ln L of every band the object is used in ----
    for (int e = t; e < nsamps; e += T) {
        const float *grow = predictive_row(models, idx[row + e], nmodel, nfilt);
        const double av = red[row + e], rv = dred[row + e], d = dist[row + e];
        for (int b = 0; b < nfilt; ++b) {
            const double v = predictive_value<false>(grow, b, av, rv, d);
            const double r = mo[b] - v;
            term[b * T + t] = msk[b] ? r * r / var[b] : 0.;
            dm[((int64_t)b * nobj + o) * nsamps + e] = usef[b] ? v - mo[b] : od_nan();
        }
        for (int i = 0; i < nfilt; ++i) {
            double lnl = 0.;
            if (usef[i]) {
                double chi2 = 0.;
                for (int b = 0; b < nfilt; ++b)
                    if (b != i && msk[b]) chi2 += term[b * T + t];
                if (dim_prior) {
                    const double xl = am1[i] == 0. ? 0. : am1[i] * log(chi2);
                    lnl = xl - chi2 / 2. - c1[i] - c2[i];
                } else {
                    lnl = -0.5 * chi2 - c1[i];
                }
            }
            wt[((int64_t)i * nobj + o) * nsamps + e] = lnl;
        }
    }

    // ---- per band: logsumexp over the draws, the normalised weights, their sum ----
    // (a lane reads back only what it stored itself)
    for (int i = 0; i < nfilt; ++i) {
        if (!usef[i]) {                       // uniform over the workgroup
            if (t == 0) use[(int64_t)i * nobj + o] = 0;
            continue;
        }
        double *w_i = wt + ((int64_t)i * nobj + o) * nsamps;
        double *dm_i = dm + ((int64_t)i * nobj + o) * nsamps;
        double v = -__builtin_huge_val();
        for (int e = t; e < nsamps; e += T) v = fmax(v, w_i[e]);
        const double mx = od_reduce<true>(v, buf, t, T);
        v = 0.;
        for (int e = t; e < nsamps; e += T) v += exp(w_i[e] - mx);
        const double levid = mx + log(od_reduce<false>(v, buf, t, T));
        v = 0.;
        for (int e = t; e < nsamps; e += T) v += exp(w_i[e] - levid);
        const double esum = od_reduce<false>(v, buf, t, T);
        v = 0.;
        for (int e = t; e < nsamps; e += T) {
            const double w = (weights ? weights[row + e] : 1.) * (exp(w_i[e] - levid) / esum);
            w_i[e] = w;
            v += w;
        }
        const double wsum = od_reduce<false>(v, buf, t, T);
        const bool ok = fabs(levid) <= 1.7976931348623157e308 && wsum > 0. && wsum <= 1.7976931348623157e308;
        if (!ok)
            for (int e = t; e < nsamps; e += T) {
                w_i[e] = 0.;
                dm_i[e] = od_nan();
            }
        if (t == 0) use[(int64_t)i * nobj + o] = ok;
    }
}

// The source of pooled sample j: object `o` (d_objs[j / nsamps], or j / nsamps) and the offset
// o nsamps + j % nsamps into an (nobj, nsamps) array; -1 for an object outside [0, nobj).
__device__ __forceinline__ int64_t od_src(int64_t j, int nsamps, const int32_t *__restrict__ objs, int64_t nobj,
                                          int64_t &o) {
    const int64_t u = j / nsamps;
    o = objs ? (int64_t)objs[u] : u;
    return o >= 0 && o < nobj ? o * nsamps + (j - u * nsamps) : -1;
}

__global__ void __launch_bounds__(OD_POOL_T)
k_od_pool(int64_t n, int nsamps, const int32_t *__restrict__ objs, int64_t nobj, const double *__restrict__ val,
          int per_sample, const double *__restrict__ wt, double *__restrict__ keys, double *__restrict__ w) {
    const int64_t j = (int64_t)blockIdx.x * OD_POOL_T + threadIdx.x;
    if (j >= n) return;
    int64_t o;
    const int64_t src = od_src(j, nsamps, objs, nobj, o);
    keys[j] = src < 0 ? od_nan() : od_canon(per_sample ? val[src] : val[o]);
    w[j] = src < 0 ? 0. : wt[src];
}

// numpy.histogramdd's bin of `v` in the nb + 1 ascending `edges`: searchsorted(side="right"), the
// last edge inclusive; -1 outside and for NaN
__device__ __forceinline__ int od_bin(const double *edges, int nb, double v) {
    int lo = 0, hi = nb + 1;                  // the number of edges <= v
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] <= v)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (v == edges[nb]) lo -= 1;
    return lo >= 1 && lo <= nb ? lo - 1 : -1;
}

__global__ void __launch_bounds__(OD_POOL_T)
k_od_bin(int64_t n, int nsamps, const int32_t *__restrict__ objs, int64_t nobj, const double *__restrict__ x,
         int x_per_sample, const double *__restrict__ dm, const double *__restrict__ wt, int nx, int ny,
         const double *__restrict__ xedges, const double *__restrict__ yedges, uint32_t *__restrict__ keys,
         double *__restrict__ w) {
    extern __shared__ __align__(16) unsigned char od_lds[];
    double *ex = (double *)od_lds, *ey = ex + nx + 1;
    for (int i = threadIdx.x; i <= nx; i += OD_POOL_T) ex[i] = xedges[i];
    for (int i = threadIdx.x; i <= ny; i += OD_POOL_T) ey[i] = yedges[i];
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * OD_POOL_T + threadIdx.x;
    if (j >= n) return;
    int64_t o;
    const int64_t src = od_src(j, nsamps, objs, nobj, o);
    uint32_t key = (uint32_t)(nx * ny);       // dropped: sorts behind every bin
    double wv = 0.;
    if (src >= 0) {
        const int cx = od_bin(ex, nx, x_per_sample ? x[src] : x[o]);
        const int cy = od_bin(ey, ny, dm[src]);
        if (cx >= 0 && cy >= 0) key = (uint32_t)(cx * ny + cy);
        wv = wt[src];
    }
    keys[j] = key;
    w[j] = wv;
}

// the first j in [0, n) with keys[j] >= k (n: none)
__device__ __forceinline__ int64_t od_lower(const uint32_t *__restrict__ keys, int64_t n, uint32_t k) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(64 * OD_BINS_PER_BLOCK)
k_od_bin_sums(int64_t n, const uint32_t *__restrict__ keys, const double *__restrict__ w, int nbins,
              double *__restrict__ H) {
    const int lane = threadIdx.x & 63;
    const int bin = blockIdx.x * OD_BINS_PER_BLOCK + (threadIdx.x >> 6);
    if (bin >= nbins) return;                 // a whole wave
    const int64_t a = od_lower(keys, n, (uint32_t)bin), b = od_lower(keys, n, (uint32_t)bin + 1u);
    double s = 0.;
    for (int64_t j = a + lane; j < b; j += 64) s += w[j];
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d);
    if (lane == 0) H[bin] = s;
}

__global__ void __launch_bounds__(OD_POOL_T)
k_od_cell_keys(int64_t n, int nsamps, const int32_t *__restrict__ objs, int64_t nobj,
               const double *__restrict__ dm, double *__restrict__ keys, uint32_t *__restrict__ src_out) {
    const int64_t j = (int64_t)blockIdx.x * OD_POOL_T + threadIdx.x;
    if (j >= n) return;
    int64_t o;
    const int64_t src = od_src(j, nsamps, objs, nobj, o);
    keys[j] = src < 0 ? od_nan() : od_canon(dm[src]);
    src_out[j] = src < 0 ? 0xffffffffu : (uint32_t)src;      // (src < 2^27)
}

__global__ void __launch_bounds__(OD_POOL_T)
k_od_cell_of(int64_t n, int nsamps, int64_t nobj, const uint32_t *__restrict__ src, const int32_t *__restrict__ cell,
             int ncell, uint32_t *__restrict__ keys) {
    const int64_t j = (int64_t)blockIdx.x * OD_POOL_T + threadIdx.x;
    if (j >= n) return;
    uint32_t key = (uint32_t)ncell;           // no cell: sorts behind every cell
    if (src[j] != 0xffffffffu) {
        const int32_t c = cell[src[j] / (uint32_t)nsamps];
        if (c >= 0 && c < ncell) key = (uint32_t)c;
    }
    keys[j] = key;
}

__global__ void __launch_bounds__(OD_POOL_T)
k_od_cell_gather(int64_t n, const uint32_t *__restrict__ src, const double *__restrict__ dm,
                 const double *__restrict__ wt, double *__restrict__ xs, double *__restrict__ ws) {
    const int64_t j = (int64_t)blockIdx.x * OD_POOL_T + threadIdx.x;
    if (j >= n) return;
    const uint32_t s = src[j];
    xs[j] = s == 0xffffffffu ? od_nan() : dm[s];
    ws[j] = s == 0xffffffffu ? 0. : wt[s];
}

// One walk over the run [a, b) of the weights `ws`: f(j, s, sn) for every sample j with
// s = S_j, the sum of the run's weights in front of j, and sn = S_{j+1} AS THE OWNER OF j + 1
// FORMS IT (so a knot has one value wherever it is used).  Lane t owns OD_RUN_E consecutive
// samples of a tile; S_j = (carry + the lanes in front, a Hillis-Steele scan) + the lane's own
// samples in front, each a fixed order.  Called by every lane; `sc` (OD_RUN_T) and `first`
// (OD_RUN_T + 1) are LDS.
template <class F>
__device__ __forceinline__ void od_walk(const double *__restrict__ ws, int64_t a, int64_t b, double *sc,
                                        double *first, int t, F &&f) {
    double carry = 0.;
    for (int64_t tile = a; tile < b; tile += OD_RUN_T * OD_RUN_E) {
        const int64_t base = tile + (int64_t)t * OD_RUN_E;
        double w[OD_RUN_E], part = 0.;
#pragma unroll
        for (int i = 0; i < OD_RUN_E; ++i) {
            w[i] = base + i < b ? ws[base + i] : 0.;
            part += w[i];
        }
        sc[t] = part;
        __syncthreads();
        for (int d = 1; d < OD_RUN_T; d <<= 1) {
            const double v = t >= d ? sc[t - d] : 0.;
            __syncthreads();
            sc[t] += v;
            __syncthreads();
        }
        double s = carry + (t ? sc[t - 1] : 0.);
        const double next_carry = carry + sc[OD_RUN_T - 1];
        first[t] = s;
        if (t == 0) first[OD_RUN_T] = next_carry;
        __syncthreads();
        const double nxt = first[t + 1];
#pragma unroll
        for (int i = 0; i < OD_RUN_E; ++i)
            if (base + i < b) {
                const double sn = i + 1 < OD_RUN_E ? s + w[i] : nxt;
                f(base + i, s, sn);
                s = sn;
            }
        carry = next_carry;
        __syncthreads();                      // sc and first are rewritten by the next tile
    }
}

// `runkeys` NULL: one run, all n samples, one workgroup.  Otherwise workgroup r takes the run of
// key r in the ascending `runkeys`; count[r] = its length / nsamps, and a count of 0 or below
// min_count gives NaN.  out: (runs, nq); `qs` NULL: the median.
__global__ void __launch_bounds__(OD_RUN_T)
k_od_run_quantiles(int64_t n, const double *__restrict__ xs, const double *__restrict__ ws,
                   const uint32_t *__restrict__ runkeys, int nsamps, int min_count, int nq,
                   const double *__restrict__ qs, double *__restrict__ out, int32_t *__restrict__ count) {
#pragma clang fp contract(off)
    __shared__ double sc[OD_RUN_T];
    __shared__ double first[OD_RUN_T + 1];
    __shared__ long long best[OD_RUN_T];
    __shared__ double s_norm;
    __shared__ long long s_ab[2];
    const int t = (int)threadIdx.x;
    const int64_t r = blockIdx.x;
    if (t == 0) {
        s_ab[0] = runkeys ? od_lower(runkeys, n, (uint32_t)r) : 0;
        s_ab[1] = runkeys ? od_lower(runkeys, n, (uint32_t)r + 1u) : n;
        s_norm = od_nan();
    }
    __syncthreads();
    const int64_t a = s_ab[0], b = s_ab[1], len = b - a;
    const int64_t cnt = len / nsamps;
    if (count && t == 0) count[r] = (int32_t)cnt;
    if (len < 2 || cnt < 1 || cnt < min_count) {             // uniform over the workgroup
        if (t < nq) out[r * nq + t] = od_nan();
        return;
    }

    // the normaliser S_{n-1}: the weights in front of the last sorted sample
    od_walk(ws, a, b, sc, first, t, [&](int64_t j, double s, double) {
        if (j == b - 1) s_norm = s;
    });
    __syncthreads();
    const double norm = s_norm;

    // the rightmost knot c_j = S_j / norm <= q, per q (c_a = 0)
    double q[OD_MAX_Q], bs[OD_MAX_Q], bn[OD_MAX_Q];
    long long bj[OD_MAX_Q];
#pragma unroll
    for (int k = 0; k < OD_MAX_Q; ++k) {
        q[k] = k < nq ? (qs ? qs[k] : 0.5) : 0.;
        bj[k] = -1;
        bs[k] = bn[k] = 0.;
    }
    od_walk(ws, a, b, sc, first, t, [&](int64_t j, double s, double sn) {
        const double c = s / norm;
#pragma unroll
        for (int k = 0; k < OD_MAX_Q; ++k)
            if (k < nq && c <= q[k]) {
                bj[k] = j;
                bs[k] = s;
                bn[k] = sn;
            }
    });
#pragma unroll
    for (int k = 0; k < OD_MAX_Q; ++k) {
        if (k >= nq) break;
        best[t] = bj[k];
        __syncthreads();
        for (int s = OD_RUN_T >> 1; s > 0; s >>= 1) {
            if (t < s && best[t + s] > best[t]) best[t] = best[t + s];
            __syncthreads();
        }
        const long long j = best[0];
        __syncthreads();
        if (j < 0 || !(norm > 0.)) {
            if (t == 0) out[r * nq + k] = od_nan();
        } else if (bj[k] == j) {              // the one lane that owns sample j
            double res;
            if (j == b - 1) {
                res = xs[j];
            } else {                          // numpy.interp, as summary_column has it
                const double cj = bs[k] / norm, cn = bn[k] / norm;
                const double x0 = xs[j], x1 = xs[j + 1];
                if (cj == q[k]) {
                    res = x0;
                } else {
                    const double slope = (x1 - x0) / (cn - cj);
                    res = slope * (q[k] - cj) + x0;
                    if (res != res) {
                        res = slope * (q[k] - cn) + x1;
                        if (res != res && x0 == x1) res = x0;
                    }
                }
            }
            out[r * nq + k] = res;
        }
    }
}

}  // namespace
