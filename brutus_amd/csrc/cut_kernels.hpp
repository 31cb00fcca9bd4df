// cut_kernels.hpp -- brutus_cut_batch: external label constraints, parallax clip and first
// `wt_thresh` cut on the full-grid planes of brutus_loglike_batch, emitting indexed records
// (reference fitting.py:1995-2009, :976-991, pdf.py:209-220).  Included by brutus_kernels.hip only
// (it defines kernels); needs fit_kernels.hpp (first_cut_lnprob) and grid_kernels.hpp (prep_parallax).
//
// Four streaming passes over (star, model); a star's models are cut into CUT_NCH contiguous
// chunks of `span` models, one workgroup per (chunk, star), each lane two adjacent models:
//   k_cut_stat     lnl (+ constraints, in registers), scale, icov00 -> lnprob plane (workspace),
//                  one partial maximum per (chunk, star)
//   k_cut_count    the star's threshold from its partial maxima; selected models per chunk
//   k_cut_offsets  exclusive scan of the counts in (star, chunk) order: record offsets, total
//   k_cut_scatter  lnl + constraints written back (same code, same bits as the first pass),
//                  records of the selected models in ascending model order
// lnprob is kept in a workspace plane between the passes rather than recomputed: per model the
// three later reads of it cost 8 B each against 24 B (lnl, scale, icov00) plus the label columns
// for every recomputation.  The lnl plane is only written after the caller's buffers are known
// to be large enough, so a call that fails with BRUTUS_ENOMEM leaves its inputs as they were
// and is simply repeated.
#pragma once

#include "grid_kernels.hpp"
#include "fit_kernels.hpp"

namespace {

constexpr int CUT_NCH = TILE;        // chunks per star (= lanes of the workgroup that reduces their maxima)
constexpr int CUT_OFF_T = 1024;      // threads of the one-workgroup scan

// One external constraint added to lnl, in the reference's order (fitting.py:2003-2008:
// `c = (label - mean)**2; c *= 1. / std**2; lnl += -0.5 * (c + log(2 pi std^2))`), every
// operation rounded on its own.  The pragma is what keeps `c * ivar + lnc` from becoming one
// FMA: HIP's __dmul_rn / __dadd_rn are the plain operators and are contracted like them.
__device__ __forceinline__ double cut_add_ext(double lnl, double lab, double mean, double ivar,
                                              double lnc) {
#pragma clang fp contract(off)
    const double d = lab - mean;
    double c = d * d;
    c = c * ivar;
    const double t = c + lnc;
    return lnl + -0.5 * t;
}

// Models m, m + 1 of a row (m even).  VEC: one 16-byte load (the host checked the alignment
// and that nmodel is even); otherwise two 8-byte loads, the second only inside the row.
template <bool VEC>
__device__ __forceinline__ void cut_load2(const double *__restrict__ row, int64_t m, bool v1,
                                          double &a, double &b) {
    if constexpr (VEC) {
        const double2 t = *reinterpret_cast<const double2 *>(row + m);
        a = t.x;
        b = t.y;
    } else {
        a = row[m];
        b = v1 ? row[m + 1] : 0.;
    }
}

// lnl + the star's active constraints for models m, m + 1.  ext_par = (next, nstar, 3):
// mean, 1 / std^2, ln(2 pi std^2); a constraint the host skips has mean = NaN.
template <bool VEC>
__device__ __forceinline__ bool cut_apply_ext(int next, int nstar, int s, int64_t nmodel,
                                              const double *__restrict__ labels,
                                              const double *__restrict__ ext_par, int64_t m,
                                              bool v1, double &l0, double &l1) {
    bool any = false;
    for (int k = 0; k < next; ++k) {
        const double *q = ext_par + ((int64_t)k * nstar + s) * 3;
        const double mean = q[0];
        if (!isfinite(mean)) continue;
        double a, b;
        cut_load2<VEC>(labels + (int64_t)k * nmodel, m, v1, a, b);
        l0 = cut_add_ext(l0, a, mean, q[1], q[2]);
        l1 = cut_add_ext(l1, b, mean, q[1], q[2]);
        any = true;
    }
    return any;
}

// grid (CUT_NCH, nstar).  lnprob plane: row stride `stride` (even, >= nmodel), 16-byte aligned.
template <bool VEC>
__global__ void __launch_bounds__(TILE)
k_cut_stat(int64_t nmodel, int64_t stride, int64_t span, int nstar,
           const double *__restrict__ lnl, const double *__restrict__ scale,
           const double *__restrict__ icov00, const double *__restrict__ par,
           const double *__restrict__ perr, int has_parallax, int next,
           const double *__restrict__ labels, const double *__restrict__ ext_par,
           double *__restrict__ lnprob, double *__restrict__ part) {
    __shared__ double slot[4];
    const int s = blockIdx.y, c = blockIdx.x;
    StarPrep sp;                     // (only the parallax fields are filled and read)
    prep_parallax(sp, has_parallax, par, perr, s);
    const int64_t row = (int64_t)s * nmodel;
    const int64_t m_end = min(nmodel, (int64_t)(c + 1) * span);
    double mx = -INFINITY;
    for (int64_t m = (int64_t)c * span + 2 * threadIdx.x; m < m_end; m += 2 * TILE) {
        const bool v1 = m + 1 < nmodel;
        double l0, l1, s0, s1, i0, i1;
        cut_load2<VEC>(lnl + row, m, v1, l0, l1);
        cut_load2<VEC>(scale + row, m, v1, s0, s1);
        cut_load2<VEC>(icov00 + row, m, v1, i0, i1);
        cut_apply_ext<VEC>(next, nstar, s, nmodel, labels, ext_par, m, v1, l0, l1);
        const double p0 = first_cut_lnprob(sp, l0, s0, i0);
        const double p1 = v1 ? first_cut_lnprob(sp, l1, s1, i1) : -INFINITY;
        *reinterpret_cast<double2 *>(lnprob + (int64_t)s * stride + m) = make_double2(p0, p1);
        mx = p0 > mx ? p0 : mx;
        mx = p1 > mx ? p1 : mx;
    }
    block_max_store(mx, slot, part + (int64_t)s * CUT_NCH + c);
}

// grid (CUT_NCH, nstar): thr[s] = ln_wt + max_m lnprob (fitting.py:985), counts[(s, c)] =
// models of the chunk with lnprob > thr.
__global__ void __launch_bounds__(TILE)
k_cut_count(int64_t nmodel, int64_t stride, int64_t span, const double *__restrict__ lnprob,
            const double *__restrict__ part, double ln_wt, double *__restrict__ thr_out,
            int32_t *__restrict__ counts) {
    static_assert(CUT_NCH == TILE, "one lane per partial maximum");
    __shared__ double slot[4];
    __shared__ double s_max;
    __shared__ int32_t s_sum[TILE / 64 + 1];
    const int s = blockIdx.y, c = blockIdx.x;
    block_max_store(part[(int64_t)s * CUT_NCH + threadIdx.x], slot, &s_max);
    const double thr = ln_wt + s_max;
    if (c == 0 && threadIdx.x == 0) thr_out[s] = thr;
    const int64_t m_end = min(nmodel, (int64_t)(c + 1) * span);
    int32_t n = 0;
    for (int64_t m = (int64_t)c * span + 2 * threadIdx.x; m < m_end; m += 2 * TILE) {
        const double2 p = *reinterpret_cast<const double2 *>(lnprob + (int64_t)s * stride + m);
        n += (p.x > thr ? 1 : 0) + (m + 1 < nmodel && p.y > thr ? 1 : 0);
    }
    int32_t total;
    block_exclusive_sum<int32_t, TILE>(n, s_sum, total);
    if (threadIdx.x == 0) counts[(int64_t)s * CUT_NCH + c] = total;
}

// One workgroup: offsets[(s, c)] = rec_base + exclusive sum of the counts in (s, c) order,
// rec_off[s] = offsets[(s, 0)], rec_off[nstar] = rec_base + total, *total_out = total.
__global__ void __launch_bounds__(CUT_OFF_T)
k_cut_offsets(int nstar, const int32_t *__restrict__ counts, int64_t rec_base,
              int64_t *__restrict__ offsets, int64_t *__restrict__ rec_off,
              int64_t *__restrict__ total_out) {
    __shared__ int64_t s_sum[CUT_OFF_T / 64 + 1];
    const int total = nstar * CUT_NCH;
    const int ept = (total + CUT_OFF_T - 1) / CUT_OFF_T;
    const int e0 = threadIdx.x * ept;
    const int e1 = min(total, e0 + ept);
    int64_t sum = 0;
    for (int e = e0; e < e1; ++e) sum += counts[e];
    int64_t all;
    int64_t pre = rec_base + block_exclusive_sum<int64_t, CUT_OFF_T>(sum, s_sum, all);
    for (int e = e0; e < e1; ++e) {
        offsets[e] = pre;
        if (e % CUT_NCH == 0) rec_off[e / CUT_NCH] = pre;
        pre += counts[e];
    }
    if (threadIdx.x == 0) {
        rec_off[nstar] = rec_base + all;
        *total_out = all;
    }
}

struct CutPlanes {           // the eleven value planes in record order, each (nstar, nmodel)
    const double *v[BRUTUS_NVALS];
};

// grid (CUT_NCH, nstar).  Writes lnl + constraints back into the lnl plane (when a constraint
// of the star is active) and the records of the chunk's selected models: positions from the
// chunk's offset plus a workgroup prefix sum over the lanes' counts, so model order is kept.
// Every record row r written lies in [rec_base, rec_base + total) <= capacity (host-checked).
template <bool VEC>
__global__ void __launch_bounds__(TILE)
k_cut_scatter(int64_t nmodel, int64_t stride, int64_t span, int nstar,
              const double *__restrict__ lnprob, const double *__restrict__ thr_in,
              const int32_t *__restrict__ counts, const int64_t *__restrict__ offsets,
              double *__restrict__ lnl, CutPlanes pl, int next,
              const double *__restrict__ labels, const double *__restrict__ ext_par,
              int64_t capacity, int32_t *__restrict__ rec_idx, int32_t *__restrict__ rec_slot,
              double *__restrict__ rec_vals) {
    __shared__ int32_t s_sum[TILE / 64 + 1];
    const int s = blockIdx.y, c = blockIdx.x;
    const int64_t row = (int64_t)s * nmodel;
    const int64_t m_beg = (int64_t)c * span, m_end = min(nmodel, m_beg + span);
    const bool emit = counts[(int64_t)s * CUT_NCH + c] > 0;       // (uniform over the workgroup)
    bool ext_on = false;
    for (int k = 0; k < next; ++k) ext_on = ext_on || isfinite(ext_par[((int64_t)k * nstar + s) * 3]);
    if (!emit && !ext_on) return;
    const double thr = thr_in[s];
    int64_t run = offsets[(int64_t)s * CUT_NCH + c];
    for (int64_t mb = m_beg; mb < m_end; mb += 2 * TILE) {        // (uniform trip count: barriers inside)
        const int64_t m = mb + 2 * threadIdx.x;
        const bool v0 = m < m_end, v1 = m + 1 < nmodel && v0;
        double l0 = 0., l1 = 0.;
        if (ext_on && v0) {
            cut_load2<VEC>(lnl + row, m, v1, l0, l1);
            cut_apply_ext<VEC>(next, nstar, s, nmodel, labels, ext_par, m, v1, l0, l1);
            lnl[row + m] = l0;
            if (v1) lnl[row + m + 1] = l1;
        }
        if (!emit) continue;
        bool sel0 = false, sel1 = false;
        if (v0) {
            const double2 p = *reinterpret_cast<const double2 *>(lnprob + (int64_t)s * stride + m);
            sel0 = p.x > thr;
            sel1 = v1 && p.y > thr;
        }
        int32_t tot;
        const int32_t pre = block_exclusive_sum<int32_t, TILE>((int32_t)sel0 + (int32_t)sel1, s_sum, tot);
        int64_t r = run + pre;
        run += tot;
        if (sel0) {
            rec_idx[r] = (int32_t)m;
            rec_slot[r] = (int32_t)r;
            rec_vals[r] = ext_on ? l0 : pl.v[0][row + m];
#pragma unroll
            for (int q = 1; q < BRUTUS_NVALS; ++q) rec_vals[(int64_t)q * capacity + r] = pl.v[q][row + m];
            ++r;
        }
        if (sel1) {
            rec_idx[r] = (int32_t)(m + 1);
            rec_slot[r] = (int32_t)r;
            rec_vals[r] = ext_on ? l1 : pl.v[0][row + m + 1];
#pragma unroll
            for (int q = 1; q < BRUTUS_NVALS; ++q)
                rec_vals[(int64_t)q * capacity + r] = pl.v[q][row + m + 1];
        }
    }
}

}  // namespace
