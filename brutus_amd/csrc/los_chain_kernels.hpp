// los_chain_kernels.hpp -- a field's chains to its dust map (brutus_amd.los.LOSChainSummary;
// include/brutus_amd_los_chain.h).  Included by los_unit.hip alone.
//
// The chain is (nkept, S, W, P) float64 as LOSFieldSampler.run lays it out; sample n = k W + w of
// column (s, p) is chain[k, s, w, p], N = nkept W samples per column.
//
// k_los_chain_select<Source>: exact order statistics of many columns, without sorting and without
// a limit on N but the ABI's.  A workgroup (256 lanes) serves ONE sightline and a tile of `tc`
// columns; a column's targets are the ranks j and j + 1 of each q (T = 2 nq of them).  MSD radix
// select on the order-preserving 64-bit keys of summary_kernels.hpp (chain_key keeps -0 below +0):
// eight passes of 8-bit digits, most significant first.  In a pass every lane walks its samples,
// forms the tile's keys from ONE read of the sample's row, and counts the digit of every key whose
// higher digits equal a target's prefix in that prefix's 256-bin LDS histogram; then one wave per
// target scans its histogram (4 bins a lane, a shuffle scan) for the digit that holds the rank,
// which extends the prefix and reduces the rank to one inside that bin.  After eight passes the
// prefix IS the key of the order statistic.  Targets of a column whose prefixes are equal share
// one histogram (all of them in pass 0, j and j + 1 mostly to the end), so a key is counted once
// per distinct prefix; a lane compares its key with the column's distinct prefixes four at a time
// (independent LDS reads: one dependent read per prefix cost 40 % more time).  Counters are integers: the LDS atomics commute and the result is the same
// bytes in every run.  Digits of near-equal keys collide on one bin (every key of a column of
// reddenings in [0, 6) has the same top byte), so the lanes of a wave that share the first
// active lane's bin add their count with ONE atomic; the rest add one each.  Histogram rows are
// 257 words apart: the scanning waves of different targets then start on different banks.
// LDS: 32 histograms (32.1 KiB) + 0.7 KiB of state, so tc = min(8, 32 / T): 3 columns at the five
// default q, 1 at nq = 16.  Four workgroups fit a CU.  No scratch.
//   Source = ParamColumn: column c is parameter c of the row.
//   Source = ProfileColumn: column c is the model's reddening at distance modulus dgrid[c]: with
//   k = the number of cloud distances row[4 + 2 i] <= dgrid[c], row[3] for k = 0, else
//   row[3 + 2 k] (+ row[3], one rounding, if additive).  The profile never exists in memory.
// The last step interpolates x_j + f (x_{j+1} - x_j), rounded as written, f = pos - floor(pos),
// pos = q (N - 1); x_j itself for f = 0; NaN for a column that holds a NaN or a q outside [0, 1].
//
// k_los_chain_moments: one workgroup per (sightline, parameter).  mean and std (ddof 1) over all
// N samples, two-pass, shifted by the column's first sample; then the split-R-hat: a lane is a
// sequence (walker w's first or last L = nkept / 2 kept steps), walks it twice (mean, then variance,
// shifted by the sequence's first sample) and leaves its mean in the caller's workspace; the
// variance of the 2 W means is two-pass again, shifted by the first mean.  Every sum across lanes
// is a lane's running sum in the order of its items, then a fixed tree over the 256 lanes.
// k_los_chain_best: one workgroup per sightline, the sample with the largest ln L (the first in
// n-order among ties; a NaN never wins) and its row.
#pragma once

#include "summary_kernels.hpp"

namespace {

constexpr int LOSCHAIN_BLOCK = 256;
constexpr int LOSCHAIN_HISTS = 32;           // histograms of a workgroup = tc * T at the most
constexpr int LOSCHAIN_HIST_STRIDE = 257;    // words between two histograms
constexpr int LOSCHAIN_TC_MAX = 8;           // columns of a tile at the most

struct LosChainDims {
    const double *chain;
    int64_t nkept;
    int nsight, nwalkers, ncol;              // S, W, P
    unsigned nsamp;                          // N = nkept W <= 2^24
};

struct LosChainSelect {
    LosChainDims d;
    const double *q;
    double *out;                             // (S, ncols, nq)
    int nq, ncols, tc, ntiles;               // columns in all, per tile, tiles per sightline
};

// summary_key with -0 below +0 (there they are one key); summary_unkey inverts it as it is
__device__ __forceinline__ uint64_t chain_key(double x) {
    return (x == 0. && (__double_as_longlong(x) < 0)) ? 0x7fffffffffffffffull : summary_key(x);
}

__device__ __forceinline__ const double *chain_row(const LosChainDims &d, int s, unsigned n) {
    const unsigned k = n / (unsigned)d.nwalkers, w = n - k * (unsigned)d.nwalkers;
    return d.chain + (((int64_t)k * d.nsight + s) * d.nwalkers + w) * (int64_t)d.ncol;
}

// A source gives the tile's values of one sample from its row.  (Two or four samples in flight per
// lane were measured: 13 % and 45 % slower at 16 000 samples, the registers cost a workgroup per CU.)
struct ParamColumn {
    __device__ __forceinline__ void init(int, int) {}
    __device__ __forceinline__ void values(const double *row, int c0, int tc, double (&v)[LOSCHAIN_TC_MAX]) const {
#pragma unroll
        for (int c = 0; c < LOSCHAIN_TC_MAX; ++c) v[c] = c < tc ? row[c0 + c] : 0.;
    }
};

struct ProfileColumn {
    const double *dgrid;
    int nclouds, additive;
    double mu[LOSCHAIN_TC_MAX];
    __device__ __forceinline__ void init(int c0, int tc) {
#pragma unroll
        for (int c = 0; c < LOSCHAIN_TC_MAX; ++c) mu[c] = c < tc ? dgrid[c0 + c] : 0.;
    }
    __device__ __forceinline__ void values(const double *row, int, int tc, double (&v)[LOSCHAIN_TC_MAX]) const {
#pragma clang fp contract(off)
        int k[LOSCHAIN_TC_MAX];
#pragma unroll
        for (int c = 0; c < LOSCHAIN_TC_MAX; ++c) k[c] = 0;
        for (int i = 0; i < nclouds; ++i) {
            const double dist = row[4 + 2 * i];
#pragma unroll
            for (int c = 0; c < LOSCHAIN_TC_MAX; ++c) k[c] += dist <= mu[c] ? 1 : 0;
        }
        const double fred = row[3];
#pragma unroll
        for (int c = 0; c < LOSCHAIN_TC_MAX; ++c) {
            v[c] = c < tc ? row[3 + 2 * k[c]] : 0.;          // (k = 0: the foreground itself)
            if (additive && k[c]) v[c] = v[c] + fred;
        }
    }
};

// pos = q (N - 1) of one q: the rank j = floor(pos) and f = pos - j; false for a q outside [0, 1]
__device__ __forceinline__ bool chain_position(double q, unsigned nsamp, unsigned *j, double *f) {
#pragma clang fp contract(off)
    if (!(q >= 0. && q <= 1.)) {
        *j = 0;
        *f = 0.;
        return false;
    }
    const double pos = q * (double)(nsamp - 1);
    const double fl = floor(pos);
    *j = (unsigned)fl < nsamp - 1 ? (unsigned)fl : nsamp - 1;
    *f = pos - fl;
    return true;
}

template <class Source>
__global__ void __launch_bounds__(LOSCHAIN_BLOCK) k_los_chain_select(LosChainSelect c, Source src) {
    __shared__ uint32_t hist[LOSCHAIN_HISTS * LOSCHAIN_HIST_STRIDE];
    __shared__ uint64_t prefix[LOSCHAIN_HISTS];       // per target: the digits found so far
    __shared__ uint32_t rank[LOSCHAIN_HISTS];         // per target: its rank among the keys of its prefix
    __shared__ int lead[LOSCHAIN_HISTS];              // per target: the histogram of its prefix
    __shared__ uint64_t distinct[LOSCHAIN_HISTS + 4]; // per column (T slots each): its distinct prefixes
    __shared__ int nlead[LOSCHAIN_TC_MAX];
    __shared__ int has_nan[LOSCHAIN_TC_MAX];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int s = blockIdx.x / c.ntiles, c0 = (blockIdx.x % c.ntiles) * c.tc;
    const int tc = c.ncols - c0 < c.tc ? c.ncols - c0 : c.tc;
    const int T = 2 * c.nq, ntarget = tc * T;
    const unsigned N = c.d.nsamp;

    if (t < ntarget) {
        unsigned j;
        double f;
        chain_position(c.q[(t % T) >> 1], N, &j, &f);
        rank[t] = (t & 1) && j + 1 < N ? j + 1 : j;
        prefix[t] = 0;
    }
    if (t < LOSCHAIN_TC_MAX) has_nan[t] = 0;
    src.init(c0, tc);

    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        __syncthreads();                              // (the targets of the last pass are written)
        for (int i = t; i < ntarget * LOSCHAIN_HIST_STRIDE; i += LOSCHAIN_BLOCK) hist[i] = 0;
        if (t < tc) {                                 // the column's distinct prefixes, one histogram each
            int n = 0;
            for (int a = 0; a < T; ++a) {
                int mine = -1;
                for (int b = 0; b < n; ++b)
                    if (distinct[t * T + b] == prefix[t * T + a]) mine = b;
                if (mine < 0) {
                    mine = n++;
                    distinct[t * T + mine] = prefix[t * T + a];
                }
                lead[t * T + a] = t * T + mine;
            }
            nlead[t] = n;
        }
        __syncthreads();

        // (every lane of a wave goes round together: the ballots below need them all)
        for (unsigned n0 = 0; n0 < N; n0 += LOSCHAIN_BLOCK) {
            const bool live = n0 + t < N;
            double v[LOSCHAIN_TC_MAX];
            src.values(chain_row(c.d, s, live ? n0 + t : 0), c0, tc, v);
#pragma unroll
            for (int col = 0; col < LOSCHAIN_TC_MAX; ++col) {
                if (col >= tc) break;
                const double x = v[col];
                const uint64_t key = chain_key(x);
                if (pass == 0 && live && x != x) has_nan[col] = 1;
                const uint64_t high = pass ? key >> (shift + 8) : 0;
                // (four prefixes a round: independent LDS reads, not a chain of them)
                int hit = -1;
                const int nl = nlead[col];
                const uint64_t *mine = distinct + col * T;
                for (int i = 0; i < nl; i += 4) {
                    const uint64_t p0 = mine[i], p1 = mine[i + 1], p2 = mine[i + 2], p3 = mine[i + 3];
                    if (p0 == high) hit = i;
                    if (p1 == high && i + 1 < nl) hit = i + 1;
                    if (p2 == high && i + 2 < nl) hit = i + 2;
                    if (p3 == high && i + 3 < nl) hit = i + 3;
                }
                const int bin = live && hit >= 0 ? (col * T + hit) * LOSCHAIN_HIST_STRIDE + (int)((key >> shift) & 0xff)
                                                 : -1;
                const unsigned long long any = __ballot(bin >= 0);
                if (any) {
                    const int first = __ffsll(any) - 1;
                    const int bin0 = __shfl(bin, first);
                    const unsigned long long same = __ballot(bin == bin0);
                    if (bin == bin0) {
                        if (lane == first) atomicAdd(&hist[bin0], (uint32_t)__popcll(same));
                    } else if (bin >= 0) {
                        atomicAdd(&hist[bin], 1u);
                    }
                }
            }
        }
        __syncthreads();

        // one wave per target: the digit whose bin holds the rank
        for (int a = wave; a < ntarget; a += LOSCHAIN_BLOCK / 64) {
            const uint32_t *h = hist + lead[a] * LOSCHAIN_HIST_STRIDE + 4 * lane;
            const uint32_t h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3];
            const uint32_t mine = h0 + h1 + h2 + h3;
            uint32_t incl = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d);
                if (lane >= d) incl += up;
            }
            const uint32_t r = rank[a];
            const uint64_t p = prefix[a];
            if (incl - mine <= r && r < incl) {
                uint32_t left = r - (incl - mine);
                int digit = 0;
                if (left >= h0) {
                    left -= h0;
                    digit = 1;
                    if (left >= h1) {
                        left -= h1;
                        digit = 2;
                        if (left >= h2) {
                            left -= h2;
                            digit = 3;
                        }
                    }
                }
                prefix[a] = (p << 8) | (uint64_t)(4 * lane + digit);
                rank[a] = left;
            }
        }
    }
    __syncthreads();

    if (t < tc * c.nq) {
#pragma clang fp contract(off)
        const int col = t / c.nq, qi = t % c.nq;
        unsigned j;
        double f;
        const bool ok = chain_position(c.q[qi], N, &j, &f);
        const double x0 = summary_unkey(prefix[col * T + 2 * qi]), x1 = summary_unkey(prefix[col * T + 2 * qi + 1]);
        double r = x0;
        if (f != 0.) r = x0 + f * (x1 - x0);
        if (!ok || has_nan[col]) r = __longlong_as_double(0x7ff8000000000000ll);
        c.out[((int64_t)s * c.ncols + c0 + col) * c.nq + qi] = r;
    }
}

// ---- moments, split-R-hat and the best sample ---------------------------------------------------

// the sum of every lane's `v` in a fixed order (a tree over the 256 lanes), to every lane
__device__ __forceinline__ double chain_block_sum(double v, double *buf) {
    const int t = threadIdx.x;
    __syncthreads();                                  // (buf may still be read from the last sum)
    buf[t] = v;
    __syncthreads();
    for (int half = LOSCHAIN_BLOCK / 2; half > 0; half >>= 1) {
        if (t < half) buf[t] = buf[t] + buf[t + half];
        __syncthreads();
    }
    return buf[0];
}

struct LosChainMoments {
    LosChainDims d;
    double *mean, *std, *rhat;                        // (S, P)
    double *seq_mean;                                 // workspace (S, P, 2 W)
};

__global__ void __launch_bounds__(LOSCHAIN_BLOCK) k_los_chain_moments(LosChainMoments c) {
#pragma clang fp contract(off)
    __shared__ double buf[LOSCHAIN_BLOCK];
    const int t = threadIdx.x;
    const int s = blockIdx.x / c.d.ncol, p = blockIdx.x % c.d.ncol;
    const unsigned N = c.d.nsamp;
    const int W = c.d.nwalkers;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    // all N samples, shifted by the first
    const double x0 = chain_row(c.d, s, 0)[p];
    double sum = 0.;
    for (unsigned n = t; n < N; n += LOSCHAIN_BLOCK) sum += chain_row(c.d, s, n)[p] - x0;
    const double m = chain_block_sum(sum, buf) / (double)N;
    sum = 0.;
    for (unsigned n = t; n < N; n += LOSCHAIN_BLOCK) {
        const double e = (chain_row(c.d, s, n)[p] - x0) - m;
        sum += e * e;
    }
    const double ss = chain_block_sum(sum, buf);
    const int64_t o = (int64_t)s * c.d.ncol + p;
    if (t == 0) {
        c.mean[o] = x0 + m;
        c.std[o] = sqrt(ss / (double)(N - 1));        // (N = 1: 0 / 0, as numpy has it)
    }

    if (c.d.nkept < 4) {
        if (t == 0) c.rhat[o] = nan;
        return;
    }
    // sequence i = h W + w: walker w, the first (h = 0) or the last (h = 1) L kept steps; the lanes
    // of a wave read neighbouring walkers of one kept step
    const int64_t L = c.d.nkept / 2;
    const int nseq = 2 * W;
    double *means = c.seq_mean + o * nseq;
    const int64_t kstride = (int64_t)c.d.nsight * W * c.d.ncol;
    double vsum = 0.;
    for (int i = t; i < nseq; i += LOSCHAIN_BLOCK) {
        const int w = i < W ? i : i - W;
        const int64_t k0 = i < W ? 0 : c.d.nkept - L;
        const double *x = c.d.chain + ((k0 * c.d.nsight + s) * W + w) * (int64_t)c.d.ncol + p;
        const double first = x[0];
        double a = 0.;
        for (int64_t k = 0; k < L; ++k) a += x[k * kstride] - first;
        const double sm = a / (double)L;
        double b = 0.;
        for (int64_t k = 0; k < L; ++k) {
            const double e = (x[k * kstride] - first) - sm;
            b += e * e;
        }
        means[i] = first + sm;
        vsum += b / (double)(L - 1);
    }
    const double Wv = chain_block_sum(vsum, buf) / (double)nseq;      // (the barriers publish `means`)
    const double m0 = means[0];
    sum = 0.;
    for (int i = t; i < nseq; i += LOSCHAIN_BLOCK) sum += means[i] - m0;
    const double mm = chain_block_sum(sum, buf) / (double)nseq;
    sum = 0.;
    for (int i = t; i < nseq; i += LOSCHAIN_BLOCK) {
        const double e = (means[i] - m0) - mm;
        sum += e * e;
    }
    const double BL = chain_block_sum(sum, buf) / (double)(nseq - 1);
    if (t == 0) c.rhat[o] = sqrt(((double)(L - 1) / (double)L * Wv + BL) / Wv);
}

struct LosChainBest {
    LosChainDims d;
    const double *lnl;                                // (nkept, S, W)
    double *best, *best_lnl;                          // (S, P), (S)
};

// whether (v, n) beats (bv, bn); bn < 0: nothing yet
__device__ __forceinline__ bool chain_beats(double v, int64_t n, double bv, int64_t bn) {
    if (n < 0) return false;
    return bn < 0 || v > bv || (v == bv && n < bn);
}

__global__ void __launch_bounds__(LOSCHAIN_BLOCK) k_los_chain_best(LosChainBest c) {
    __shared__ double bval[LOSCHAIN_BLOCK];
    __shared__ int64_t bidx[LOSCHAIN_BLOCK];
    const int t = threadIdx.x, s = blockIdx.x;
    const unsigned N = c.d.nsamp;
    const unsigned W = (unsigned)c.d.nwalkers;
    double bv = 0.;
    int64_t bn = -1;
    for (unsigned n = t; n < N; n += LOSCHAIN_BLOCK) {
        const unsigned k = n / W, w = n - k * W;
        const double v = c.lnl[((int64_t)k * c.d.nsight + s) * W + w];
        if (v == v && chain_beats(v, n, bv, bn)) {
            bv = v;
            bn = n;
        }
    }
    bval[t] = bv;
    bidx[t] = bn;
    __syncthreads();
    for (int half = LOSCHAIN_BLOCK / 2; half > 0; half >>= 1) {
        if (t < half && chain_beats(bval[t + half], bidx[t + half], bval[t], bidx[t])) {
            bval[t] = bval[t + half];
            bidx[t] = bidx[t + half];
        }
        __syncthreads();
    }
    const int64_t n = bidx[0];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double *row = chain_row(c.d, s, n < 0 ? 0 : (unsigned)n);
    for (int p = t; p < c.d.ncol; p += LOSCHAIN_BLOCK) c.best[(int64_t)s * c.d.ncol + p] = n < 0 ? nan : row[p];
    if (t == 0) c.best_lnl[s] = n < 0 ? nan : bval[0];
}

}  // namespace
