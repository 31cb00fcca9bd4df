// dust_unit.hip -- translation unit of libbrutus_amd.so: Bayestar 3-D dust map lookups
// (brutus_dust_*; reference dust.py:22-68, 231-299, dust_kernels.hpp).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/brutus_amd.h"

#include "host.hpp"
#include "dust_kernels.hpp"

namespace {
static unsigned dust_blocks(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }
// (the gather runs as few as 4 objects per workgroup: 2^29 workgroups at the most)
constexpr int64_t DUST_MAX_N = INT32_MAX;
}  // namespace

extern "C" {

int brutus_dust_lb2pix(int64_t n, const double *d_l, const double *d_b, int order, int64_t *d_pix,
                       void *stream) {
    if (n < 1 || n > DUST_MAX_N) return fail(BRUTUS_EINVAL, "bad dust dimensions (n=%lld)", (long long)n);
    if (order < 0 || order > BRUTUS_DUST_MAX_ORDER)
        return fail(BRUTUS_EINVAL, "bad HEALPix order %d (0 .. %d)", order, BRUTUS_DUST_MAX_ORDER);
    if (!d_l || !d_b || !d_pix) return fail(BRUTUS_EINVAL, "NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    tm.begin("k_dust_lb2pix");
    hipLaunchKernelGGL(k_dust_lb2pix, dim3(dust_blocks(n, DUST_BLOCK)), dim3(DUST_BLOCK), 0, st, n, d_l, d_b,
                       order, d_pix);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

int brutus_dust_query(int nlev, const int32_t *h_order, const int64_t *h_off, const int64_t *h_len,
                      const int64_t *d_hpix, const int64_t *d_row, int64_t npix, int nd,
                      const float *d_av_mean, const float *d_av_std, const double *d_dists,
                      int64_t n, const double *d_l, const double *d_b, int64_t *d_idx,
                      float *d_mean, float *d_std, double *d_los, int32_t *d_ok, void *stream) {
    if (n < 1 || n > DUST_MAX_N || nlev < 1 || nlev > BRUTUS_DUST_MAX_LEVELS || nd < 1 ||
        nd > BRUTUS_DUST_MAX_ND || npix < 1 || npix > INT32_MAX)
        return fail(BRUTUS_EINVAL, "bad dust dimensions (n=%lld, nlev=%d, nd=%d, npix=%lld)", (long long)n, nlev,
                    nd, (long long)npix);
    if (!h_order || !h_off || !h_len || !d_hpix || !d_row || !d_av_mean || !d_av_std || !d_dists || !d_l ||
        !d_b || !d_idx)
        return fail(BRUTUS_EINVAL, "NULL pointer");
    if ((d_mean == nullptr) != (d_std == nullptr) || (d_los == nullptr) != (d_ok == nullptr))
        return fail(BRUTUS_EINVAL, "a dust output form is two arrays (d_mean + d_std, d_los + d_ok)");
    if (!d_mean && !d_los) return fail(BRUTUS_EINVAL, "no dust output form");
    if (d_los && nd < 2) return fail(BRUTUS_EINVAL, "the d_los form needs nd >= 2 (nd=%d)", nd);
    DustLevels lv;
    for (int k = 0; k < nlev; ++k) {
        if (h_order[k] < 0 || h_order[k] > BRUTUS_DUST_MAX_ORDER || (k && h_order[k] <= h_order[k - 1]))
            return fail(BRUTUS_EINVAL, "bad dust level %d: order %d (0 .. %d, strictly increasing)", k,
                        (int)h_order[k], BRUTUS_DUST_MAX_ORDER);
        if (h_off[k] < 0 || h_len[k] < 0 || h_len[k] > INT32_MAX || h_off[k] > npix - h_len[k])
            return fail(BRUTUS_EINVAL, "bad dust level %d: slice (%lld, %lld) of %lld", k, (long long)h_off[k],
                        (long long)h_len[k], (long long)npix);
        lv.off[k] = h_off[k];
        lv.len[k] = (int32_t)h_len[k];
    }
    lv.nlev = nlev;
    lv.order_deep = h_order[nlev - 1];
    for (int k = 0; k < nlev; ++k) lv.shift[k] = 2 * (lv.order_deep - h_order[k]);
    for (int k = nlev; k < DUST_MAX_LEVELS; ++k) lv.off[k] = lv.len[k] = lv.shift[k] = 0;

    int lg = 3;                                     // lanes per object: 8 .. 64, along the bins
    while (lg < 6 && (1 << lg) < nd) ++lg;
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    tm.begin("k_dust_index");
    hipLaunchKernelGGL(k_dust_index, dim3(dust_blocks(n, DUST_BLOCK)), dim3(DUST_BLOCK), 0, st, lv, d_hpix,
                       d_row, n, d_l, d_b, d_idx);
    tm.end();
    tm.begin("k_dust_gather");
    hipLaunchKernelGGL(k_dust_gather, dim3(dust_blocks(n, DUST_BLOCK >> lg)), dim3(DUST_BLOCK), 0, st, lg, n, nd,
                       (const int64_t *)d_idx, d_av_mean, d_av_std, d_dists, d_mean, d_std, d_los, d_ok);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

}  // extern "C"
