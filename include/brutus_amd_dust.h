/*
 * brutus_amd_dust.h -- Bayestar 3-D dust map lookups (brutus_amd.dust; reference dust.py:22-68,
 * 231-299): the HEALPix nested pixel of Galactic coordinates and the multi-resolution map query.
 *
 * Part of the product ABI; included by brutus_amd.h, inside its extern "C" block -- include that
 * header, not this one.  Conventions as there (d_: device memory, h_: host memory).
 * Additive: BRUTUS_ABI_VERSION stays 4.
 */
#ifndef BRUTUS_AMD_DUST_H
#define BRUTUS_AMD_DUST_H

#define BRUTUS_DUST_MAX_ORDER 29     /* nside = 2^order <= 2^29: a pixel index fits 63 bits */
#define BRUTUS_DUST_MAX_LEVELS 30
#define BRUTUS_DUST_MAX_ND 65536

/* Nested HEALPix pixel of n Galactic coordinates (degrees) at nside = 2^order:
 *   d_l, d_b (n) f64;  d_pix (n) i64 out, -1 where b is outside [-90, 90] (NaN too) or l is not
 *   finite.
 * All of it in float64 / int64 with exact sqrt and fmod, a sine / cosine below 1 ulp and without
 * fused multiply-adds, rounded exactly as the host path of brutus_amd.dust rounds: a pixel edge is
 * a discontinuity.  The pixel at a coarser level is
 * pix >> 2 (order - order'), exactly.
 * BRUTUS_EINVAL: n < 1, order outside [0, BRUTUS_DUST_MAX_ORDER], a NULL pointer. */
int brutus_dust_lb2pix(int64_t n, const double *d_l, const double *d_b, int order, int64_t *d_pix,
                       void *stream);

/* The map query for n coordinates: which data row of a multi-resolution map (a partition of part
 * of the sphere into nested pixels of nlev values of nside) holds each of them, and that row.
 *   h_order (nlev) i32: log2(nside) of the levels, strictly increasing
 *   h_off, h_len (nlev) i64: the level's slice of d_hpix / d_row; 0 <= len < 2^31 (an empty level
 *                  matches nothing), off >= 0, off + len <= npix
 *   d_hpix (npix) i64: the nested pixel ids of a level, ascending within its slice
 *   d_row  (npix) i64: the data row of each of them, in [0, npix)  (the caller guarantees it)
 *   d_av_mean, d_av_std (npix, nd) f32: the map;  d_dists (nd) f64 [kpc]
 *   d_l, d_b (n) f64: Galactic degrees
 *   d_idx (n) i64 out: the data row, -1 outside the footprint or for a coordinate
 *                  brutus_dust_lb2pix gives -1.  Where levels overlap the finest one wins, as
 *                  the reference's loop over the levels overwrites.
 * Two output forms, either may be absent (NULL), not both:
 *   d_mean, d_std (n, nd) f32: the rows as they are, NaN where d_idx is -1 (dust.py:277-299)
 *   d_los (n, 3, nd) f64, d_ok (n) i32: what brutus_post_set_dust takes -- d_dists, mean, std per
 *                  object; entries that are not finite become 0 and d_ok is 0 for that object (and
 *                  where d_idx is -1), else 1.  This form needs nd >= 2 (the caller widens a
 *                  one-node profile on the host).
 * BRUTUS_EINVAL: n < 1, nlev outside [1, BRUTUS_DUST_MAX_LEVELS], nd outside
 * [1, BRUTUS_DUST_MAX_ND], npix outside [1, 2^31), bad levels, a NULL input, d_mean without d_std
 * or d_los without d_ok (and the reverse), no output form -- checked before any HIP call. */
int brutus_dust_query(int nlev, const int32_t *h_order, const int64_t *h_off, const int64_t *h_len,
                      const int64_t *d_hpix, const int64_t *d_row, int64_t npix, int nd,
                      const float *d_av_mean, const float *d_av_std, const double *d_dists,
                      int64_t n, const double *d_l, const double *d_b, int64_t *d_idx,
                      float *d_mean, float *d_std, double *d_los, int32_t *d_ok, void *stream);

#endif /* BRUTUS_AMD_DUST_H */
