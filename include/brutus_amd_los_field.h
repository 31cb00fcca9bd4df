/*
 * brutus_amd_los_field.h -- the line-of-sight cloud likelihood of MANY sightlines in one call
 * (brutus_amd.los.LOSField): a ragged set of sightlines, each with its own stars and draws, all
 * fitted with the same model; K thetas per sightline per call.
 *
 * Part of the product ABI; included by brutus_amd.h, inside its extern "C" block, after
 * brutus_los_params and the BRUTUS_LOS_MAX_* limits it uses -- include that header, not this one.
 * Conventions as there (d_: device memory, h_: host memory).
 * Additive: BRUTUS_ABI_VERSION stays 4.
 *
 * Layout.  Sightline s has nobj_s stars and ndraws_s draws per star.  Its draws are one
 * DRAW-major block (ndraws_s, nobj_s), as brutus_los_loglike takes them; the blocks of all
 * sightlines lie end to end in d_dsamps / d_rsamps, the template values and the columns of the
 * terms in the order of the stars.  A tile is 64 consecutive stars of ONE sightline: the tiles of
 * sightline s start at its first star, the last one is partial, none crosses into the next
 * sightline.  Two tables say where everything is; brutus_los_field_plan fills them and is their
 * only definition:
 *   sightline table (nsight, BRUTUS_LOSFIELD_COLS) i64, per sightline
 *       [BRUTUS_LOSFIELD_STAR0]  its first star = sum of nobj of the sightlines before it
 *       [BRUTUS_LOSFIELD_DRAW0]  the first element of its draw block = sum of ndraws nobj before it
 *       [BRUTUS_LOSFIELD_TILE0]  its first tile = sum of ceil(nobj / 64) before it
 *       [BRUTUS_LOSFIELD_NOBJ], [BRUTUS_LOSFIELD_NDRAWS]
 *       [BRUTUS_LOSFIELD_LNDRAWS] the bits of the double ln(ndraws), the divisor of every star's sum
 *   tile table (ntiles) i32: the sightline of every tile.
 */
#ifndef BRUTUS_AMD_LOS_FIELD_H
#define BRUTUS_AMD_LOS_FIELD_H

#define BRUTUS_LOSFIELD_MAX_SIGHTLINES (1 << 20)
#define BRUTUS_LOSFIELD_MAX_TILES ((1 << 20) + (1 << 16))   /* MAX_SIGHTLINES + BRUTUS_LOS_MAX_OBJ / 64 */
#define BRUTUS_LOSFIELD_COLS 6
#define BRUTUS_LOSFIELD_STAR0 0
#define BRUTUS_LOSFIELD_DRAW0 1
#define BRUTUS_LOSFIELD_TILE0 2
#define BRUTUS_LOSFIELD_NOBJ 3
#define BRUTUS_LOSFIELD_NDRAWS 4
#define BRUTUS_LOSFIELD_LNDRAWS 5
/* flags of brutus_los_field_loglike */
#define BRUTUS_LOSFIELD_CHECK_THETA 1   /* the device decides the rows the host would (below) */
#define BRUTUS_LOSFIELD_MONOTONIC 2     /* with CHECK_THETA: falling reddenings give -inf */

/* The tables of nsight sightlines with h_nobj[s] stars and h_ndraws[s] draws each (host code, no
 * HIP call).  h_totals (3) out: the stars, the elements of the concatenated draws, the tiles.
 * h_sightlines (nsight, BRUTUS_LOSFIELD_COLS) and h_tiles (ntiles_cap) out, or both NULL to ask
 * for h_totals alone.  BRUTUS_EINVAL: nsight outside [1, BRUTUS_LOSFIELD_MAX_SIGHTLINES], a
 * sightline with nobj < 1 or ndraws outside [1, BRUTUS_LOS_MAX_DRAWS] (it is named), more than
 * BRUTUS_LOS_MAX_OBJ stars in all, a NULL input, one table without the other, ntiles_cap below the
 * number of tiles. */
int brutus_los_field_plan(int nsight, const int32_t *h_nobj, const int32_t *h_ndraws,
                          int64_t *h_sightlines, int32_t *h_tiles, int64_t ntiles_cap,
                          int64_t *h_totals);

/* Bytes of workspace for ntheta rows per sightline of a field of ntiles tiles: one double per
 * (row, tile), rounded up to 256.  0: ntiles outside [1, BRUTUS_LOSFIELD_MAX_TILES] or ntheta
 * outside [1, BRUTUS_LOS_MAX_THETA]. */
size_t brutus_los_field_workspace_bytes(int64_t ntiles, int ntheta);

/* ln L of ntheta profiles PER SIGHTLINE, for all nsight sightlines; model, limits and arithmetic
 * as brutus_los_loglike, whose bytes a sightline's values are: the same per-star code, the same
 * tiles, the same order of every sum -- whatever else is in the field and wherever the sightline
 * stands in it.
 *   nstars, ntiles     h_totals[0] and h_totals[2] of the plan
 *   d_dsamps, d_rsamps f64: the concatenated draw-major blocks (h_totals[1] elements)
 *   d_template (nstars) f64 or NULL
 *   d_sightlines, d_tiles: the plan's tables, copied to the device
 *   d_theta (nsight, ntheta, 4 + 2 nclouds) f64: row k of sightline s is that sightline's alone
 *   flags              0: every row is evaluated as it stands (the caller has checked it).
 *                      BRUTUS_LOSFIELD_CHECK_THETA: a row's value is decided here, in this order,
 *                      a later rule overriding an earlier one: NaN where s0 or s is not > 0; NaN
 *                      where the cloud distances do not ascend (or one is NaN); with
 *                      BRUTUS_LOSFIELD_MONOTONIC, -inf where the reddenings [fred, r1, ...] fall
 *                      anywhere (or one is NaN).  The row's terms take the same value.
 *   d_loglike (nsight, ntheta) f64 out
 *   d_terms f64 out or NULL: per sightline a block (ntheta, nobj_s), the blocks in the order of
 *                      the sightlines (that of s begins at ntheta x its first star)
 * BRUTUS_EINVAL: nsight outside [1, BRUTUS_LOSFIELD_MAX_SIGHTLINES], nstars outside
 * [nsight, BRUTUS_LOS_MAX_OBJ], ntiles outside [nsight, BRUTUS_LOSFIELD_MAX_TILES] or outside
 * [ceil(nstars / 64), nsight + nstars / 64], ntheta outside [1, BRUTUS_LOS_MAX_THETA], nclouds outside
 * [0, BRUTUS_LOS_MAX_CLOUDS], unknown flags, the parameters as in brutus_los_loglike, a NULL
 * pointer; BRUTUS_ENOMEM: workspace -- all checked before any HIP call.  What the tables say
 * (ndraws_s <= BRUTUS_LOS_MAX_DRAWS among it) is the plan's to check: they are read as they are. */
int brutus_los_field_loglike(int nsight, int64_t nstars, int64_t ntiles, const double *d_dsamps,
                             const double *d_rsamps, const double *d_template,
                             const int64_t *d_sightlines, const int32_t *d_tiles, int ntheta,
                             int nclouds, const double *d_theta, const brutus_los_params *params,
                             int flags, double *d_loglike, double *d_terms, void *d_workspace,
                             size_t workspace_bytes, void *stream);

#endif /* BRUTUS_AMD_LOS_FIELD_H */
