/*
 * brutus_amd.h -- C ABI of the MI355X (gfx950) brute-force photometric fitter.
 *
 * The upstream reference (joshspeagle/brutus) is pure Python; its "native" layer
 * is four numba-jitted loops.  This library replaces exactly that layer plus
 * the full-grid part of `loglike`/`lnpost`:
 *
 *   brutus/utils.py:286-347     _get_seds
 *   brutus/fitting.py:34-271    _optimize_fit_mag
 *   brutus/fitting.py:274-427   _optimize_fit_flux
 *   brutus/fitting.py:430-576   _get_sed_mle
 *   brutus/fitting.py:579-820   loglike            (whole function)
 *   brutus/fitting.py:976-991   lnpost: parallax clip + first `wt_thresh` cut
 *   brutus/utils.py:130-176     _chisquare_logpdf
 *   brutus/cluster.py:336-414   isochrone_loglike hot block (brutus_cluster_lnl)
 *
 * Conventions
 *   - every pointer prefixed d_ is a DEVICE pointer (HBM), h_ is a host pointer;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - all functions return 0 on success, a negative BRUTUS_E* code on failure;
 *     brutus_last_error() returns a human-readable message for the calling thread;
 *   - no allocation happens inside the hot calls: the caller owns every buffer
 *     (sizes from the *_bytes() queries) -- PyTorch tensors in the Python host.
 *
 * The Python host (brutus_amd/fitting.py) binds these with ctypes; see
 * INTEGRATION.md for the stub a maintainer of the reference would add.
 */
#ifndef BRUTUS_AMD_H
#define BRUTUS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BRUTUS_ABI_VERSION 4
#ifndef BRUTUS_MAX_FILT      /* (overridable for A/B builds of the library only: it sizes the per-star blocks) */
#define BRUTUS_MAX_FILT 64   /* bands per call: brutus_loglike_batch (full-grid outputs), offsets */
#endif
#define BRUTUS_MAX_FILT_FIT 32 /* bands per brutus_fit_batch / cluster call (register budget of the list kernels) */
#define BRUTUS_MAX_BATCH 256 /* stars per brutus_*_batch call                     */
#define BRUTUS_NVALS 11      /* lnlike, chi2, scale, av, rv, icov[00,01,02,11,12,22] */

#define BRUTUS_OK 0
#define BRUTUS_EINVAL (-1)    /* bad argument                                      */
#define BRUTUS_ENOMEM (-2)    /* workspace / record buffer too small               */
#define BRUTUS_EHIP (-3)      /* HIP runtime error (message in brutus_last_error)  */
#define BRUTUS_ENOCONV (-4)   /* iteration cap hit (the reference would spin)      */
#define BRUTUS_EPRECISION (-5) /* brutus_fit_batch: the audited float32 error bound does not hold (see there) */

/* Keyword arguments of fitting.loglike (fitting.py:579-585) plus lnpost's
 * wt_thresh (fitting.py:823-827).  av_gauss=None maps to (0, 1e6) on the host
 * exactly like fitting.py:695-696. */
typedef struct brutus_params {
    double avlim[2];
    double av_gauss[2];
    double rvlim[2];
    double rv_gauss[2];
    double ltol;           /* flux-phase tolerance; mag-phase tol = 2.5*ltol     */
    double ltol_subthresh;
    double init_thresh;    /* logl_initthresh                                     */
    double wt_thresh;      /* lnpost first cut; only used by brutus_fit_batch     */
    int32_t dim_prior;     /* logl_dim_prior                                      */
    int32_t max_iter;      /* safety cap on mag sweeps / flux iterations (0 = 65536: the reference has none) */
} brutus_params;

int brutus_abi_version(void);
const char *brutus_last_error(void);

/* ---- model grid ------------------------------------------------------------
 * `utils.load_models` (utils.py:588-591) returns models as (Nmodel, Nfilt, 3)
 * float32 = (mag, R, dR/dRv) per band.  The device grid blob holds the
 * coefficients twice -- a band-major structure-of-arrays
 * [nfilt_pad][3][nmodel_pad] that the full-grid scans stream with coalesced
 * loads, and a model-major [nmodel_pad][nfilt_pad][3] copy for the kernels
 * that gather single models -- followed by the band-major float64 table of
 * unreddened model fluxes 10^(-0.4 mag) (fitting.py:529).
 * nfilt_pad = the compiled band count >= nfilt (see brutus_padded_filters: 8, 12, 16, 24, 32 and,
 * for brutus_loglike_batch only, 48 and 64),
 * nmodel_pad = nmodel rounded up to 256.  Padded entries are zero. */
int brutus_padded_filters(int nfilt);              /* <0 if nfilt unsupported     */
size_t brutus_grid_soa_bytes(int64_t nmodel, int nfilt);
int brutus_grid_relayout(const float *d_models_aos, int64_t nmodel, int nfilt,
                         float *d_grid_soa, void *stream);

/* ---- per-star grid likelihood ---------------------------------------------
 * Inputs for a batch of `nstar` stars (row-major, C order):
 *   d_flux, d_err  (nstar, nfilt) float64 maggies;  d_mask (nstar, nfilt) uint8;
 *   d_parallax, d_parallax_err (nstar,) float64 mas, NaN = no measurement
 *   (the notebooks' convention; `None` in the Python API maps to NaN with
 *   has_parallax=0, see fitting.py:749-756 vs :976-982).
 */
size_t brutus_workspace_bytes(int64_t nmodel, int nfilt, int nstar);

/* fitting.loglike(..., return_vals=True) for every star of the batch, full-grid
 * outputs, each plane (nstar, nmodel) float64; d_icov is (6, nstar, nmodel)
 * holding the unique entries [00, 01, 02, 11, 12, 22] of icov_sar
 * (fitting.py:563-574).  d_ndim (nstar,) int32.  h_k1/h_k2 (optional, host,
 * (nstar,) int32) receive the number of magnitude sweeps / flux iterations.
 * d_av_init / d_rv_init (optional, (nmodel,) float64): per-model starting values of the
 * magnitude phase, `av_init` / `rv_init` of fitting.py:697-703, shared by the stars of the
 * batch; NULL = the prior means av_gauss[0] / rv_gauss[0] (the reference's default). */
int brutus_loglike_batch(const float *d_grid_soa, int64_t nmodel, int nfilt,
                         int nstar, const double *d_flux, const double *d_err,
                         const uint8_t *d_mask, const double *d_parallax,
                         const double *d_parallax_err, int has_parallax,
                         const brutus_params *params, void *d_workspace,
                         size_t workspace_bytes, double *d_lnl, double *d_chi2,
                         double *d_scale, double *d_av, double *d_rv,
                         double *d_icov, int32_t *d_ndim, int32_t *h_k1,
                         int32_t *h_k2, const double *d_av_init,
                         const double *d_rv_init, void *stream);

/* The fit() hot path: loglike + lnpost's parallax clip + first wt_thresh cut
 * (fitting.py:976-991), emitting only the selected models as INDEXED RECORDS:
 *   d_rec_idx  (capacity,) int32   model index, ascending per star (= np.where order)
 *   d_rec_slot (capacity,) int32   column of that record's values in d_rec_vals
 *   d_rec_vals (BRUTUS_NVALS, capacity) float64
 *   d_rec_off  (nstar + 1,) int64  record range of star s is [off[s], off[s+1])
 * i.e. value v of record r is d_rec_vals[v * capacity + d_rec_slot[r]].  The indirection
 * exists because a value is written exactly once, where it is computed: columns
 * [0, ncand) belong to the candidates of the likelihood cull (fitting.py:758-759) in
 * candidate-list order and receive the flux-phase results (fitting.py:778-803) of those
 * that survive it; columns [ncand, ncand + nder) receive the selected models the cull
 * dropped.  Columns of candidates that fail the cull or the first cut are never referenced.
 * When Rv is pinned (rvlim[0] == rvlim[1] == rv_gauss[0]) plane 4 (rv) is NOT written:
 * every record's rv is rv_gauss[0].
 * h_counts (host, 3 x int64): [0] selected models of the batch (= off[nstar]),
 * [1] ncand, [2] columns needed = ncand + nder.  BRUTUS_ENOMEM if [2] > capacity (or
 * already [1] > capacity: then [2] is an estimate): call again with larger buffers.
 * Float32 never produces an output value or a decision here, it only proves models to be below
 * the thresholds; the error bound that rests on is AUDITED on the first call of a process and
 * every BRUTUS_AUDIT_EVERY-th (environment, default 64; 0 = never) after it -- every pair the
 * call re-evaluates in float64 anyway is compared with its float32 value -- and a call whose
 * audit finds |float32 - float64| >= the bound fails with BRUTUS_EPRECISION. */
int brutus_fit_batch(const float *d_grid_soa, int64_t nmodel, int nfilt,
                     int nstar, const double *d_flux, const double *d_err,
                     const uint8_t *d_mask, const double *d_parallax,
                     const double *d_parallax_err, int has_parallax,
                     const brutus_params *params, void *d_workspace,
                     size_t workspace_bytes, int64_t capacity,
                     int32_t *d_rec_idx, int32_t *d_rec_slot, double *d_rec_vals,
                     int64_t *d_rec_off, int32_t *d_ndim, int32_t *h_k1, int32_t *h_k2,
                     int64_t *h_counts, void *stream);

/* The same first cut for the fits brutus_fit_batch does not take -- more than BRUTUS_MAX_FILT_FIT
 * bands, or external per-object Gaussian constraints on model labels (`lnprior_ext`,
 * fitting.py:1995-2009) -- from the full-grid planes brutus_loglike_batch wrote for `nstar` stars
 * (each (nstar, nmodel), d_icov (6, nstar, nmodel)); d_parallax / d_parallax_err / has_parallax
 * as there.  Per star s:
 *   1. for each constraint k < next, in order, that applies to the star:
 *        lnl[m] += -0.5 * ((label_k[m] - mean)^2 * ivar + lnc)
 *      d_ext_labels (next, nmodel) holds the label columns, d_ext_par (next, nstar, 3) holds
 *      (mean, ivar = 1 / std^2, lnc = ln(2 pi std^2)) per (constraint, star), computed by the
 *      caller in host doubles -- no logarithm or division happens on the device.  A constraint
 *      the reference skips (non-finite mean, std <= 0; fitting.py:2002) is passed as mean = NaN.
 *      The operations are performed in exactly this order (subtract, square, times ivar, plus
 *      lnc, times -0.5, add to lnl), each rounded on its own, never contracted to a fused
 *      multiply-add: the sum equals the reference's to the bit.  It is written back into
 *      d_lnl, so the records carry lnlike + constraints like the reference's `results`;
 *   2. lnprob = lnl, plus the scale-space parallax Gaussian when the parallax is finite with
 *      p / err > 4 (fitting.py:976-983, pdf.py:209-220), non-finite -> -1e300 (fitting.py:984);
 *      the same device function as brutus_fit_batch's exact first cut;
 *   3. model m is selected iff lnprob[m] > ln(wt_thresh) + max_m lnprob (strict,
 *      fitting.py:985-991); a star with nothing selected has an empty range.
 * Output: records in brutus_fit_batch's layout, dense (d_rec_slot[r] = r), ascending model
 * index per star, starting at row `rec_base` of the caller's buffers; d_rec_off (nstar + 1)
 * entries are absolute rows (d_rec_off[0] = rec_base), so a batch can be cut in several
 * calls into one set of buffers: pass the previous call's h_counts[1] as rec_base and
 * d_rec_off advanced by that call's nstar.
 * h_counts (host, 2 x int64): [0] models selected by this call, [1] rows needed = rec_base +
 * [0].  BRUTUS_ENOMEM if [1] > capacity: nothing has been written to the planes or the
 * record buffers then (d_rec_off excepted), repeat the call with buffers of at least [1]
 * rows (rows below rec_base carried over by the caller).
 * BRUTUS_EINVAL: nstar outside [1, BRUTUS_MAX_BATCH], next < 0, next > 0 with a NULL
 * d_ext_labels / d_ext_par, wt_thresh not positive and finite. */
size_t brutus_cut_workspace_bytes(int64_t nmodel, int nstar);
int brutus_cut_batch(int64_t nmodel, int nstar, double *d_lnl, const double *d_chi2,
                     const double *d_scale, const double *d_av, const double *d_rv,
                     const double *d_icov, const double *d_parallax,
                     const double *d_parallax_err, int has_parallax, int next,
                     const double *d_ext_labels, const double *d_ext_par, double wt_thresh,
                     void *d_workspace, size_t workspace_bytes, int64_t capacity,
                     int64_t rec_base, int32_t *d_rec_idx, int32_t *d_rec_slot,
                     double *d_rec_vals, int64_t *d_rec_off, int64_t *h_counts, void *stream);

/* ---- lnpost on the device ------------------------------------------------------
 * Everything of fitting.lnpost after the first cut (fitting.py:1000-1107) and
 * the resampling tail of BruteForce._fit (fitting.py:2021-2061), for the
 * built-in priors: static lnprior + the Galactic model of pdf.gal_lnprior
 * (pdf.py:476-749; Galactocentric frame passed in, see frame_mat) + the parallax
 * likelihood.  Random numbers follow brutus_amd/rng.py (PhiloxRandomState:
 * Philox4x32-7; 53-bit uniforms; normals by a 1024-layer ziggurat, two per call):
 * normal j / uniform q are functions of (seed, j) / (seed, q), so the result is
 * what the reference produces when it is handed that object as `rstate`.
 *
 * Input = the device-resident indexed records brutus_fit_batch emitted (d_sel_idx = its
 * d_rec_idx, d_rec_slot, d_sel_vals = d_rec_vals, d_sel_off = d_rec_off, same capacity).  Output per
 * object s and draw q < ndraws:
 *   d_out_idx  (nstar, ndraws) i32      resampled model index
 *   d_out_vals (nstar, ndraws, 17) f64  scale, av, rv, cov_sar[9], lnprob,
 *                                       dist, red, dred, logwt
 *   h_star_out (nstar, 4) f64 (host)    levid, chi2min, sum of weights, Nsel
 *   h_flags    (nstar,) i32 (host)      0; an object with more than nsel_max
 *                                       survivors of the second cut is clipped to
 *                                       the nsel_max best, best first, by a device
 *                                       radix sort (fitting.py:1029-1036); a
 *                                       non-zero flag asks the caller to redo that
 *                                       object on the host (not used at present)
 *   h_nbase (nstar + 1,) u64 (host, optional)  normal-stream position at which
 *                                       each object starts; [nstar] = after the batch
 * Object s consumes 3*nmc*min(Nsel_s, nsel_max) normals starting where object
 * s-1 stopped (first at normal_base) and uniforms
 * [uniform_base + s*K, uniform_base + (s+1)*K), K = ndraws * (1 + return_distreds). */
typedef struct brutus_post_params {
    int32_t nmc, ndraws, return_distreds, has_feh, has_loga;
    int32_t per_object;   /* 1: object s draws from its own stream keyed
                             seed + object0 + s, positions from 0 (order- and
                             sharding-independent); 0: one shared stream */
    double wt_thresh, avlim[2], rvlim[2];
    int64_t nsel_max, object0;
    uint64_t seed, normal_base, uniform_base;
    double R_solar, Z_solar, R_thin, Z_thin, Rs_thin, R_thick, Z_thick, f_thick, Rs_thick;
    double Rs_halo, q_halo_ctr, q_halo_inf, r_q_halo, eta_halo, f_halo;
    double feh_mean[3], feh_sigma[3];
    double age_mean[3], age_sigma[3], age_lnnorm[3], min_age, max_age;
    /* Galactic -> Galactocentric frame of the prior (reference pdf.py:631-635 goes through
     * astropy's `Galactocentric`): x_gc [kpc] = frame_mat (row-major 3x3) @ d (cos b cos l,
     * cos b sin l, sin b) + frame_off; R = hypot(x, y), Z = z.  brutus_amd/galprior.py
     * (`astropy_frame`, `simple_frame`) builds the two frames the host knows. */
    double frame_mat[9], frame_off[3];
} brutus_post_params;

size_t brutus_post_workspace_bytes(int nstar, int64_t capacity, int nmc);
int brutus_post_batch(int nstar, int64_t capacity, const int32_t *d_sel_idx, const int32_t *d_rec_slot,
                      const double *d_sel_vals, const int64_t *d_sel_off,
                      const double *d_lnprior, const double *d_feh,
                      const double *d_loga, const double *d_coords,
                      const double *d_parallax, const double *d_parallax_err,
                      const brutus_post_params *params, void *d_workspace,
                      size_t workspace_bytes, int32_t *d_out_idx,
                      double *d_out_vals, double *h_star_out, int32_t *h_flags,
                      uint64_t *h_nbase, void *stream);

/* The same with NUMPY'S OWN random stream (legacy `numpy.random.RandomState`: MT19937,
 * polar Box-Muller with the cached second deviate, `choice` = searchsorted of
 * random_sample), i.e. what the reference consumes when `rstate` is a RandomState or
 * None (fitting.py:937-944, utils.py:892-905, fitting.py:2037-2053).  h_states holds
 * `nstream` generator states in numpy's representation, 628 words each:
 * key[624], pos, has_gauss, cached_gaussian (2 words, little endian double) --
 * `RandomState.get_state()`; they are advanced in place, so `set_state` makes the
 * caller's generator continue exactly where the reference's would.
 *   nstream == 1     one stream serves the objects in order (the reference's semantics);
 *                    a stream is sequential by nature: one workgroup walks it
 *   nstream == nstar object s has its own stream (per-object seeds: sharded runs)
 * d_zbuf (zbuf_doubles float64) receives the normals of a group of objects; an object
 * needs 3 * nmc * Nsel + 3 doubles; BRUTUS_ENOMEM if a single object does not fit.  The
 * first eighth of the buffer is scratch of the stream walk.  When all objects of the call
 * fit as one group, nmc <= 64 and the rest of the buffer also holds 16 bytes per generated
 * slot (about 1.3 x the flat normals), the stream is walked once: the accepted candidates'
 * normals stay where the walk produced them and the consumers read them through per-object
 * segment lists; otherwise a second walk writes the flat array.  Same results either way. */
int brutus_post_batch_numpy(int nstar, int64_t capacity, const int32_t *d_sel_idx, const int32_t *d_rec_slot,
                            const double *d_sel_vals, const int64_t *d_sel_off,
                            const double *d_lnprior, const double *d_feh,
                            const double *d_loga, const double *d_coords,
                            const double *d_parallax, const double *d_parallax_err,
                            const brutus_post_params *params, void *d_workspace,
                            size_t workspace_bytes, int32_t *d_out_idx,
                            double *d_out_vals, double *h_star_out, int32_t *h_flags,
                            int nstream, uint32_t *h_states, double *d_zbuf,
                            size_t zbuf_doubles, void *stream);

/* The same call in two halves, so that a caller can overlap them across batches: the
 * generator state of a numpy stream is final once the stream has been walked, before
 * the Monte Carlo integral that consumes the normals.  phase 1 = first and second cut,
 * covariances, stream walk (h_states advanced; normals and uniforms stay in d_zbuf /
 * the workspace; fails with BRUTUS_ENOMEM if the objects do not fit d_zbuf as ONE group
 * -- use the whole-call form then); phase 2 = Monte Carlo integral, evidence, draws,
 * outputs, with the SAME arguments, workspace and buffer, on any stream / thread, after
 * phase 1 returned.  phase 0 = brutus_post_batch_numpy. */
int brutus_post_batch_numpy_phase(int nstar, int64_t capacity, const int32_t *d_sel_idx, const int32_t *d_rec_slot,
                                  const double *d_sel_vals, const int64_t *d_sel_off,
                                  const double *d_lnprior, const double *d_feh, const double *d_loga,
                                  const double *d_coords, const double *d_parallax,
                                  const double *d_parallax_err, const brutus_post_params *params,
                                  void *d_workspace, size_t workspace_bytes, int32_t *d_out_idx,
                                  double *d_out_vals, double *h_star_out, int32_t *h_flags,
                                  int nstream, uint32_t *h_states, double *d_zbuf,
                                  size_t zbuf_doubles, int phase, void *stream);

/* Scheduling hook for callers that pipeline the two phases: `fn(arg)` is called once, on the
 * calling thread, from inside the NEXT brutus_post_batch_numpy[_phase] call of this thread,
 * as soon as the jump-ahead windows of its stream walk are complete (the call's stream is
 * drained first), at the latest before that call returns or fails after its walk.  The
 * jump-ahead kernels need whole compute units (125 KB of LDS per workgroup) and starve
 * behind a long kernel of another stream: a caller holds back phase 2 of the previous batch
 * until the hook fires, and the two then overlap where they can (stream walk: LDS-bound,
 * Monte Carlo integral: float64-issue-bound).  fn == NULL clears a pending hook. */
int brutus_post_set_after_jump(void (*fn)(void *), void *arg);

/* Line-of-sight dust prior for the NEXT brutus_post_batch / brutus_post_batch_numpy call
 * of the calling thread (one-shot): the reference's `dust_lnprior` (pdf.py:752-840,
 * Gaussian in Av around the profile interpolated at the distance) with the profile of every
 * object's sightline supplied by the caller instead of the Bayestar map:
 *   d_los (nstar, 3, nd) f64: dist [kpc], Av_mean, Av_err;  d_ok (nstar,) i32: 0 = no
 *   coverage (flat prior, like the reference).  Applied at the MLE point (fitting.py:1009-
 *   1010) and to every Monte Carlo sample (fitting.py:1084-1085). */
int brutus_post_set_dust(const double *d_los, const int32_t *d_ok, int nd,
                         double offset, double scale, double smooth, double scatter);

/* Tabulated distance prior for the NEXT brutus_post_batch / brutus_post_batch_numpy /
 * brutus_post_batch_numpy_phase call of the calling thread (one-shot, like
 * brutus_post_set_dust: set it before every call and every retry; a phase-2 call reads it too,
 * so set the same table before phase 1 and before phase 2):
 *   d_tab (nstar, 2, nd) f64: dist [kpc] (strictly increasing), ln prior at those distances,
 *   one table per object; interpolated like numpy.interp, end values outside the table.
 *   replace_gal == 0: the table multiplies the Galactic prior of brutus_post_params;
 *   replace_gal != 0: it replaces it (no density, no d^2 volume factor, no label terms).
 * Applied at the MLE point and to every Monte Carlo sample.  d_tab == NULL clears a pending
 * table.  BRUTUS_EINVAL "bad distance table" unless 2 <= nd <= 4096 (checked before any HIP
 * call).  An additive entry point: BRUTUS_ABI_VERSION stays. */
int brutus_post_set_dist_table(const double *d_tab, int nd, int replace_gal);

/* Jump-ahead polynomials of MT19937 (brutus_amd/mt_jump.npz, made and checked against
 * numpy by tools/gen_mt_jump.py): h_polys = uint32 (npoly, 624), x^(stride - 1) mod phi
 * for stride0 = 2 096 640 words and 128 * stride0 * 2^r, r = 0 .. npoly - 2.  With them
 * loaded one stream is walked by many workgroups (sub-streams of stride0 words, their
 * start windows from a doubling tree of jumps); without them by one. */
int brutus_set_mt_jump(const uint32_t *h_polys, int npoly, int64_t stride0,
                       int64_t stride1);

/* ---- cluster mode ------------------------------------------------------------
 * Hot block of cluster.isochrone_loglike (cluster.py:336-414): for nobj objects
 * and npts isochrone points (all secondary-mass-fraction slices concatenated,
 * masked points removed by the caller),
 *   d_pts_flux (npts, nfilt) f64  model fluxes 10^(-0.4 cmd_sed), NaN = no model
 *   d_pts_lnw  (npts,)       f64  ln(grad_mini) + ln(grad_smf)   (cluster.py:397-403)
 *   d_phot, d_ivar (nobj, nfilt)  offset-scaled fluxes and 1/err^2 (0 for missing bands)
 *   d_chi2_p, d_lnorm (nobj,)     parallax chi2; ln-normalisation (dim_prior == 0)
 *   d_ndim (nobj,) i32            phot_n, the chi-square degrees of freedom
 * writes d_lnl (nobj,) = logsumexp over points of (lnl + lnw), i.e. the
 * `lnl` of cluster.py:407 before the outlier mixture. */
/* Isochrone points of all secondary-mass-fraction slices from the plug-in's apparent
 * magnitudes (reference cluster.py:346-366, the `10**(-0.4 * seds)` and the
 * any-finite-band test of every slice): d_mags (nrow, nfilt) float64 and d_lnw_in (nrow)
 * = ln(d mini) + ln(d smf) over the whole table, d_src (npts) int32 the rows the host
 * kept, in order (NULL: all nrow = npts rows) -> d_pts_flux (npts, nfilt), d_pts_lnw
 * (npts), the inputs of brutus_cluster_lnl; a kept row without a finite band gets
 * weight -inf. */
int brutus_cluster_points(int64_t npts, int nfilt, const int32_t *d_src, const double *d_mags,
                          const double *d_lnw_in, double *d_pts_flux, double *d_pts_lnw,
                          void *stream);
/* The same where all slices share one initial-mass grid (the reference's isochrones do:
 * `mini` depends on EEP, [Fe/H] and age, not on the mass fraction): the weight of table row
 * r is d_lnw_eep[r % neep] + d_lnw_smf[r / neep] = ln(d mini) + ln(d smf) (-inf for an EEP
 * the caller drops), formed here instead of in a host array of nrow values per call. */
int brutus_cluster_points_grid(int64_t npts, int nfilt, int neep, const int32_t *d_src,
                               const double *d_mags, const double *d_lnw_eep,
                               const double *d_lnw_smf, double *d_pts_flux,
                               double *d_pts_lnw, void *stream);
size_t brutus_cluster_workspace_bytes(int nobj);
int brutus_cluster_lnl(int nobj, int nfilt, int npts, const double *d_pts_flux,
                       const double *d_pts_lnw, const double *d_phot,
                       const double *d_ivar, const double *d_chi2_p,
                       const double *d_lnorm, const int32_t *d_ndim,
                       int dim_prior, void *d_workspace, size_t workspace_bytes,
                       double *d_lnl, void *stream);
/* The same in pieces, for a caller that gets the isochrone points a few slices at a time
 * (the reference asks its plug-in once per secondary-mass-fraction slice, cluster.py:346-366)
 * and wants the device to work on one piece while the host prepares the next: the sum over
 * points is kept as brutus_cluster_chunks() partial (max, sum) pairs per object in the
 * workspace; `_part` fills the chunks [chunk_lo, chunk_lo + chunk_n) from ITS npts points
 * (npts = 0: they hold "no point"), `_merge` folds the first nchunk chunks into d_lnl.
 * brutus_cluster_lnl = one `_part` over all chunks + `_merge`.  Every chunk below nchunk
 * must have been filled by a `_part` call on the same stream. */
int brutus_cluster_chunks(void);
int brutus_cluster_lnl_part(int nobj, int nfilt, int npts, const double *d_pts_flux,
                            const double *d_pts_lnw, const double *d_phot,
                            const double *d_ivar, const double *d_chi2_p,
                            const double *d_lnorm, const int32_t *d_ndim, int dim_prior,
                            void *d_workspace, size_t workspace_bytes, int chunk_lo,
                            int chunk_n, void *stream);
/* `_part` straight from the plug-in's magnitude table: the inputs of
 * brutus_cluster_points_grid (kept rows d_src (npts), d_mags (nrow, nfilt), the two factors of
 * the ln-weight, neep) instead of a flux table -- the kernel forms fluxes and weights of its
 * own sub-slices, one launch and one table less per piece. */
int brutus_cluster_lnl_part_mags(int nobj, int nfilt, int npts, int neep, const int32_t *d_src,
                                 const double *d_mags, const double *d_lnw_eep,
                                 const double *d_lnw_smf, const double *d_phot,
                                 const double *d_ivar, const double *d_chi2_p,
                                 const double *d_lnorm, const int32_t *d_ndim, int dim_prior,
                                 void *d_workspace, size_t workspace_bytes, int chunk_lo,
                                 int chunk_n, void *stream);
int brutus_cluster_lnl_merge(int nobj, int nchunk, void *d_workspace, size_t workspace_bytes,
                             double *d_lnl, void *stream);
/* Outlier mixture and total of cluster.py:410-414 on the device: d_lnl_mix (nobj) =
 * logaddexp(d_lnl + ln_fin, d_lnl_outlier + ln_fout) (numpy's logaddexp, NaN and infinities
 * included) and d_lnl_tot (1) = their sum in a fixed order (the same bits on every run). */
int brutus_cluster_mix(int nobj, const double *d_lnl, const double *d_lnl_outlier, double ln_fin,
                       double ln_fout, double *d_lnl_mix, double *d_lnl_tot, void *stream);

/* ---- seds.Isochrone (reference seds.py:1081-1502; FastNN evaluation seds.py:960-1078) ----
 * MIST isochrones + one small network per filter, for the plug-in of the cluster likelihood:
 * one call makes the magnitudes of every (mass-fraction slice, EEP, filter) on the device.
 * Float64.  Table and axes as the reference holds them AFTER build_interpolator (holes
 * filled, a single [alpha/Fe] padded to two nodes). */
#define BRUTUS_ISO_APPLY_CORR 1  /* empirical Teff / radius corrections (seds.py:1327-1356)     */
#define BRUTUS_ISO_EEP2_GIVEN 2  /* d_eep2 holds np.interp's secondaries' EEPs (before the cuts) */
#define BRUTUS_ISO_PRED_ONLY 4   /* stop after the primaries' predictions (d_prim, d_mini)      */
typedef struct {
    int32_t nfeh, nafe, nloga, neep_tab, npred;   /* table (nfeh, nafe, nloga, neep_tab, npred)  */
    int32_t idx_mini, idx_logl, idx_logt, idx_logg, idx_feh_surf, idx_afe_surf; /* its columns   */
    int32_t nfilt, h1, h2;                        /* networks 6 -> h1 -> h2 -> 1, h1 <= 64       */
    int32_t neep, nsmf, flags;                    /* the query; BRUTUS_ISO_* bits                */
    double feh, afe, loga, av, rv, dist;          /* dist in pc                                  */
    double mini_bound, eep_binary_max;
    double corr[4];                               /* dtdm, drdm, msto_smooth, feh_scale          */
} brutus_iso_params;
size_t brutus_iso_workspace_bytes(int neep, int nsmf, int nfilt);   /* 0: bad dimensions */
/*   d_table   (nfeh, nafe, nloga, neep_tab, npred)       d_axes  feh | afe | loga | eep nodes
 *   d_weights per filter w1 (h1, 6) | b1 (h1) | w2 (h2, h1) | b2 (h2) | w3 (h2) | b3 (1)
 *   d_xmin, d_xmax (6)  bounds of the networks' inputs [Teff, logg, feh_surf, afe_surf, av, rv]
 *   d_eep (neep), d_smf (nsmf)
 * writes d_mags (nsmf, neep, nfilt) apparent magnitudes, combined as seds.py:1467-1496 does
 * (NaN rows where the reference has them); d_prim (neep, npred) and d_sec (nsmf, neep, npred),
 * the predictions of the two components (d_sec NaN outside 0 < smf < 1); d_mini (neep);
 * d_eep2 (nsmf, neep) the secondaries' EEPs after the cuts; d_status int32[2]: [0] = 1 if the
 * finite initial masses are not strictly increasing with EEP -- the device's bisection is
 * then not np.interp, and the caller repeats the call with np.interp's values in d_eep2 and
 * BRUTUS_ISO_EEP2_GIVEN --, [1] the number of finite primaries.
 * BRUTUS_EINVAL (before any HIP call): an axis with fewer than 2 nodes, npred outside
 * [1, 16], a column index outside the table, neep / nsmf / nfilt < 1, h1 outside [1, 64] or
 * more than 64 KiB of weights per filter, a NULL pointer.  BRUTUS_ENOMEM: workspace. */
int brutus_iso_seds_grid(const brutus_iso_params *p, const double *d_table, const double *d_axes,
                         const double *d_weights, const double *d_xmin, const double *d_xmax,
                         const double *d_eep, const double *d_smf, double *d_mags, double *d_prim,
                         double *d_sec, double *d_mini, double *d_eep2, int32_t *d_status,
                         void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- seds.MISTtracks / seds.SEDmaker (reference seds.py:49-857; FastNN seds.py:960-1078) ----
 * EEP tracks + one small network per filter: predictions at labels (mini, eep, feh, afe),
 * the SED of a single star or an unresolved binary (get_sed), and the model grid that
 * BruteForce fits against (make_grid): per model and filter the magnitude at (av, rv) and the
 * linear fits of the magnitudes in Av and Rv.  Float64.  Table and axes as the reference holds
 * them AFTER build_interpolator (a single [alpha/Fe] padded to two nodes, holes NaN). */
#define BRUTUS_SED_APPLY_CORR 1  /* empirical Teff / radius corrections at the label mass (seds.py:349-384) */
#define BRUTUS_SED_EEP2_GIVEN 2  /* d_eep2_in holds the secondaries' EEPs; nothing is solved              */
#define BRUTUS_SED_PRED_ONLY 4   /* stop after the primaries' predictions (d_out_param)                   */
#define BRUTUS_SED_FIT 8         /* make_grid: (sed, seda, sedr) per filter; without it get_sed: one value */
#define BRUTUS_SED_SCAN 16       /* loga does not rise along every track: the root nearest the primary's EEP */
#define BRUTUS_SED_EEP_ONLY 32   /* get_eep: d_out_eep2 alone, for the age loga_target at the label's afe  */
typedef struct {
    int32_t nmini, neep_tab, nfeh, nafe, npred;   /* table (nmini, neep_tab, nfeh, nafe, npred)   */
    int32_t idx_loga, idx_logl, idx_logt, idx_logg, idx_feh_surf, idx_afe_surf; /* its columns    */
    int32_t nfilt, h1, h2;                        /* networks 6 -> h1 -> h2 -> 1, h1 <= 64        */
    int32_t nmodel, nav, nrv, flags;              /* the query; BRUTUS_SED_* bits                 */
    double av, rv, dist;                          /* the reference point; dist in pc              */
    double loga_max, eep_binary_max, mini_min;    /* the cuts; mini_min binds the secondary alone */
    double tol, loga_target;                      /* get_eep                                      */
    double corr[4];                               /* dtdm, drdm, msto_smooth, feh_scale           */
} brutus_sed_params;
size_t brutus_sed_workspace_bytes(int nmodel, int nfilt, int nfit);   /* 0: bad dimensions */
/*   d_table   (nmini, neep_tab, nfeh, nafe, npred)       d_axes  mini | eep | feh | afe nodes
 *   d_weights, d_xmin, d_xmax as brutus_iso_seds_grid takes them
 *   d_labels (nmodel, 5)   mini, eep, feh, afe, smf of every model
 *   d_eep2_in (nmodel) or NULL   the secondaries' EEPs (BRUTUS_SED_EEP2_GIVEN)
 *   d_fitcoef (2, nrv, nav)   seda = sum fitcoef[0] * mag, sedr = sum fitcoef[1] * mag over the fit
 *                             points (av[a], rv[r]): the two weighted straight-line fits of
 *                             seds.py:828-831 as linear functionals; d_av (nav), d_rv (nrv)
 * writes d_out_sed (nmodel, nfilt, 3) = (mag at (av, rv), seda, sedr) with BRUTUS_SED_FIT, else
 * (nmodel, nfilt) magnitudes; d_out_param, d_out_param2 (nmodel, npred) the predictions of the
 * two components (param2 NaN without a secondary); d_out_eep2 (nmodel) the secondaries' EEPs,
 * given or solved: loga along a track is piecewise linear in EEP, so the root is exact (a cell
 * with a NaN node holds none; a target outside the range of the finite nodes takes the nearer
 * finite end node if its squared residual is below tol); d_out_sel (nmodel) 1 where the magnitudes at (av, rv) and the
 * primary's predictions hold no NaN -- with BRUTUS_SED_FIT the other rows of d_out_sed are NaN
 * throughout.  d_status is reserved and may be NULL.
 * BRUTUS_EINVAL (before any HIP call): an axis with fewer than 2 nodes, npred outside [1, 16],
 * a column index outside the table, nmodel / nfilt < 1, nav * nrv outside [4, 256], h1 outside
 * [1, 64] or more than 64 KiB of LDS per filter, a NULL pointer.  BRUTUS_ENOMEM: workspace. */
int brutus_sed_grid(const brutus_sed_params *p, const double *d_table, const double *d_axes,
                    const double *d_weights, const double *d_xmin, const double *d_xmax,
                    const double *d_labels, const double *d_eep2_in, const double *d_fitcoef,
                    const double *d_av, const double *d_rv, double *d_out_sed, double *d_out_param,
                    double *d_out_param2, double *d_out_eep2, uint8_t *d_out_sel, int32_t *d_status,
                    void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- utils.photometric_offsets (reference utils.py:1218-1400) ------------------------
 * The per-band bootstrap of model / data flux ratios over the resampled fits of many
 * objects.  The caller keeps numpy's random stream and the final median / std over the
 * rounds; these two calls replace the reference's get_seds + phot_loglike + per-object
 * `choice` loop.
 *
 * brutus_offsets_weights: for every object o and resampled draw k
 *   d_models (nmodel, nfilt, 3) f32   the grid as utils.load_models returns it
 *   d_idxs, d_reds, d_dreds, d_dists (nobj, nsamps)   the fit's draws (negative idx wraps)
 *   d_phot, d_err (nobj, nfilt) f64, d_mask (nobj, nfilt) u8, d_weights (nobj, nsamps)
 *   d_old_offsets (nfilt), d_mask_fit (nfilt) u8
 *   d_use (nfilt, nobj) u8            the objects that enter band b (utils.py:1337-1350)
 * writes d_flux (nfilt, nobj, nsamps) = 10^(-0.4 sed) / dist^2 (utils.py:1327-1331) and
 * d_cdf (nfilt, nobj, nsamps) = cumulative normalised weights of the draws: leave-one-band-
 * out likelihood x weights where mask_fit[b], plain weights otherwise (utils.py:1355-1372);
 * rows with d_use == 0 are left untouched. */
int brutus_offsets_weights(int nobj, int nsamps, int nfilt, int64_t nmodel, const float *d_models,
                           const int64_t *d_idxs, const double *d_reds, const double *d_dreds,
                           const double *d_dists, const double *d_phot, const double *d_err,
                           const uint8_t *d_mask, const double *d_weights,
                           const double *d_old_offsets, const uint8_t *d_use,
                           const uint8_t *d_mask_fit, int dim_prior, double *d_flux, double *d_cdf,
                           void *stream);
/* brutus_offsets_bootstrap: the nmc bootstrap rounds of ONE band (utils.py:1374-1387):
 *   d_subset (n) i32   the objects of this band, d_cdf_obj (n) their cumulative weights
 *   d_u (nmc, 2, n)    the 2 n uniforms of every round in numpy's order: the n of
 *                      `choice(n, size=n, p=wt_obj)`, then one per `choice(Nsamps, p=wt[i])`
 * both `choice`s are numpy's legacy searchsorted(cdf, u, 'right'); writes d_meds (nmc) =
 * np.median of the round's model / data ratios.  0 bytes from the size query = bad sizes. */
size_t brutus_offsets_workspace_bytes(int n, int nmc);
int brutus_offsets_bootstrap(int band, int nobj, int nsamps, int nfilt, int n, int nmc,
                             const int32_t *d_subset, const double *d_cdf_obj, const double *d_u,
                             const double *d_flux, const double *d_cdf, const double *d_phot,
                             void *d_workspace, size_t workspace_bytes, double *d_meds,
                             void *stream);

/* ---- binned (distance, reddening) posteriors: pdf.bin_pdfs_distred on the device ----------
 * One call bins, smooths and (cdf) accumulates the posteriors of nobj objects into
 * d_out (nobj, nx, ny) f32, row-major, y fastest.  Additive entry points: BRUTUS_ABI_VERSION
 * stays.
 *   nx, ny         bins along the distance axis / the reddening axis
 *   dist_type      what the distance axis holds: 0 scale 1/d^2, 1 parallax 1/d, 2 distance d,
 *                  3 distance modulus 5 log10(d) + 10
 *   ebv            != 0: the reddening axis holds Av / Rv
 *   cdf            != 0: cumulative sum along the distance axis (float32, sequential)
 *   nr, prior_mode, max_attempts, avlim, rvlim, seed, object0: the regenerating form only.
 *                  prior_mode 0: Galactic prior, 1: the distance table replaces it, 2: the
 *                  table multiplies it.  1 <= max_attempts <= 65536 bounds the rejection loop.
 *   ysigma_bins    width of the Gaussian along the reddening axis, in bins (>= 0, finite)
 * Binning is numpy.histogram2d's with explicit edges (d_xedges (nx + 1), d_yedges (ny + 1) f64,
 * increasing; the last bin is closed on the right; values outside and NaN are dropped),
 * divided by nsamps and rounded once to float32; smoothing is scipy.ndimage.gaussian_filter's
 * (radius int(4 sigma + 0.5), boundary `reflect`, float64 accumulation, float32 between the
 * axes, an axis with sigma <= 1e-15 skipped) with the per-object width d_xsigma_bins (nobj) f64
 * along the distance axis.  A radius above 2047 bins is refused (y) / clamped (x: the caller
 * checks the array it computed).  Sums are integers (counts; weights in 2^-50 fixed point), so
 * the result does not depend on the order the device meets the draws in.
 * Limits: 1 <= nobj <= 65535, 1 <= nx, ny <= 65536, nx ny <= 2^28, 1 <= nsamps <= 4096,
 * 1 <= nr <= 65536, nsamps nr <= 2^24; checked, like every pointer, before any HIP call. */
typedef struct brutus_binpdf_params {
    int32_t nx, ny, dist_type, ebv, cdf, nr, prior_mode, max_attempts;
    double avlim[2], rvlim[2];
    double ysigma_bins;
    uint64_t seed;
    int64_t object0;
} brutus_binpdf_params;

/* Bytes of d_workspace for a call of either form (nr = 0: the saved-draws form); 0 = bad sizes. */
size_t brutus_binpdf_workspace_bytes(int nobj, int nx, int ny, int nsamps, int nr);

/* Saved draws: d_dist, d_red, d_dred (nobj, nsamps) f64 = distance [kpc], Av, Rv of every draw
 * (d_dred may be NULL unless params->ebv). */
int brutus_binpdf_saved(int nobj, int nsamps, const double *d_dist, const double *d_red,
                        const double *d_dred, const double *d_xedges, const double *d_yedges,
                        const double *d_xsigma_bins, const brutus_binpdf_params *params,
                        float *d_out, void *d_workspace, size_t workspace_bytes, void *stream);

/* Regenerated draws: around every draw (d_scale, d_av, d_rv (nobj, nsamps) f64 with covariance
 * d_cov (nobj, nsamps, 9) f64, row-major 3x3) params->nr realisations are drawn from the
 * truncated normal (scale >= 0, avlim, rvlim) with the indexed stream of
 * brutus_amd/utils.py `draw_sar_indexed` (key seed + object0 + object; normals
 * 3 ((t nsamps + k) nr + r) + c of draw k, realisation r, attempt t), weighted by the
 * distance prior at d = 1 / sqrt(scale) and the parallax likelihood (d_par, d_parerr (nobj),
 * NaN = none; either may be NULL), normalised per draw, and binned with those weights.
 *   d_coord (nobj, 2) f64 Galactic l, b [deg]; gal: the Galactic prior's constants (label
 *   terms are not evaluated; required in every mode); d_dtab (nobj, 2, nd) f64 the distance
 *   tables as for brutus_post_set_dist_table, NULL with prior_mode 0.
 *   d_status (nobj, 3) i32 out: [0] != 0: a covariance of the object is not positive definite
 *   (its plane is not meaningful); [1] slots that exhausted max_attempts; [2] realisations
 *   whose ln prior was not finite.  Slots of [1] and [2] carry weight 0. */
int brutus_binpdf_regen(int nobj, int nsamps, const double *d_scale, const double *d_av,
                        const double *d_rv, const double *d_cov, const double *d_par,
                        const double *d_parerr, const double *d_coord,
                        const brutus_post_params *gal, const double *d_dtab, int nd,
                        const double *d_xedges, const double *d_yedges,
                        const double *d_xsigma_bins, const brutus_binpdf_params *params,
                        int32_t *d_status, float *d_out, void *d_workspace,
                        size_t workspace_bytes, void *stream);

/* ---- line-of-sight cloud likelihood (reference los.py:119-248) ----------------------------
 * ln L of ntheta cumulative-reddening profiles of nclouds clouds, given the (distance, reddening)
 * draws of the nobj objects of one sightline.  Additive entry points: BRUTUS_ABI_VERSION stays.
 *   d_dsamps, d_rsamps (ndraws, nobj) f64, DRAW-major: the draws that enter (the caller has
 *                  sub-sampled them); ndraws is also the divisor of every object's sum
 *   d_template (nobj) f64 or NULL: cloud reddenings are multiples of the object's value
 *   d_theta (ntheta, 4 + 2 nclouds) f64: [pb, s0, s, fred, d1, r1, d2, r2, ...] per row, cloud
 *                  distances ascending (the caller checks; rows are independent)
 *   kernel         0 Gaussian, 1 Lorentzian, 2 top hat, of width s0 area (foreground) / s area
 *                  with area = rlims[1] - rlims[0] > 0, finite
 *   additive_foreground != 0: fred is added to every later bin's mean (after the template)
 *   d_loglike (ntheta) f64 out; d_terms (ntheta, nobj) f64 out or NULL: the per-object values
 *                  after the outlier mixture, whose sum is d_loglike
 * A draw belongs to the bin whose edges [0, d1, ..., dn, 1e10] hold it (lower edge included);
 * any other draw (NaN too) has weight zero; a NaN reddening makes the object's term NaN for the
 * Gaussian and the Lorentzian and has weight zero for the top hat, as in the reference.
 * Sums run in a fixed order: a row's value does not depend on the rest of the batch.
 * Limits: 1 <= nobj <= 2^22, 1 <= ndraws <= 4096, 0 <= nclouds <= 32, 1 <= ntheta <= 65535;
 * checked, like every pointer, before any HIP call.  BRUTUS_ENOMEM: workspace. */
#define BRUTUS_LOS_MAX_OBJ (1 << 22)
#define BRUTUS_LOS_MAX_DRAWS 4096
#define BRUTUS_LOS_MAX_CLOUDS 32
#define BRUTUS_LOS_MAX_THETA 65535
typedef struct brutus_los_params {
    int32_t kernel, additive_foreground;
    double rlims[2];
} brutus_los_params;
size_t brutus_los_workspace_bytes(int nobj, int ntheta);   /* 0: bad sizes */
int brutus_los_loglike(int nobj, int ndraws, const double *d_dsamps, const double *d_rsamps,
                       const double *d_template, int ntheta, int nclouds, const double *d_theta,
                       const brutus_los_params *params, double *d_loglike, double *d_terms,
                       void *d_workspace, size_t workspace_bytes, void *stream);


/* Name and average duration (HIP events on `stream`) of the kernels launched
 * by the last *_batch call; used by bench.py for the roofline line. */
int brutus_last_timing(int *n_entries, const char **names, float *ms,
                       int max_entries);
void brutus_enable_timing(int on);

/* ---- K thetas per call: seds.Isochrone and the cluster likelihood in batches ---- */
#include "brutus_amd_batch.h"

/* ---- Bayestar 3-D dust map: nested HEALPix pixels and the map query (reference dust.py) ---- */
#include "brutus_amd_dust.h"

/* ---- per-object posterior summaries: quantiles of the saved draws (reference plotting.py) ---- */
#include "brutus_amd_summary.h"

/* ---- posterior-predictive check: the draws' model SEDs and their quantiles per band ---- */
#include "brutus_amd_predictive.h"

/* ---- photometric-offset residual maps: leave-one-band-out residuals, histograms, medians ---- */
#include "brutus_amd_offdiag.h"

/* ---- corner-plot marginals: per-object 1-D and 2-D histograms, smoothing, contour levels ---- */
#include "brutus_amd_corner.h"

/* ---- line-of-sight cloud likelihood of many sightlines per call (a ragged field of them) ---- */
#include "brutus_amd_los_field.h"

/* ---- fitting a field of sightlines: the LOS prior transform and the ensemble sampler's kernels ---- */
#include "brutus_amd_los_walk.h"

/* ---- a field's chains to its dust map: quantiles, reddening profile, moments and R-hat ---- */
#include "brutus_amd_los_chain.h"

#ifdef __cplusplus
}
#endif
#endif /* BRUTUS_AMD_H */
