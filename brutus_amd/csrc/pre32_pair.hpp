// pre32_pair.hpp -- what one (star, model) pair of the star-lane float32 proof passes computes,
// once for both of them: k_pre32s (pre32s_kernels.hpp, all-vector) and k_pre32m
// (pre32m_kernels.hpp, the band contractions on the matrix pipe).  The kernels differ in how a
// tile is staged, how the sweep's Gram sums over the bands are formed and how the two planes
// leave; from the sums on -- the Av / Rv steps, the running maxima, the MLE of the scale and the
// two statistics with their NaN and survivor-tag conventions -- a pair is the same code, and a
// fix to it has to reach both passes.  Everything here is inlined into the lane that owns the
// pair; nothing touches LDS or global memory.
// Units: av is c Av throughout, c = -0.4 log2(10) (pre32s_kernels.hpp, "Scaled magnitudes").
// Semantics to hold: as in pre32s_kernels.hpp.
#pragma once

#include "pre32_types.hpp"

namespace {

constexpr float PS_C10 = -1.32877123795494494f;      // c = -0.4 log2(10)
constexpr int PS_WM = F2_T * PS_TILE / 4;            // models per wave: a block of F2_T tiles over four waves

// v_max_f32 as the hardware defines it: a NaN operand yields the other one (fmaxf compiles to
// two canonicalising v_max per call on top)
__device__ __forceinline__ float vmaxf(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// ln x for a normal-range positive argument: v_log_f32 (log2, 1 ulp) times ln 2 -- __logf's
// denormal rescue and its extended-precision multiplication are ten more instructions, and the
// arguments here (chi2 above chi2_lo >= 0.5, variances) never need them
__device__ __forceinline__ float ln_pos(float x) { return 0.69314718055994531f * __builtin_amdgcn_logf(x); }
// LDS hand-over between the lanes of ONE wave (its instructions reach the LDS in order: no
// hardware wait is needed, but the compiler must not move the reads of other lanes' words
// across the writes, in either direction)
__device__ __forceinline__ void ps_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// A lane's running maxima over its models, in the order of part32's NV32 values per (block, star)
enum {
    MX_LW1 = 0,     // logwt after the first sweep: every model, step >= mtol_hi, step >= mtol_lo
    MX_LW2 = 3,     // the same three after the second sweep (general Rv only)
    MX_LNLP = 6,    // lnl_p~
    MX_LNPR = 7,    // lnprob~
    MX_NAN_LW = 8,  // 1 where a logwt came out NaN
    MX_NAN_PL = 9,  // 1 where a value of the two planes did
};

// The star's constants, resident in the lane for its whole run of models (the per-band arrays
// stay with the kernels: each keeps the ones its sums need)
struct PairStar {
    float S, rS, gbarC, DD2;
    bool has_par, sp_on;
    bool any_par, any_sp;         // wave-uniform: some lane of the wave has a parallax / a scale prior
    float eps4, chi2_lo;
    float par, par_hiv, sp_mean, sp_var, c0, c1;
    float avm, av_lo, av_hi;      // prior mean and limits of c Av
    float tol_hi, tol_lo;         // the step tolerances in units of c Av
    float lw_scale;
};

// Call with the whole wave: the two ballots are taken here.
// (the star by pointer, not by reference: a reference argument declares all of Star32 readable, the
// conditional loads below are then hoisted and merged, and of the register allocations that follow
// the one of k_pre32s<12, general> keeps four loop-invariant canonicalising v_max_f32 inside its
// loop over the models: + 1.2 % measured)
__device__ __forceinline__ PairStar pair_star(const Star32 *sp, const P32 &p) {
    PairStar c;
    c.S = sp->S, c.rS = __builtin_amdgcn_rcpf(sp->S), c.gbarC = PS_C10 * sp->gbar, c.DD2 = sp->DD2;
    c.has_par = sp->has_par != 0, c.sp_on = sp->sp_on != 0;
    // (a star float32 cannot represent: both limits at +inf turn every value into NaN)
    c.eps4 = sp->ok ? 4.f * sp->eps : INFINITY, c.chi2_lo = sp->ok ? sp->chi2_lo : INFINITY;
    c.par = c.has_par ? sp->par : 0.f, c.par_hiv = c.has_par ? 0.5f * sp->par_ivar : 0.f;
    c.sp_mean = sp->sp_mean, c.sp_var = sp->sp_var, c.c0 = sp->c0, c.c1 = sp->c1;
    c.any_par = __ballot(c.has_par) != 0ull, c.any_sp = __ballot(c.sp_on) != 0ull;
    // the Av solve in av' = c av (c < 0: the clamps trade places)
    c.avm = PS_C10 * p.av_mean, c.av_lo = PS_C10 * p.avmax, c.av_hi = PS_C10 * p.avmin;
    c.tol_hi = -PS_C10 * p.mtol_hi, c.tol_lo = -PS_C10 * p.mtol_lo;
    c.lw_scale = -0.5f / (PS_C10 * PS_C10);
    return c;
}

// One sweep's logwt into its three maxima mx[K .. K + 2] (every model; the models whose step st
// is still at least thr_hi / thr_lo) and into the NaN flag
template <int K>
__device__ __forceinline__ void pair_max(float (&mx)[NV32], float lw, float st, float thr_hi, float thr_lo) {
    const float NINF = -INFINITY;
    mx[K] = vmaxf(mx[K], lw);
    mx[K + 1] = vmaxf(mx[K + 1], st >= thr_hi ? lw : NINF);
    mx[K + 2] = vmaxf(mx[K + 2], st >= thr_lo ? lw : NINF);
    mx[MX_NAN_LW] = lw != lw ? 1.f : mx[MX_NAN_LW];
}

// Pinned Rv: the one Av step of fitting.py:176-204 from the prior mean, on the sums over the
// bands uR = sum w R, RR = sum w R^2, yR = sum w R y, uy = sum w y, yy = sum w y^2.  Returns c Av.
__device__ __forceinline__ float pair_av_step(float uR, float RR, float yR, float uy, float yy, float dbar,
                                              const PairStar &c, const P32 &p, float (&mx)[NV32]) {
    float av = c.avm;
    const float rs = uy - av * uR;
    const float ra = (yR - av * RR) + (c.avm - av) * p.av_ivar;
    const float a_den = RR + p.av_ivar;
    float dav = (c.S * ra - uR * rs) * __builtin_amdgcn_rcpf(c.S * a_den - uR * uR);
    dav = fminf(dav, c.av_hi - av);
    dav = fmaxf(dav, c.av_lo - av);
    av += dav;
    const float oc = (uy - av * uR) * c.rS;
    const float tt0 = dbar + oc;
    const float lw = c.lw_scale * ((yy - av * (2.f * yR - av * RR)) + c.S * (tt0 * tt0 - oc * oc));
    pair_max<MX_LW1>(mx, lw, fabsf(dav), c.tol_hi, c.tol_lo);
    return av;
}

// General Rv: one sweep of fitting.py:176-243 with av -> c av on the sums with R = a + rv b
// (ua = sum w a, ub = sum w b, aa, ab, bb likewise, ay = sum w a y, by, uy, yy): the Av half as
// in pair_av_step; in the Rv half every product av x (a y-free sum) carries one c and every
// product av x (a y sum) two, so its numerator and denominator are both c^2 times the
// reference's once the prior terms are scaled likewise: drv comes out unscaled.  Moves av and
// rv, returns logwt; st: the larger of the two steps, |dAv| back in magnitudes.
__device__ __forceinline__ float pair_sweep(float ua, float ub, float uy, float aa, float ab, float bb, float ay,
                                            float by, float yy, float dbar, const PairStar &c, const P32 &p,
                                            float &av, float &rv, float &st) {
    const float c2 = PS_C10 * PS_C10;
    const float uR = ua + rv * ub;
    const float RR = aa + rv * (2.f * ab + rv * bb);
    const float yR = ay + rv * by;
    float rs = uy - av * uR;
    const float ra = (yR - av * RR) + (c.avm - av) * p.av_ivar;
    const float a_den = RR + p.av_ivar;
    float dav = (c.S * ra - uR * rs) * __builtin_amdgcn_rcpf(c.S * a_den - uR * uR);
    dav = fminf(dav, c.av_hi - av);
    dav = fmaxf(dav, c.av_lo - av);
    av += dav;
    const float r_den = bb * av * av + c2 * p.rv_ivar;
    const float sr = ub * av;
    rs = uy - av * uR;
    const float bres = by - av * (ab + rv * bb);
    const float rr = av * bres + c2 * ((p.rv_mean - rv) * p.rv_ivar);
    float drv = (c.S * rr - sr * rs) * __builtin_amdgcn_rcpf(c.S * r_den - sr * sr);
    drv = fmaxf(drv, p.rvmin - rv);
    drv = fminf(drv, p.rvmax - rv);
    rv += drv;
    const float RR2 = aa + rv * (2.f * ab + rv * bb);
    const float yR2 = ay + rv * by;
    st = fmaxf(fabsf(dav) * (-1.f / PS_C10), fabsf(drv));
    const float uR2 = ua + rv * ub;
    const float oc = (uy - av * uR2) * c.rS;
    const float tt0 = dbar + oc;
    return c.lw_scale * ((yy - av * (2.f * yR2 - av * RR2)) + c.S * (tt0 * tt0 - oc * oc));
}

// The opening pass of the general kernels: two sweeps from the prior means (every star of the
// launch has kfix = 2), each with its own three maxima
__device__ __forceinline__ void pair_sweeps(float ua, float ub, float uy, float aa, float ab, float bb, float ay,
                                            float by, float yy, float dbar, const PairStar &c, const P32 &p,
                                            float &av, float &rv, float (&mx)[NV32]) {
    av = c.avm, rv = p.rv_mean;
    float st;
    const float lw1 = pair_sweep(ua, ub, uy, aa, ab, bb, ay, by, yy, dbar, c, p, av, rv, st);
    pair_max<MX_LW1>(mx, lw1, st, p.mtol_hi, p.mtol_lo);
    const float lw2 = pair_sweep(ua, ub, uy, aa, ab, bb, ay, by, yy, dbar, c, p, av, rv, st);
    pair_max<MX_LW2>(mx, lw2, st, p.mtol_hi, p.mtol_lo);
}

// What follows the sweeps: the MLE of the scale at (av, rv) and the two statistics, lnl_p~ (the
// cull statistic) and lnprob~ (the first-cut statistic), into their maxima too.  mcC, A, B: the
// model's row (B: dr per band, unused and of any length when Rv is pinned and A holds R).
template <int NB, bool RVF, int NBB>
__device__ __forceinline__ void pair_tail(const float (&mcC)[NB], const float (&A)[NB], const float (&B)[NBB],
                                          const float (&dd)[NB], const float (&iv)[NB], float av, float rv,
                                          float dbar, const PairStar &c, const P32 &p, float &lnlp, float &lnpr,
                                          float (&mx)[NV32]) {
    // MLE in scaled units: F = A f, A = 10^(-0.4 mbar), d = D dd
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        float Rj;
        if constexpr (RVF) Rj = A[j];
        else Rj = fmaf(rv, B[j], A[j]);
        const float e = __builtin_amdgcn_exp2f(fmaf(av, Rj, mcC[j]));
        const float fw = e * iv[j];
        num = fmaf(dd[j], fw, num);
        den = fmaf(e, fw, den);
    }
    const float q = __builtin_amdgcn_exp2f(dbar);       // D / A
    const float rden = __builtin_amdgcn_rcpf(den);
    float tt = num * rden;
    float sc = tt * q;
    {
        const bool tiny = sc <= 1e-20f;
        const float tt_lo = 1e-20f * __builtin_amdgcn_rcpf(q);
        tt = tiny ? tt_lo : tt;
        sc = tiny ? 1e-20f : sc;
    }
    const float chi2 = fmaf(tt, fmaf(tt, den, -2.f * num), c.DD2);
    const float lnl = -0.5f * chi2;
    // (both statistics in locals, the references written once at the end: assigned inside the ifs
    // they are stores until this is inlined, and the parallax block ends up a branch, not selects)
    float lp = lnl;
    if (c.any_par) {
        const float dp = __builtin_amdgcn_sqrtf(sc) - c.par;
        lp = c.has_par ? lnl - dp * dp * c.par_hiv : lnl;
    }
    float pr = lnl;
    if (p.dim_prior) pr = c.c0 + c.c1 * ln_pos(chi2) - 0.5f * chi2;
    if (c.any_sp) {
        const float vt = c.sp_var + q * q * rden;
        const float ds = sc - c.sp_mean;
        // (ln(2 pi vt) joins as an explicit fma, the form the kernels have always been compiled to:
        // of a plain "a b + c d" the compiler fuses one product or the other as the code around it
        // changes, and the two roundings differ)
        const float t = -0.5f * fmaf(0.69314718055994531f, __builtin_amdgcn_logf(6.2831853071795865f * vt),
                                     ds * ds * __builtin_amdgcn_rcpf(vt));
        pr = c.sp_on ? pr + t : pr;
    }
    // a chi2 the cancellation cannot resolve, or a star float32 cannot represent:
    // NaN = "re-evaluate in float64"
    lnlp = chi2 > c.eps4 ? lp : NAN;
    // (|lnprob~| < 2^-100 is stored as +0: that range of bit patterns marks survivors in
    // this plane, fit_kernels.hpp surv_tag)
    pr = fabsf(pr) < 0x1p-100f ? 0.f : pr;
    lnpr = chi2 > c.chi2_lo ? pr : NAN;
    mx[MX_NAN_PL] = (lnlp != lnlp || lnpr != lnpr) ? 1.f : mx[MX_NAN_PL];
    mx[MX_LNLP] = vmaxf(mx[MX_LNLP], lnlp);
    mx[MX_LNPR] = vmaxf(mx[MX_LNPR], lnpr);
}

}  // namespace
