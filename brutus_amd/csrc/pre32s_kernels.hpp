// pre32s_kernels.hpp -- the float32 proof pass with the roles of the lanes swapped: lane = STAR,
// the models pass by as rows broadcast from LDS.  Compiled in the library's second translation unit,
// pre32s_unit.hip (same statistics, same outputs as k_pre32 of fit2_kernels.hpp, which stays for
// short star lists and for more than 12 bands).
//
// Why (round 5; profiles/r05_pre32_bound.txt).  k_pre32 (lane = model, four stars per
// workgroup) holds the tile's coefficients in vector registers and takes the stars' ~60
// constants as scalar operands -- 4 x 60 scalars do not fit the scalar file, so every (tile,
// star) step reloads them through the scalar cache in ~8 dependent s_load / s_waitcnt
// lgkmcnt(0) round trips; with its branches (`live`, `lw == lw`, has_par, sp_on) and the
// 40-value cross-lane reduction at the end of a workgroup it issues ~295 vector instructions
// per (star, model) pair, 19 of them transcendental (3 issue slots each, tools/ubench/
// dpp_rate.hip): 0.57 ms of pure issue per 128 stars at the measured 1.16 ns per float32
// wave-instruction and SIMD, 0.69 ms observed.  Here a wave owns 64 STARS for a run of models:
// the stars' constants stay in ~60 vector registers for the whole run; everything that depends
// on the model alone (the centred magnitudes times -0.4 log2(10), R = r0 + Rv dr) is computed
// once per model, not once per (star, model), and reaches the lanes as a row of broadcast LDS
// reads; every per-star condition is a select, the running maxima live in the lanes (no
// cross-lane reduction at all), and the two float32 planes leave through a 16-model LDS
// transposition as 64-byte row segments.  ~230 vector instructions per pair.
// Forms tried on the way (same-box A/B, profiles/r05_pre32_forms.txt):
//  * the rows as a table in global memory read with scalar loads, one batch per step: every row
//    a scalar-cache miss, ~1.3 us of exposed latency per step -- 0.80-0.90 ms; a streaming read
//    does not belong on the scalar path;
//  * 49 broadcast values per step (mc AND -0.4 log2(10) mc, R, R^2, mbar) against 25 (scaled
//    magnitudes, below; R^2 formed in the lanes): 0.605 against 0.64 ms -- neither the LDS pipe
//    nor the global stores (left out: 0.613) set the pace, the vector instructions do (measured
//    1.16 ns per float32 wave-instruction and SIMD from two waves per SIMD up, 3 slots per
//    transcendental: 234 + 34 slots x 1536 steps per SIMD = 0.48 ms at full issue rate);
//  * the row in the LANES of four registers, read through the DPP row broadcast of the
//    consuming instructions (v_fmac_f32_dpp row_newbcast:j): no LDS traffic to speak of, but a
//    DPP operation issues at 0.6 of the plain rate (ubench) and hipcc cannot see a VALU-write ->
//    DPP-read hazard inside asm statements (a software-pipelined form produced wrong maxima):
//    0.74 ms.
// Scaled magnitudes.  With c = -0.4 log2(10), the stars' centred magnitudes pre-multiplied
// (gcC = c gc, gbarC = c gbar) and the models' too (mcC = c mc, mbarC = c mbar), every sum
// that carries y picks up a factor c per y, and the Av solve of fitting.py:176-204 holds
// verbatim for av' = c av with limits and prior mean scaled (c < 0 swaps the two clamps);
// av' is what the flux phase's exponent wants (2^(av' R + mcC)), so the models' plain centred
// magnitudes are never needed.
// Semantics to hold: /root/reference/brutus/fitting.py:173-264 (sweep statistics), :743-759
// (cull statistic), :976-985 + pdf.py:209-218 (first-cut statistic); float32 only ever
// classifies (see fit2_kernels.hpp).
#pragma once

#include "pre32_pair.hpp"

namespace {

constexpr int PS_M = 16;                      // models per tile (staging and transposition)
constexpr int PS_STRIDE = 66;                 // floats per transposition row: (2 m + star) mod 32 is conflict-free
constexpr int ps_row(int nb) { return 3 * nb + 4; }
// (16 bands: 168 registers + 72-160 bytes of scratch at three waves per SIMD -- k_pre32 keeps them)
constexpr bool ps_bands(int nb) { return nb <= 12; }

// One workgroup = one block of F2_T tiles (the unit of part32) x one group of 64 stars; wave w
// takes a quarter of the block's models, in tiles of 16.  Per tile: the wave's lanes (model m =
// lane & 15, band group lane >> 4) turn the 16 models' raw coefficients -- requested a whole
// tile ahead -- into rows of everything that depends on the model alone ([0, NB) mcC_j =
// c (m_j - mbar), [NB, 2NB) R_j = r0_j + rv_mean dr_j (RVF) or r0_j, [2NB, 3NB) R_j^2 (RVF)
// or dr_j, then mbarC = c mbar) in LDS; then lane = star, and each of the 16 steps reads its row with
// uniform-address ds_read_b128 (a broadcast: four values per instruction into every lane).
// The star group is the FAST block index: the workgroups that run together read the same
// coefficients.  General kernels: every star of the launch has kfix = 2 (the opening pass; a
// re-run with other sweep counts goes through k_pre32).
template <int NB, bool RVF>
__global__ void __launch_bounds__(PS_TILE, 3)
k_pre32s(const float *__restrict__ grid, int64_t nmodel, int64_t nmodel_pad, int nstar, int nrun,
         const int32_t *__restrict__ star_ids, const Star32 *__restrict__ stars, P32 p,
         float *__restrict__ lnlp32, float *__restrict__ lnpr32, float *__restrict__ part) {
    // (general rows carry r0^2, r0 dr, dr^2 behind the rest: the five sums without y then cost one
    // fma per band each -- 11 instead of 13 operations per band and pair, k_pre32s<12, general>
    // 1.33 -> 1.24 ms with its re-run; occupancy is not what limits this kernel: two workgroups
    // per CU instead of three cost the pinned form 12 %, the general one 3 %)
    constexpr int ROW = RVF ? ps_row(NB) : ps_row(NB) + 3 * NB;
    constexpr int NBG = NB / 4;                   // bands per staging lane
    constexpr int NF = 3;                         // per-band fields of a row
    __shared__ float s_t[4][2][PS_M][PS_STRIDE];
    __shared__ __attribute__((aligned(16))) float s_row[4][PS_M][ROW];
    __shared__ int64_t s_base[64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ngroup = (nrun + 63) >> 6;
    const int bx = blockIdx.x / ngroup, sg = blockIdx.x - bx * ngroup;
    const int sl = sg * 64 + lane;
    const bool slive = sl < nrun;
    const int s = star_ids[slive ? sl : nrun - 1];
    if (wv == 0) s_base[lane] = slive ? (int64_t)s * nmodel : (int64_t)-1;
    // the star's constants, resident for the whole run of models
    const Star32 &sp = stars[s];
    float gcC[NB], w[NB], dd[NB], iv[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        gcC[j] = PS_C10 * sp.gc[j];
        w[j] = sp.w[j];
        dd[j] = sp.dd[j];
        iv[j] = sp.iv[j];
    }
    const PairStar cst = pair_star(&sp, p);
    // (written out: a loop is unrolled too late for the maxima a kernel never updates to fold away)
    const float NINF = -INFINITY;
    float mx[NV32] = {NINF, NINF, NINF, NINF, NINF, NINF, NINF, NINF, NINF, NINF};
    const int64_t i0 = (int64_t)bx * (F2_T * PS_TILE) + (int64_t)wv * PS_WM;
    const int64_t i1 = i0 + PS_WM < nmodel ? i0 + PS_WM : nmodel;
    // staging role of this lane
    const int sm = lane & 15, bg = lane >> 4;
    const float inv_nf = 1.f / (float)p.nfilt;
    float cm[NBG], cr0[NBG], cdr[NBG];
    auto fetch = [&](int64_t ib) {
        int64_t i = ib + sm;
        i = i < nmodel_pad ? i : nmodel_pad - 1;
#pragma unroll
        for (int k = 0; k < NBG; ++k) {
            const float *q = grid + (int64_t)(3 * (bg * NBG + k)) * nmodel_pad + i;
            cm[k] = q[0];
            cr0[k] = q[nmodel_pad];
            cdr[k] = q[2 * nmodel_pad];
        }
    };
    if (i0 < i1) fetch(i0);
    __syncthreads();
    for (int64_t ib = i0; ib < i1; ib += PS_M) {
        const int nm = (int)(i1 - ib < PS_M ? i1 - ib : PS_M);
        {   // the tile's rows
            float ps = 0.f;
#pragma unroll
            for (int k = 0; k < NBG; ++k)
                if (bg * NBG + k < p.nfilt) ps += cm[k];
            ps += __shfl_xor(ps, 16, 64);
            ps += __shfl_xor(ps, 32, 64);
            const float mbar = ps * inv_nf;
            float *rw = &s_row[wv][sm][0];
#pragma unroll
            for (int k = 0; k < NBG; ++k) {
                const int j = bg * NBG + k;
                rw[j] = PS_C10 * (cm[k] - mbar);
                if constexpr (RVF) {
                    const float R = fmaf(p.rv_mean, cdr[k], cr0[k]);
                    rw[NB + j] = R;
                    rw[2 * NB + j] = R * R;
                } else {
                    rw[NB + j] = cr0[k];
                    rw[2 * NB + j] = cdr[k];
                    rw[NF * NB + 4 + j] = cr0[k] * cr0[k];
                    rw[NF * NB + 4 + NB + j] = cr0[k] * cdr[k];
                    rw[NF * NB + 4 + 2 * NB + j] = cdr[k] * cdr[k];
                }
            }
            if (bg == 0) rw[NF * NB] = PS_C10 * mbar;
        }
        if (ib + PS_M < i1) fetch(ib + PS_M);        // the next tile's coefficients: a whole tile of latency cover
        ps_wave_sync();
        for (int u = 0; u < nm; ++u) {
            // (wave-uniform address: every ds_read_b128 is a broadcast into all lanes)
            const float4 *__restrict__ r4 = reinterpret_cast<const float4 *>(&s_row[wv][u][0]);
            float mcC[NB], A[NB], B[NB];
#pragma unroll
            for (int k = 0; k < NB / 4; ++k) {
                const float4 a = r4[k], c = r4[NB / 4 + k], d = r4[2 * (NB / 4) + k];
                mcC[4 * k] = a.x; mcC[4 * k + 1] = a.y; mcC[4 * k + 2] = a.z; mcC[4 * k + 3] = a.w;
                A[4 * k] = c.x; A[4 * k + 1] = c.y; A[4 * k + 2] = c.z; A[4 * k + 3] = c.w;
                B[4 * k] = d.x; B[4 * k + 1] = d.y; B[4 * k + 2] = d.z; B[4 * k + 3] = d.w;
            }
            const float dbar = cst.gbarC - s_row[wv][u][NF * NB];      // c (gbar - mbar)
            float av, rv = p.rv_mean;                                  // av: c Av throughout
            if constexpr (RVF) {
                float uR = 0.f, RR = 0.f, yR = 0.f, uy = 0.f, yy = 0.f;
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    const float y = gcC[j] - mcC[j];
                    const float yw = y * w[j];
                    uR = fmaf(A[j], w[j], uR);
                    RR = fmaf(B[j], w[j], RR);
                    yR = fmaf(A[j], yw, yR);
                    uy += yw;
                    yy = fmaf(y, yw, yy);
                }
                av = pair_av_step(uR, RR, yR, uy, yy, dbar, cst, p, mx);
            } else {
                float ua = 0.f, ub = 0.f, uy = 0.f, aa = 0.f, ab = 0.f, bb = 0.f, ay = 0.f, by = 0.f, yy = 0.f;
#pragma unroll
                for (int k = 0; k < NB / 4; ++k) {
                    const float4 pa = r4[(NF * NB + 4) / 4 + k], pc = r4[(NF * NB + 4 + NB) / 4 + k],
                                 pb = r4[(NF * NB + 4 + 2 * NB) / 4 + k];
                    const float A2[4] = {pa.x, pa.y, pa.z, pa.w}, AB[4] = {pc.x, pc.y, pc.z, pc.w},
                                B2[4] = {pb.x, pb.y, pb.z, pb.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int j = 4 * k + q;
                        const float y = gcC[j] - mcC[j];
                        const float yw = y * w[j];
                        ua = fmaf(A[j], w[j], ua);
                        ub = fmaf(B[j], w[j], ub);
                        aa = fmaf(A2[q], w[j], aa);
                        ab = fmaf(AB[q], w[j], ab);
                        bb = fmaf(B2[q], w[j], bb);
                        uy += yw;
                        ay = fmaf(A[j], yw, ay);
                        by = fmaf(B[j], yw, by);
                        yy = fmaf(y, yw, yy);
                    }
                }
                pair_sweeps(ua, ub, uy, aa, ab, bb, ay, by, yy, dbar, cst, p, av, rv, mx);
            }
            float lnlp, lnpr;
            pair_tail<NB, RVF>(mcC, A, B, dd, iv, av, rv, dbar, cst, p, lnlp, lnpr, mx);
            s_t[wv][0][u][lane] = lnlp;
            s_t[wv][1][u][lane] = lnpr;
        }
        // the tile leaves transposed: a store covers four stars x sixteen models (64-byte row
        // segments; the next tile of this wave completes the lines)
        ps_wave_sync();
#pragma unroll
        for (int qq = 0; qq < 16; ++qq) {
            const int ss = 4 * qq + bg;
            const float a = s_t[wv][0][sm][ss], b = s_t[wv][1][sm][ss];
            const int64_t base = s_base[ss];
#ifndef PS_DIAG_NOSTORE
            if (sm < nm && base >= 0) {
                // (plain stores: two tiles of this wave complete a 128-byte line in the L2; as
                // non-temporal 64-byte pieces the pass ran 2-3 % slower, its readers 0.02 ms faster)
                lnlp32[base + ib + sm] = a;
                lnpr32[base + ib + sm] = b;
            }
#else
            if (a == 12345.f && b == 54321.f) lnlp32[0] = a;
#endif
        }
        ps_wave_sync();
    }
    // the four waves' maxima meet in LDS (the transposition tiles are free now)
    __syncthreads();
    float *s_mx = &s_t[0][0][0][0];                      // [4][NV32][64]
#pragma unroll
    for (int k = 0; k < NV32; ++k) s_mx[(wv * NV32 + k) * 64 + lane] = mx[k];
    __syncthreads();
    if (wv == 0 && slive) {
#pragma unroll
        for (int k = 0; k < NV32; ++k) {
            float x = s_mx[k * 64 + lane];
            x = vmaxf(x, s_mx[(NV32 + k) * 64 + lane]);
            x = vmaxf(x, s_mx[(2 * NV32 + k) * 64 + lane]);
            x = vmaxf(x, s_mx[(3 * NV32 + k) * 64 + lane]);
            part[((int64_t)bx * nstar + s) * NV32 + k] = x;
        }
    }
}

}  // namespace
