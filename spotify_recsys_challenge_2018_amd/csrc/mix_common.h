// mix_common.h -- what the units of the exact title mix (mixexact.hip has the overview) share: the constants, and the
// scalar device helpers more than one of their kernels uses -- the mixed score and its cheap bounds.
//
// BOUNDS.  DAE side: hidden rows lie in [0, 1], eps_c of exact_bounds_kernel (prepack.hip) as in the plain exact mode.
// Title side: the features are ReLU maxima, not confined to [0, 1]; with F_r = max_k |feat[r][k]| every term of that
// derivation that is linear in the hidden row scales by F_r:
//     |z16_t - z32_t| <= F_r alpha_c + beta_c,
//     alpha_c = (1 + 2^-8) d_c + 2^-9 n_c + A16 (1 + 2^-8)(n_c + d_c) + A32 n_c,   beta_c = (1.01 A16 + A32 + 2^-23) |b_c|
// (d_c, n_c, A16, A32 as there; both inflated for the feedback of the shift through the accumulation: mix_prep.hip
// mix_title_bounds_kernel).  The shift itself goes through the matrix pipe like the bias: k-slot 3 of the tile's bias fragment
// holds +-alpha_c (bf16, rounded up), k-slot 3 of the row's "ones" fragment holds F_r (bf16, rounded up), slots 0..2 the
// three-term split of b_c +- beta_c.
// The canonical sigmoid is monotone only to one unit in the last place (920 one-ulp inversions among the 2.2 10^9 floats of
// [-88, 88], checked exhaustively), so bounds of the mixed value are widened (2^-15 with the hardware's exp2 / rcp, whose
// results lie within 6e-6 of the canonical ones) before they are compared; the guard compares LOGITS, which need none.
#pragma once
#include "dae_internal.h"
#include "mix_plan.h"               // MX_RB, MX_NW, MX_REF_CAP, MX_MAX_STEPS, MX_LDS_BYTES, MR_MAX_SEG, MR_STAGE

constexpr int MX_QR = 8;            // W ring depth (steps)

// the mixed score with the operations of mix_scores_kernel (title.hip) / the fp32 mix epilogue (decode_generic.hip), in their order
__device__ __forceinline__ float mixf(float zt, float zd, float wt, float wp)
{
    const float ts = dae_sigmoidf(zt) * wt;
    const float pd = dae_sigmoidf(zd) * wp;
    return ts + pd;
}
// The threshold sample evaluates every element, so it takes the hardware's exp2 / rcp (1 ulp each) instead of the canonical
// polynomial (4 instructions against ~35): within 6.1e-6 relative of the canonical value for every finite logit (the
// argument's rounding, |z| log2(e) 2^-24 <= 7.6e-6 in the exponent, dominates), hence a lower bound after 2^-15 relative.
__device__ __forceinline__ float sig_fast(float z)
{
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(z * -1.44269504088896341f));
}
// Can w_t sigmoid(z_t) + w_p sigmoid(z_d) reach tau?  True whenever the canonical mixed value, widened by 2^-20, does (the
// caller passes tau (1 - 2^-17): rounding, the canonical sigmoid's <= 3 ulp and its 1-ulp inversions); false only with 2^-15 of room.  With E = exp(-z) (v_exp_f32: 1 ulp, its argument's
// rounding <= 6e-6 relative in E; arguments capped at 2^60, which only raises the left side's share):
//     w_t / (1 + E_t) + w_p / (1 + E_d) >= tau  <=>  w_t (1 + E_d) + w_p (1 + E_t) >= tau (1 + E_t)(1 + E_d)
__device__ __forceinline__ bool mix_can_reach(float zt, float zd, float wt, float wp, float tau)
{
    const float et = 1.0f + __builtin_amdgcn_exp2f(fminf(zt * -1.44269504088896341f, 60.0f));
    const float ed = 1.0f + __builtin_amdgcn_exp2f(fminf(zd * -1.44269504088896341f, 60.0f));
    const float lhs = fmaf(wp, et, wt * ed);
    const float rhs = (tau * et) * ed;
    return fmaf(lhs, 0x1p-15f, lhs) >= rhs;
}
// Per-lane LOGIT thresholds that every column passing mix_can_reach must meet, given the lane's maxima mT >= z_t, mD >= z_d over its
// columns: w_t s(z_t) + w_p s(z_d) >= tau with s(z_d) <= s(mD) needs s(z_t) >= (tau - w_p s(mD)) / w_t =: a, i.e. z_t >= logit(a) -- and the
// same with the roles swapped.  One compare per element instead of two v_exp_f32 and five multiply-adds: on a title scorer whose
// score is a flat background (an untrained one: bench.py's) the pair of maxima passes in nearly every lane, and the per-element tests
// were a third of the launch.  NECESSARY conditions only (the exact test still decides): every bound is taken on the safe side --
// tau 2^-12 lower (mix_can_reach's own slack is 2^-15 plus a few 1e-7 of hardware exp / rcp error), the maxima's sigmoids 2^-18 higher,
// the quotient 2^-18 lower, the logit 2^-16 (relative and absolute) lower; a >= 0.999 (a column that needs a saturated sigmoid) keeps
// logit(0.999), a <= 0 (the other scorer's maximum alone reaches tau) keeps -inf.  A scorer with weight 0 puts no condition on its logit.
__device__ __forceinline__ float mix_logit_floor(float a)
{
    if (!(a > 1e-30f)) return -__builtin_inff();
    a = fminf(a, 0.999f);
    const float l = (__builtin_amdgcn_logf(a) - __builtin_amdgcn_logf(1.0f - a)) * 0.69314718f;        // ln(a / (1 - a))
    return l - (fabsf(l) * 0x1p-16f + 0x1p-16f);
}
__device__ __forceinline__ void mix_thresholds(float mT, float mD, float wt, float wp, float tau, float& th_t, float& th_d)
{
    const float sT = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(fminf(mT * -1.44269504088896341f, 60.0f))) * (1.0f + 0x1p-18f);
    const float sD = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(fminf(mD * -1.44269504088896341f, 60.0f))) * (1.0f + 0x1p-18f);
    const float tl = tau * (1.0f - 0x1p-12f);
    const float nt = tl - wp * sD, nd = tl - wt * sT;            // what the title / the DAE term has to supply at least
    th_t = wt > 0.0f ? mix_logit_floor(nt > 0.0f ? nt * __builtin_amdgcn_rcpf(wt) * (1.0f - 0x1p-18f) : -1.0f) : -__builtin_inff();
    th_d = wp > 0.0f ? mix_logit_floor(nd > 0.0f ? nd * __builtin_amdgcn_rcpf(wp) * (1.0f - 0x1p-18f) : -1.0f) : -__builtin_inff();
}
__device__ __forceinline__ float mix_fast_dn(float zt, float zd, float wt, float wp)
{
    const float y = sig_fast(zt) * wt + sig_fast(zd) * wp;
    return fmaf(y, -0x1p-15f, y);
}
__device__ __forceinline__ float mix_fast_up(float zt, float zd, float wt, float wp)
{
    const float y = sig_fast(zt) * wt + sig_fast(zd) * wp;
    return fmaf(y, 0x1p-15f, y);
}
