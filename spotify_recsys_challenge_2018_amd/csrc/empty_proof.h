// empty_proof.h -- the arithmetic by which the threshold launch proves the filter launch's live list EMPTY without any hand-off
// between its workgroups (tau_select.hip tau_select_kernel's LIVE && SPARSE instances).  Free of HIP and
// callable from host and device, as tau_search.h is, so that a plain C++ program can exercise it (tests/host/empty_proof_main.cpp).
//
// The live-list tail keeps item t of a row group iff !(U_t(d) < tau_min), U_t(d) = A_t + d' M_t + pad (decode_common.h
// dae_tile_is_live), d = the group's max |h - 0.5| in double, tau_min = its smallest threshold.  For M_t >= 0 every operation in
// U_t is a monotone rounding, so U_t is non-decreasing in d.  The ENVELOPE of a filter list is, on the grid d_j = j 2^-9,
// j = 0 .. DAE_PROOF_GRID, G[j] >= max_t U_t(d_j), as a float rounded UP (NaN: an item with a NaN pair or M_t < 0 -- no proof).
// With D >= d and T <= tau_min (the sample launch's dq and tau_safe of the group's half groups), j = dae_proof_index(D):
//     G[j] < T   =>   U_t(d) <= U_t(d_j) <= G[j] < T <= tau_min for every t   =>   the tail would keep nothing.
#pragma once
#include <math.h>

#include "tau_search.h"           // DAE_HD

constexpr int DAE_PROOF_GRID = 256;                      // d_j = j * 2^-9: [0, 0.5], what a hidden row in [0, 1] can reach
constexpr int DAE_PROOF_ENV = DAE_PROOF_GRID + 1;         // floats of an envelope

DAE_HD float dae_proof_grid_d(int j) { return (float)j * 0x1p-9f; }      // exact

// the smallest j with d_j >= D; -1 (no proof) for D > 0.5, D < 0 and a NaN
DAE_HD int dae_proof_index(float D)
{
    if (!(D >= 0.0f) || !(D <= 0.5f)) return -1;
    int j = (int)(D * 512.0f);                            // (a power of two: exact; truncated)
    if ((float)j * 0x1p-9f < D) ++j;
    return j;
}

// what dae_tile_is_live compares with tau_min, at d_max = d: the same operations in the same order (the library is built without
// contraction, and so is the host test)
DAE_HD double dae_proof_bound(float A_t, float M_t, double d_max)
{
    const double d = d_max * (1.0 + 0x1p-40);
    const double A = (double)A_t, dm = d * (double)M_t;
    return A + dm + (fabs(A) + fabs(dm)) * 0x1p-48;
}

// one item's contribution to G[j], before the maximum: U at d_j; a NaN for M_t < 0 (U would not be monotone in d) or a NaN pair
DAE_HD double dae_proof_item(float A_t, float M_t, int j)
{
    if (!(M_t >= 0.0f) || A_t != A_t) return (double)__builtin_nanf("");
    return dae_proof_bound(A_t, M_t, (double)dae_proof_grid_d(j));
}

// a double as a float that is not below it (NaN stays NaN, +-inf stay)
DAE_HD float dae_proof_float_up(double u)
{
    float f = (float)u;
    if ((double)f < u) f = nextafterf(f, __builtin_inff());
    return f;
}

// the verdict: false on a NaN and on T = -inf
DAE_HD bool dae_proof_holds(float G_j, float T) { return (double)G_j < (double)T; }
