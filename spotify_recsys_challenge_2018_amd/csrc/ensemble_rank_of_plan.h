// ensemble_rank_of_plan.h -- where the scratch of a dae_ensemble_rank_of / dae_ensemble_candidates call lies inside ONE allocation of
// the ranking context.  Host only and free of HIP, like rank_of_plan.h, so that a plain C++ program can sweep it
// (tests/host/ensemble_rank_of_plan_main.cpp).  rank_of.hip and ensemble.hip carve by what dae_plan_ensemble_scratch returns.
//
//   thr     [n_ans]  u64    sorted composites per chunk                         (the rank_of words: rank_of.hip)
//   z       [n_ans]  fp32   the answers' canonical y
//   inv     [n_ans]  int32  place of an answer in its chunk
//   gcnt    [n_ans]  u32    buckets          } contiguous: one memset zeroes both
//   glen    [n_rg]   int32  longest rows     }
//   seed_y  [n_seed] fp32   the seeds' canonical y
//   s       [K][n_pairs] fp32   one array of canonical sigmoids per scorer (K = M members, + 1 for the title scorer) over the
//                               LARGER of the two pair lists: the answers' pass and the seeds' pass follow each other on one
//                               stream and share the arrays
// Every section starts on a multiple of 16 bytes, but glen, which follows gcnt directly (a multiple of 4).
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr size_t DAE_ENS_ALIGN = 16;

struct dae_ens_scratch {
    size_t o_thr, o_z, o_inv, o_gcnt, o_glen, o_seed_y, o_s;   // byte offsets
    size_t s_stride;        // floats between two scorers' arrays (a multiple of 4: every array 16-byte aligned)
    size_t zero_bytes;      // gcnt and glen, from o_gcnt
    size_t total;           // bytes of the allocation (0: bad arguments)
};

inline size_t dae_ens_up(size_t x) { return (x + DAE_ENS_ALIGN - 1) / DAE_ENS_ALIGN * DAE_ENS_ALIGN; }

// K scorers, n_ans answers, n_seed seed slots, n_rg row groups of the counting launch.  dae_ensemble_candidates alone: the
// candidates are the "answers" of a plan with n_seed = 0 and n_rg = 0, of which it uses s only.
inline dae_ens_scratch dae_plan_ensemble_scratch(int K, long long n_ans, long long n_seed, int n_rg)
{
    dae_ens_scratch p{};
    if (K < 1 || n_ans < 0 || n_seed < 0 || n_rg < 0) return p;
    const size_t na = (size_t)n_ans, ns = (size_t)n_seed;
    size_t o = 0;
    p.o_thr = o;    o = dae_ens_up(o + na * 8);
    p.o_z = o;      o = dae_ens_up(o + na * 4);
    p.o_inv = o;    o = dae_ens_up(o + na * 4);
    p.o_gcnt = o;   o += na * 4;
    p.o_glen = o;   o += (size_t)n_rg * 4;
    p.zero_bytes = o - p.o_gcnt;
    o = dae_ens_up(o);
    p.o_seed_y = o; o = dae_ens_up(o + ns * 4);
    p.o_s = o;
    const size_t np = na > ns ? na : ns;
    p.s_stride = (np + 3) / 4 * 4;
    o += (size_t)K * p.s_stride * 4;
    p.total = o > 0 ? o : DAE_ENS_ALIGN;
    return p;
}
