// tau_search.h -- the integer part of the threshold launch (tau_select.hip): the search for the largest 16-bit key prefix with
// enough keys at or above it, and the key -> threshold rule.  Free of HIP and callable from host and device, so that a plain
// C++ program can exercise it (tests/host/tau_search_main.cpp) and both threshold kernels run the one copy.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DAE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DAE_HD inline
#endif

constexpr uint32_t DAE_KEY_NEG_INF = 0x007FFFFFU;   // dae_okey(-inf): "absent" marker

// prefixes below DAE_TAU_P_MIN would count -inf / absent entries
constexpr unsigned DAE_TAU_P_MIN = (DAE_KEY_NEG_INF >> 16) + 1u;

// The largest prefix P in [DAE_TAU_P_MIN, 0xFFFF] with count(key >= P << 16) >= need, or DAE_TAU_P_MIN - 1 when fewer than
// `need` finite keys exist.  4-ary: count3(q0, q1, q2, step, c) leaves in c[e] the number of keys >= q_e (q0 <= q1 <= q2; the
// same values in every thread that takes part; `step` counts the calls, for callers that alternate buffers) -- 8 calls.
// The search runs over [P_MIN - 1, 0xFFFF]: P_MIN - 1 stands for "fewer than `need` keys exist" (count taken as >= need by
// convention, never probed -- every probe is > lo), so no separate existence pass is needed.
template <typename Count3>
DAE_HD unsigned dae_tau_search(unsigned need, Count3 count3)
{
    unsigned lo = DAE_TAU_P_MIN - 1u, hi = 0xFFFFu;              // the answer lies in [lo, hi]
    int it = 0;
    unsigned c[3];
    while (lo < hi) {                                            // invariant: count(lo) >= need, count(hi + 1) < need
        const unsigned span = hi - lo;                           // >= 1; three probes cut [lo + 1, hi] into four parts
        const unsigned m1 = lo + (span + 3u) / 4u, m2 = lo + (2u * span + 3u) / 4u, m3 = lo + (3u * span + 3u) / 4u;
        count3(m1 << 16, m2 << 16, m3 << 16, it++, c);           // lo < m1 <= m2 <= m3 <= hi
        if (c[2] >= need) lo = m3;
        else if (c[1] >= need) { lo = m2; hi = m3 - 1u; }
        else if (c[0] >= need) { lo = m1; hi = m2 - 1u; }
        else hi = m1 - 1u;
    }
    return lo;
}

// The threshold of a found prefix, as an order-preserving key.  tau = the float of P << 16: at most 2^-7 (relative) below the
// element of that rank.
// No dense sample (n_s == 0: the bf16 filter launch decodes the sample tiles AGAIN and every candidate comes from it):
// the element tau was taken from has to pass a compare in ANOTHER kernel.  Both kernels run the same MFMA sequence on
// the same operands, so the values agree bit for bit (tests/test_gpu_bf16.py); 4 ulp of slack make the row's k
// candidates independent of that (a tau sitting exactly on its element, and a last-bit difference, would otherwise
// leave the row one candidate short: -1 padding instead of an error).
DAE_HD unsigned dae_tau_key(unsigned lo, int n_s)
{
    return (n_s == 0 && (lo << 16) > DAE_KEY_NEG_INF + 8u) ? (lo << 16) - 4u : (lo << 16);
}

// ... and as the float the kernels store: -inf when the search found no prefix (fewer than `need` keys)
DAE_HD float dae_tau_value(unsigned lo, int n_s)
{
    const bool found = lo >= DAE_TAU_P_MIN;
    const uint32_t k = dae_tau_key(lo, n_s);
    const uint32_t u = (k & 0x80000000U) ? (k & 0x7FFFFFFFU) : ~k;       // dae_okey_inv
    return found ? __builtin_bit_cast(float, u) : -__builtin_inff();
}
