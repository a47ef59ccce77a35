// Stand-alone program (no device, no HIP): the integer part of the threshold launch, csrc/tau_search.h.
//   1. dae_tau_search, fed by a brute-force counting functor over an array of order-preserving keys, returns the largest
//      prefix P >= DAE_TAU_P_MIN with count(key >= P << 16) >= need, or DAE_TAU_P_MIN - 1 exactly when fewer than `need` keys
//      above -inf exist; it asks for at most 8 counts, its probes ascend, and `step` numbers the calls;
//   2. dae_tau_key lowers the key by 4 only when there is no dense sample (n_s == 0) and the key is more than 8 above
//      DAE_KEY_NEG_INF;
//   3. dae_tau_value is <= the element of rank `need`, and -inf when the search found nothing.
// Arrays of 0 .. 300 keys: random floats over several magnitudes, all equal, all -inf, a plateau that straddles the cut, values
// that share their 16 leading key bits; need in {1, n - 1, n, n + 1, 1024 + 100}.
// Exits 0 and prints "all checks passed".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "tau_search.h"

namespace {

int g_failed = 0;
long long g_cases = 0, g_found = 0, g_missing = 0;

// csrc/dae_internal.h dae_okey: order-preserving fp32 -> u32 (bigger key = bigger float, -0 == +0)
uint32_t okey(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u << 1) == 0) u = 0;
    return (u & 0x80000000U) ? ~u : (u | 0x80000000U);
}
float okey_inv(uint32_t k)
{
    const uint32_t u = (k & 0x80000000U) ? (k & 0x7FFFFFFFU) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}
float rnd_unit() { return (float)(rnd() >> 8) * (1.0f / 16777216.0f); }

void fail(const char* what, const char* kind, size_t n, unsigned need, int n_s)
{
    if (++g_failed <= 20) printf("FAILED: %s (%s, n=%zu need=%u n_s=%d)\n", what, kind, n, need, n_s);
}

unsigned count_ge(const std::vector<uint32_t>& keys, uint32_t q)
{
    unsigned c = 0;
    for (uint32_t k : keys) c += k >= q ? 1u : 0u;
    return c;
}

void check(const char* kind, const std::vector<float>& v, unsigned need)
{
    ++g_cases;
    std::vector<uint32_t> keys;
    for (float f : v) keys.push_back(okey(f));
    int calls = 0;
    bool order_ok = true, step_ok = true;
    const unsigned lo = dae_tau_search(need, [&](unsigned q0, unsigned q1, unsigned q2, int step, unsigned (&c)[3]) {
        order_ok = order_ok && q0 <= q1 && q1 <= q2 && q0 >= (DAE_TAU_P_MIN << 16) && (q0 & 0xFFFFu) == 0 && (q1 & 0xFFFFu) == 0 &&
                   (q2 & 0xFFFFu) == 0;
        step_ok = step_ok && step == calls;
        ++calls;
        c[0] = count_ge(keys, q0); c[1] = count_ge(keys, q1); c[2] = count_ge(keys, q2);
    });
    if (!order_ok) fail("probes out of order, below the smallest prefix or not whole prefixes", kind, v.size(), need, -1);
    if (!step_ok) fail("step does not number the calls", kind, v.size(), need, -1);
    if (calls > 8) fail("more than 8 counting steps", kind, v.size(), need, -1);
    // the largest prefix with enough keys at or above it (the count falls as the prefix rises, so its two neighbours decide)
    if (lo < DAE_TAU_P_MIN - 1u || lo > 0xFFFFu) fail("prefix out of range", kind, v.size(), need, -1);
    if (lo >= DAE_TAU_P_MIN && count_ge(keys, lo << 16) < need) fail("too few keys at or above the prefix", kind, v.size(), need, -1);
    if (lo < 0xFFFFu && count_ge(keys, (lo + 1u) << 16) >= need) fail("a larger prefix has enough keys", kind, v.size(), need, -1);
    unsigned present = 0;
    for (uint32_t k : keys) present += k > DAE_KEY_NEG_INF ? 1u : 0u;
    const bool found = lo >= DAE_TAU_P_MIN;
    if (found != (present >= need)) fail("the sentinel must come back exactly when fewer than `need` keys exist", kind, v.size(), need, -1);
    found ? ++g_found : ++g_missing;
    std::vector<float> sorted(v);
    std::sort(sorted.begin(), sorted.end(), std::greater<float>());
    for (int n_s : {0, 32, 2048}) {
        const float tv = dae_tau_value(lo, n_s);
        if (!found) {
            if (!(tv == -INFINITY)) fail("no prefix found: tau must be -inf", kind, v.size(), need, n_s);
            continue;
        }
        if (!(tv <= sorted[need - 1])) fail("tau above the element of rank `need`", kind, v.size(), need, n_s);
        if (!(tv > -INFINITY)) fail("a found tau must be above -inf", kind, v.size(), need, n_s);
        if (okey(tv) != dae_tau_key(lo, n_s)) fail("dae_tau_value is not the float of dae_tau_key", kind, v.size(), need, n_s);
    }
}

void check_all_needs(const char* kind, const std::vector<float>& v)
{
    const unsigned n = (unsigned)v.size();
    for (unsigned need : {1u, n - 1u, n, n + 1u, 1024u + 100u})
        if (need >= 1u && need != 0xFFFFFFFFu) check(kind, v, need);
}

}  // namespace

int main()
{
    // 2. the slack rule, over every prefix the search can return
    for (unsigned lo = DAE_TAU_P_MIN - 1u; lo <= 0xFFFFu; ++lo) {
        const uint32_t key = lo << 16;
        for (int n_s : {0, 32, 4096}) {
            const bool slack = n_s == 0 && key > DAE_KEY_NEG_INF + 8u;
            const uint32_t got = dae_tau_key(lo, n_s);
            if (got != (slack ? key - 4u : key)) fail("dae_tau_key: the 4-key slack rule", "prefix sweep", 0, lo, n_s);
            if (lo >= DAE_TAU_P_MIN && got <= DAE_KEY_NEG_INF) fail("dae_tau_key fell to -inf", "prefix sweep", 0, lo, n_s);
        }
    }
    if (dae_tau_key(DAE_TAU_P_MIN, 0) != (DAE_TAU_P_MIN << 16)) fail("the smallest prefix sits 1 above -inf: no slack", "edge", 0, DAE_TAU_P_MIN, 0);
    if (dae_tau_key(DAE_TAU_P_MIN + 1u, 0) != ((DAE_TAU_P_MIN + 1u) << 16) - 4u) fail("slack expected", "edge", 0, DAE_TAU_P_MIN + 1u, 0);

    // 1. and 3.
    const float mags[] = {1e-30f, 1e-6f, 1.0f, 37.5f, 1e6f, 1e30f};
    for (size_t n = 0; n <= 300; ++n) {
        std::vector<float> v(n);
        for (float mag : mags) {                                  // random, both signs, one magnitude
            for (float& x : v) x = (rnd_unit() * 2.0f - 1.0f) * mag;
            check_all_needs("random", v);
        }
        for (float& x : v) x = (rnd_unit() * 2.0f - 1.0f) * mags[rnd() % 6];   // ... and mixed magnitudes, with zeros and -inf
        for (size_t i = 0; i < n; i += 7) v[i] = (i % 14) ? -INFINITY : (i % 28 ? 0.0f : -0.0f);
        check_all_needs("mixed", v);
        for (float c : {0.0f, -3.25f, 1e-38f, 12345.678f}) {      // all equal
            std::fill(v.begin(), v.end(), c);
            check_all_needs("all equal", v);
        }
        std::fill(v.begin(), v.end(), -INFINITY);                 // nothing present
        check_all_needs("all -inf", v);
        if (n >= 4) {
            // a plateau that straddles the cut: a third above, a third ON the value, the rest below; cut inside the plateau
            for (size_t i = 0; i < n; ++i) v[i] = i < n / 3 ? 2.0f + rnd_unit() : (i < 2 * n / 3 + 1 ? 1.5f : rnd_unit());
            for (size_t i = n - 1; i > 0; --i) std::swap(v[i], v[rnd() % (uint32_t)(i + 1)]);
            check_all_needs("plateau", v);
            check("plateau", v, (unsigned)(n / 3 + 1));
            check("plateau", v, (unsigned)(n / 2));
            // values that share their 16 leading key bits: the search cannot separate them, tau sits at or below all of them
            const uint32_t base = okey(-0.7312f) & 0xFFFF0000u;
            for (float& x : v) x = okey_inv(base | (rnd() & 0xFFFFu));
            check_all_needs("shared prefix", v);
            check("shared prefix", v, (unsigned)(n / 2));
            v[0] = okey_inv(base + 0x10000u);                     // ... and one in the next prefix
            check("shared prefix + 1", v, 1u);
            check("shared prefix + 1", v, 2u);
        }
    }
    printf("%lld cases (%lld with a threshold, %lld without), %d failed\n", g_cases, g_found, g_missing, g_failed);
    if (g_failed || g_found == 0 || g_missing == 0) return 1;
    printf("all checks passed\n");
    return 0;
}
