// Stand-alone program (no device, no HIP): the host side of the threshold sample's skip.
//   1. the safe threshold: for sets of group maxima and ANY x <= the need-th largest of them, the threshold rule applied to x
//      itself -- dae_tau_value(okey(x) >> 16, 1), what decode_f32_kernel's HALF computes from the image's bounds -- is <= the
//      threshold dae_tau_search finds on the maxima (csrc/tau_search.h: the one copy the kernels run).  x = -inf, sets with
//      fewer than `need` finite keys, NaN x.
//   2. the plan's sample_skip field over a grid of shapes: true exactly where the launcher takes the half-row-group sample
//      (dae_sample_takes_half) on an image with bounds, and what the kernel and the bound table rely on there.
// Exits 0 and prints "all checks passed".  Meant to be built with -fsanitize=address,undefined as well.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "score_plan.h"
#include "tau_search.h"

namespace {

int g_failed = 0;

void fail(const std::string& what)
{
    if (++g_failed <= 20) printf("FAILED: %s\n", what.c_str());
}

// order-preserving fp32 -> u32, restated from csrc/dae_internal.h dae_okey (a device function there)
uint32_t okey(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u << 1) == 0) u = 0;
    return (u & 0x80000000U) ? ~u : (u | 0x80000000U);
}

float tau_of(const std::vector<uint32_t>& keys, unsigned need)
{
    const unsigned lo = dae_tau_search(need, [&](unsigned q0, unsigned q1, unsigned q2, int, unsigned (&c)[3]) {
        c[0] = c[1] = c[2] = 0;
        for (uint32_t k : keys) { c[0] += k >= q0; c[1] += k >= q1; c[2] += k >= q2; }
    });
    return dae_tau_value(lo, 1);
}

float tau_safe_of(float x) { return dae_tau_value(okey(x) >> 16, 1); }

// !(a <= b) with -inf <= -inf; a NaN tau_safe keeps every tile (the kernel's !(U < tau)), so it is never "above"
bool above(float tau_safe, float tau) { return tau_safe > tau; }

long long check_tau_safe()
{
    std::mt19937 rng(12345);
    long long n = 0;
    const float inf = INFINITY;
    for (int rep = 0; rep < 4000; ++rep) {
        const int cnt = (int)(rng() % 301);
        const int kind = rep % 6;
        std::vector<float> v(cnt);
        for (float& f : v) {
            const double u = (double)rng() / 4294967296.0;
            switch (kind) {
                case 0: f = (float)(-12.0 + 14.0 * u); break;                     // logits of a scoring call
                case 1: f = (float)((u - 0.5) * pow(10.0, (double)(rng() % 60) - 30.0)); break;
                case 2: f = -4.5f; break;                                         // all equal
                case 3: f = (rng() % 3) ? -inf : (float)(-8.0 + u); break;        // mostly absent
                case 4: f = (float)(-4.0 - u * 0x1p-9); break;                    // one 16-bit prefix
                default: f = (rng() % 2) ? (float)(u - 0.5) : (rng() % 2 ? 0.0f : -0.0f); break;
            }
        }
        std::vector<uint32_t> keys(cnt);
        for (int i = 0; i < cnt; ++i) keys[i] = okey(v[i]);
        std::vector<float> sorted = v;
        std::sort(sorted.begin(), sorted.end(), std::greater<float>());
        for (unsigned need : {1u, (unsigned)std::max(cnt - 1, 1), (unsigned)std::max(cnt, 1), (unsigned)cnt + 1u, 1124u}) {
            const float tau = tau_of(keys, need);
            const bool have = need <= (unsigned)cnt && sorted[need - 1] > -inf;
            if (!have && tau != -inf) fail("fewer than `need` finite keys: tau is not -inf");
            const float m = have ? sorted[need - 1] : -inf;                       // the need-th largest maximum
            if (above(tau, m)) fail("tau above the element of rank `need`");
            // x: the element itself, a little and a lot below it, the next float down, -inf
            const float xs[] = {m, nextafterf(m, -inf), m - fabsf(m) * 0x1p-10f, m - 1.0f, m - fabsf(m), -inf, m * 1.0f - 1e-30f};
            for (float x : xs) {
                if (!(x <= m)) continue;                                          // (m = -inf: only -inf itself)
                const float ts = tau_safe_of(x);
                if (above(ts, tau)) {
                    char b[160];
                    snprintf(b, sizeof(b), "tau_safe %.9g of x = %.9g above tau = %.9g (need %u of %d, rank element %.9g)", ts, x, tau, need, cnt, m);
                    fail(b);
                }
                if (x == -inf && ts != -inf) fail("x = -inf must give tau_safe = -inf");
                ++n;
            }
        }
    }
    // a NaN x keeps everything: tau_safe is a NaN (positive) or -inf (negative: its key lies below -inf's)
    const float q = tau_safe_of(NAN), qn = tau_safe_of(-NAN);
    if (!(q != q || q == -inf) || !(qn != qn || qn == -inf)) fail("NaN x must give a NaN or -inf");
    if (tau_safe_of(-inf) != -inf) fail("tau_safe(-inf)");
    return n;
}

long long check_plans()
{
    const int Bs[] = {1, 32, 64, 65, 128, 129, 130, 192, 256, 257, 512, 1024, 4096};
    const int Hps[] = {32, 128, 224, 256, 512};
    const int ks[] = {1, 100, 500, 1024, 1025, 2048, 4096};
    const int widths[] = {32, 2048, 8000, 16384, 36000, 65536, 100000, 170000, 300000};
    long long n = 0, n_true = 0;
    for (int B : Bs) for (int Hp : Hps) for (int w : widths) for (int k : ks) for (int dt = 0; dt < 3; ++dt)
    for (int mixed = 0; mixed < 2; ++mixed) for (int ov = 0; ov < 2; ++ov) for (int ub = 0; ub < 2; ++ub) for (int fs = 0; fs < 2; ++fs)
    for (int part = 0; part < 2; ++part) {
        const int n_tracks = part ? (int)((long long)w * 14 / 17) : w;
        const dae_rowgeom g = dt == DAE_DTYPE_F32 ? dae_row_geometry(B, Hp) : dae_row_geometry_bf16(B, Hp);
        const dae_plan_in in{(w + 31) / 32, 0, w, Hp, ub != 0, g, n_tracks, k, dt, mixed != 0, ov, fs, false, B};
        const dae_score_plan p = dae_plan_topk(in);
        ++n;
        if (p.bad_mix) { if (p.sample_skip) fail("sample_skip on a refused plan"); continue; }
        const bool half = p.fused && dae_sample_takes_half(p.gA, p.dtype, Hp, p.mixed, p.gmax_per_wave, p.n_samp);
        if (p.sample_skip != (half && ub != 0)) fail("sample_skip != half-row-group sample on an image with bounds");
        // no other field moves with the switch or the bounds' presence (build_live / live_in_tau are the filter launch's)
        dae_plan_in in2 = in;
        in2.ub_valid = !in.ub_valid;
        const dae_score_plan p2 = dae_plan_topk(in2);
        if (p2.n_samp != p.n_samp || p2.ld_g != p.ld_g || p2.ld_s != p.ld_s || p2.gmax_per_wave != p.gmax_per_wave || p2.S != p.S ||
            memcmp(p2.last, p.last, sizeof(p.last)) != 0)
            fail("the sample's geometry depends on the bounds");
        if (!p.sample_skip) continue;
        ++n_true;
        if (!(p.dtype == DAE_DTYPE_F32 && !p.mixed && !p.exact && !p.whole_b && !p.wave_groups && !p.use_band)) fail("sample_skip: not the fp32 sample");
        if (!(g.R_TILE == 128 && Hp == 256 && g.waves == 4 && B > 64)) fail("sample_skip: not 128-row groups of hidden 256");
        if (p.gA.nb_rg != g.nb_rg) fail("sample_skip: the sample has a geometry of its own");
        if (p.n_samp > 4 * g.nb_rg) fail("sample_skip: more than one round of tiles");
        if (p.ld_g != (int64_t)g.nb_rg * 32) fail("sample_skip: one maximum per (workgroup, position)");
        if (p.ld_g < 4 * (int64_t)k) fail("sample_skip: fewer than 4 k maxima");
        if (g.nb_rg * 32 > 8192) fail("sample_skip: more groups than the bound table sorts");
    }
    if (n_true == 0) fail("the sweep never met a plan with sample_skip");
    printf("plans: %lld, %lld with sample_skip\n", n, n_true);
    return n;
}

}  // namespace

int main()
{
    const long long n_tau = check_tau_safe();
    printf("tau_safe: %lld cases\n", n_tau);
    check_plans();
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("all checks passed\n");
    return 0;
}
