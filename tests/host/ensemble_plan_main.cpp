// Stand-alone program (no device, no HIP): the plans of the ranking call of an ensemble, csrc/score_plan.h dae_plan_topk with
// `mixed` set on a DAE's own context.  Untitled, the ranking context of dae_ensemble_topk is the last member's, so the mixed
// score meets hidden 256 -- the shape whose unmixed calls take the half-row-group sample, the live tile lists and the filter
// skip, none of which knows the mix: score.hip launches by the plan unchecked, and the launchers of decode_f32.hip ask the
// same predicates.
//   1. over a grid of rows, hidden sizes, widths, k, dtypes, bounds and hints: what the mixed launches rely on;
//   2. the shapes of tests/test_gpu_ensemble.py: which of them take the threshold path (sample -> tau -> filter).
// Exits 0 and prints "all checks passed".  Meant to be built with -fsanitize=address,undefined as well.
#include <stdio.h>
#include <string.h>

#include <string>

#include "score_plan.h"

namespace {

int g_failed = 0;

void fail(const std::string& what)
{
    if (++g_failed <= 20) printf("FAILED: %s\n", what.c_str());
}

dae_plan_in plan_in(int B, int Hp, int V, int n_tracks, int k, int dt, bool mixed, bool ub, int overlap, bool own_tau)
{
    const dae_rowgeom g = dt == DAE_DTYPE_F32 ? dae_row_geometry(B, Hp) : dae_row_geometry_bf16(B, Hp);
    dae_plan_in in{(V + 31) / 32, 0, V, Hp, ub, g, n_tracks, k, dt, mixed, overlap, 1};
    in.own_tau = own_tau;
    in.B = B;
    return in;
}

void check_mixed(const dae_plan_in& in, const dae_score_plan& p, const dae_score_plan& plain)
{
    auto bad = [&](const char* what) {
        char b[256];
        snprintf(b, sizeof(b), "%s (B=%d Hp=%d V=%d n_tracks=%d k=%d dtype=%d ub=%d overlap=%d)", what, in.B, in.Hp, in.col_hi, in.n_tracks,
                 in.k, in.dtype_in, (int)in.ub_valid, in.overlap_hint);
        fail(b);
    };
    const dae_rowgeom& g = in.g;
    if (in.dtype_in == DAE_DTYPE_BF16_EXACT) {
        if (!p.bad_mix) bad("exact + mix not refused");
        return;
    }
    if (p.bad_mix || !p.mixed) bad("a mixed plan of fp32 / bf16 arithmetic");
    // the kernels that do not know the mix are never planned, nor asked for by the launchers
    if (p.sample_skip) bad("the mixed sample skips tiles");
    if (p.build_live || p.live_in_tau) bad("the mixed filter launch walks live lists");
    if (p.wave_groups) bad("the mixed sample takes per-wave maxima");
    if (p.whole_b) bad("the mixed filter launch decodes the sample tiles again (maxima-only sample)");
    if (memcmp(&p.gA, &g, sizeof(g)) != 0) bad("the mixed sample has a geometry of its own");
    if (dae_sample_takes_half(g, p.dtype, in.Hp, true, p.gmax_per_wave, p.n_samp)) bad("the mixed sample runs in half row groups");
    if (dae_filter_takes_live(g, p.dtype, in.Hp, true)) bad("the mixed filter launch is the hidden-256 kernel");
    // the generic kernel's walk sizes the candidate lists
    const int n_ws = g.nb_rg * g.waves;
    if (p.cap != g.waves * ((p.n_filter + n_ws - 1) / n_ws) * 32) bad("cap is not the generic kernel's");
    if (p.n_filter != p.n_other) bad("n_filter != n_other");
    // the mix lives in the GMAX / FILTER epilogues: every launch of a mixed call, the unfused one included, stores group maxima
    if (p.ntiles > 0 && p.ld_g < 32) bad("no room for the group maxima");
    if (p.ntiles > 0 && p.gmax_per_wave == 1 && p.ld_g < p.ld_s) bad("gmax_per_wave 1 keeps every sample element");
    if (p.gmax_per_wave != 0 && p.gmax_per_wave != 1) bad("gmax_per_wave of the generic kernel");
    // which tiles form the sample is the unmixed call's: the mix changes kernels, never the split
    if (p.fused != plain.fused || p.S != plain.S || p.n_samp != plain.n_samp || p.n_other != plain.n_other || p.ntiles != plain.ntiles ||
        p.n_valid_col != plain.n_valid_col)
        bad("the mixed plan splits the tiles differently");
}

long long sweep()
{
    const int Bs[] = {1, 5, 32, 37, 64, 65, 128, 129, 256, 257, 1024, 4096};
    const int Hps[] = {64, 96, 256, 320, 448};
    const int ks[] = {1, 500, 1024};
    const int Vs[] = {33, 3295, 5003, 9001, 11003, 21250, 42500, 85000, 170000};
    long long n = 0;
    for (int B : Bs) for (int Hp : Hps) for (int V : Vs) for (int k : ks) for (int dt = 0; dt < 3; ++dt)
    for (int ub = 0; ub < 2; ++ub) for (int ov = 0; ov < 2; ++ov) for (int own = 0; own < 2; ++own) for (int prefix = 0; prefix < 3; ++prefix) {
        const int n_tracks = prefix == 0 ? V : prefix == 1 ? (int)((long long)V * 14 / 17) : V - 5 > 0 ? V - 5 : V;
        const dae_plan_in in = plan_in(B, Hp, V, n_tracks, k, dt, true, ub != 0, ov, own != 0);
        const dae_plan_in in0 = plan_in(B, Hp, V, n_tracks, k, dt, false, ub != 0, ov, own != 0);
        check_mixed(in, dae_plan_topk(in), dae_plan_topk(in0));
        ++n;
    }
    return n;
}

// tests/test_gpu_ensemble.py: (rows, hidden of the ranking context, V, n_tracks) -> does the call take the threshold path?
void test_shapes()
{
    // (hidden 320 in fp32 keeps 64-row groups -- 5 of them at 257 rows, 192 SIMD slots -- so its 232 ranked tiles take the
    // threshold path in fp32 and, in 128-row groups, the dense one in bf16)
    struct S { int B, Hp, V, nt; bool fused[2]; };
    const S shapes[] = {
        {5, 64, 3295, 3290, {false, false}},    {5, 96, 3295, 3290, {false, false}},    {37, 256, 5003, 4100, {false, false}},
        {37, 128, 5003, 4100, {false, false}},  {257, 256, 9001, 7411, {false, false}}, {257, 320, 9001, 7411, {true, false}},
        {257, 256, 11003, 10501, {true, true}}, {37, 64, 3301, 2990, {false, false}},
    };
    for (const S& s : shapes)
        for (int dt = 0; dt < 2; ++dt) {
            const dae_score_plan p = dae_plan_topk(plan_in(s.B, s.Hp, s.V, s.nt, 500, dt, true, true, 0, true));
            char b[128];
            snprintf(b, sizeof(b), "B=%d Hp=%d V=%d n_tracks=%d dtype=%d: fused=%d S=%d", s.B, s.Hp, s.V, s.nt, dt, (int)p.fused, p.S);
            if (p.fused != s.fused[dt]) fail(std::string("the test shape takes another path: ") + b);
            if (s.V == 11003 && (p.S != 2 || p.n_samp != 165 || p.n_other != 164)) fail(std::string("the threshold path's split: ") + b);
        }
    // and the unmixed call of the hidden-256 member on the same rows DOES take what the mixed one must not (fp32, bounds valid)
    const dae_score_plan q = dae_plan_topk(plan_in(257, 256, 11003, 10501, 500, DAE_DTYPE_F32, false, true, 0, true));
    if (!(q.fused && q.sample_skip && q.build_live)) fail("the unmixed hidden-256 plan no longer skips: this test compares against nothing");
}

}  // namespace

int main()
{
    const long long n = sweep();
    printf("sweep: %lld mixed plans\n", n);
    test_shapes();
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("all checks passed\n");
    return 0;
}
