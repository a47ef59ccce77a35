// Stand-alone program (no device, no HIP): WHO builds the live lists of the fp32 filter launch, csrc/score_plan.h
// dae_plan_topk's live_in_tau.  Over the sweep of shapes of score_plan_main.cpp, with the thresholds the call's own or not
// (dae_plan_in::own_tau) and the rows of the call (dae_plan_in::B):
//   1. live_in_tau implies build_live, own_tau, and the workgroup-per-row threshold kernel (!dae_tau_wave_per_row);
//   2. it is false whenever own_tau is false;
//   3. every other field of the plan is independent of own_tau and B.
// Exits 0 and prints "all checks passed".
#include <stdio.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "score_plan.h"

namespace {

int g_failed = 0;
long long g_live = 0, g_wave = 0;

void fail(const char* what, const dae_plan_in& in)
{
    if (++g_failed <= 20)
        printf("FAILED: %s (ntiles=%d cols=[%d,%d) Hp=%d n_rg=%d n_tracks=%d k=%d dtype=%d mixed=%d overlap=%d skip=%d own_tau=%d B=%d)\n", what,
               in.ntiles, in.col_lo, in.col_hi, in.Hp, in.g.n_rg, in.n_tracks, in.k, in.dtype_in, (int)in.mixed, in.overlap_hint,
               in.filter_skip, (int)in.own_tau, in.B);
}

// every field but live_in_tau
std::vector<long long> words(const dae_score_plan& p)
{
    std::vector<long long> w = {p.bad_mix, p.dtype, p.exact, p.mixed, p.n_valid_col, p.nrank, p.ntiles, p.S, p.n_samp, p.n_other,
                                p.fused, p.gA.R_TILE, p.gA.n_rg, p.gA.Bpad, p.gA.nb_rg, p.gA.grid, p.gA.waves, p.wave_groups,
                                p.use_band, p.ld_s, p.ld_g, p.gmax_per_wave, p.whole_b, p.n_filter, p.cap, p.build_live};
    for (int i = 0; i < 8; ++i) w.push_back(p.last[i]);
    return w;
}

void check(const dae_plan_in& base, int B)
{
    const dae_score_plan p0 = dae_plan_topk(base);             // the defaults: own_tau = false, B = 0
    if (p0.live_in_tau) fail("live_in_tau with the default own_tau", base);
    const std::vector<long long> w0 = words(p0);
    for (int own = 0; own < 2; ++own) for (int rows : {0, B}) {
        dae_plan_in in = base;
        in.own_tau = own != 0; in.B = rows;
        const dae_score_plan p = dae_plan_topk(in);
        if (words(p) != w0) fail("a field other than live_in_tau depends on own_tau / B", in);
        const bool wave = dae_tau_wave_per_row(rows, p.ld_g, p.whole_b ? 0 : p.ld_s);
        if (p.live_in_tau && !(p.build_live && in.own_tau && !wave)) fail("live_in_tau without build_live && own_tau && workgroup-per-row", in);
        if (!in.own_tau && p.live_in_tau) fail("live_in_tau with foreign thresholds", in);
        if (p.live_in_tau != (p.build_live && in.own_tau && !wave)) fail("live_in_tau is not the conjunction", in);
        if (p.live_in_tau) ++g_live;
        if (p.build_live && in.own_tau && wave) ++g_wave;
    }
}

long long sweep()
{
    const int Bs[] = {1, 31, 32, 33, 64, 65, 128, 129, 256, 1024, 2048, 4096};
    const int Hps[] = {32, 128, 256, 512};
    const int ks[] = {1, 100, 500, 1024};
    std::set<int> widths;                                  // columns of the image: 1 tile .. 170 000 columns
    for (int t = 1; t <= 72; ++t) widths.insert(t * 32);
    for (int w : {1, 31, 33, 300, 1000, 4095, 4097, 8193, 16384, 17500, 21250, 32768, 42500, 65536, 85000, 100000, 131072, 140000,
                  150001, 170000})
        widths.insert(w);
    for (double w = 2400; w < 170000; w *= 1.13) widths.insert((int)w);
    long long n = 0;
    for (int B : Bs) for (int Hp : Hps) for (int w : widths) for (int k : ks) for (int dt = 0; dt < 3; ++dt)
    for (int mixed = 0; mixed < 2; ++mixed) for (int ov = 0; ov < 2; ++ov) for (int col_lo : {0, 21250})
    for (int prefix = 0; prefix < 4; ++prefix) for (int ub = 0; ub < (dt == 0 ? 2 : 1); ++ub) for (int skip = 0; skip < (dt == 0 ? 2 : 1); ++skip) {
        const int n_tracks = prefix == 0 ? col_lo + w : prefix == 1 ? col_lo + (int)((long long)w * 14 / 17)
                           : prefix == 2 ? col_lo + (w < 4000 ? (w + 1) / 2 : 2000 + w / 64) : col_lo;
        const dae_rowgeom g = dt == DAE_DTYPE_F32 ? dae_row_geometry(B, Hp) : dae_row_geometry_bf16(B, Hp);
        const dae_plan_in in{(w + 31) / 32, col_lo, col_lo + w, Hp, ub != 0, g, n_tracks, k, dt, mixed != 0, ov, skip};
        check(in, B);
        ++n;
    }
    return n;
}

}  // namespace

int main()
{
    // the predicate itself, at its three edges (tau_select.hip launch_tau_select: many short rows take a wave per row)
    if (!dae_tau_wave_per_row(1024, 2048, 2048) || dae_tau_wave_per_row(1023, 2048, 2048) || dae_tau_wave_per_row(1024, 2049, 2048) ||
        dae_tau_wave_per_row(1024, 2048, 2052) || !dae_tau_wave_per_row(4096, 1, 0)) {
        printf("FAILED: dae_tau_wave_per_row\n");
        return 1;
    }
    const long long n = sweep();
    printf("sweep: %lld shapes, live_in_tau in %lld plans, build_live behind the wave-per-row kernel in %lld\n", n, g_live, g_wave);
    if (g_live == 0) { printf("FAILED: the sweep never reaches live_in_tau\n"); return 1; }
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("all checks passed\n");
    return 0;
}
