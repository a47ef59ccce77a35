// Stand-alone program (no device, no HIP): the plan of a ranking call, csrc/score_plan.h dae_plan_topk.
//   1. against tests/golden/score_plans.txt (argv[1]): one line per branch of the plan, inputs | expected words.  The table was
//      written by the planning arithmetic of topk_phase_a / _b as it stood inline in api.hip, before it became this function.
//   2. over a grid of shapes, the conditions the launches rely on (score.hip reserves and launches by the plan unchecked).
// Exits 0 and prints "all checks passed".  Meant to be built with -fsanitize=address,undefined as well.
#include <stdio.h>
#include <string.h>

#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "score_plan.h"

namespace {

int g_failed = 0;

void fail(const std::string& what)
{
    if (++g_failed <= 20) printf("FAILED: %s\n", what.c_str());
}

std::vector<long long> words(const dae_score_plan& p)
{
    std::vector<long long> w = {p.bad_mix, p.dtype, p.exact, p.mixed, p.n_valid_col, p.nrank, p.ntiles, p.S, p.n_samp, p.n_other,
                                p.fused, p.gA.R_TILE, p.gA.n_rg, p.gA.Bpad, p.gA.nb_rg, p.gA.grid, p.gA.waves, p.wave_groups,
                                p.use_band, p.ld_s, p.ld_g, p.gmax_per_wave, p.whole_b, p.n_filter, p.cap, p.build_live};
    for (int i = 0; i < 8; ++i) w.push_back(p.last[i]);
    return w;
}

int check_table(const char* path)
{
    FILE* f = fopen(path, "r");
    if (!f) { printf("cannot open %s\n", path); return -1; }
    char line[2048];
    int n = 0;
    while (fgets(line, sizeof(line), f)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        std::istringstream is(line);
        std::string name, bar;
        long long v;
        std::vector<long long> in, want;
        is >> name >> bar;
        while (is >> v) in.push_back(v);
        is.clear(); is >> bar;
        while (is >> v) want.push_back(v);
        if (in.size() != 17 || want.size() != 34) { fail(name + ": malformed line"); continue; }
        dae_plan_in pi{};
        pi.ntiles = (int)in[0]; pi.col_lo = (int)in[1]; pi.col_hi = (int)in[2]; pi.Hp = (int)in[3]; pi.ub_valid = in[4] != 0;
        pi.g = dae_rowgeom{(int)in[5], (int)in[6], (int)in[7], (int)in[8], (int)in[9], (int)in[10]};
        pi.n_tracks = (int)in[11]; pi.k = (int)in[12]; pi.dtype_in = (int)in[13]; pi.mixed = in[14] != 0;
        pi.overlap_hint = (int)in[15]; pi.filter_skip = (int)in[16];
        const std::vector<long long> got = words(dae_plan_topk(pi));
        if (got != want) {
            std::string s = name + ": got";
            for (long long x : got) s += " " + std::to_string(x);
            fail(s);
        }
        ++n;
    }
    fclose(f);
    return n;
}

// what score.hip and the kernels take for granted of any plan
void check_invariants(const dae_plan_in& in, const dae_score_plan& p, const char* tag)
{
    auto bad = [&](const char* what) {
        char b[256];
        snprintf(b, sizeof(b), "%s: %s (ntiles=%d cols=[%d,%d) Hp=%d n_rg=%d n_tracks=%d k=%d dtype=%d mixed=%d overlap=%d)", what, tag,
                 in.ntiles, in.col_lo, in.col_hi, in.Hp, in.g.n_rg, in.n_tracks, in.k, in.dtype_in, (int)in.mixed, in.overlap_hint);
        fail(b);
    };
    const dae_rowgeom& g = in.g;
    if (p.bad_mix) {
        if (!(in.mixed && in.dtype_in == DAE_DTYPE_BF16_EXACT)) bad("bad_mix without exact + mix");
        return;
    }
    if (in.mixed && in.dtype_in == DAE_DTYPE_BF16_EXACT) bad("exact + mix not refused");
    if (p.n_samp + p.n_other != p.ntiles) bad("n_samp + n_other != ntiles");
    if (p.gA.nb_rg % 8 != 0 || p.gA.nb_rg > g.nb_rg || p.gA.nb_rg < 8) bad("gA.nb_rg");
    if (p.gA.grid != p.gA.nb_rg * g.n_rg || p.gA.R_TILE != g.R_TILE || p.gA.n_rg != g.n_rg || p.gA.Bpad != g.Bpad || p.gA.waves != g.waves)
        bad("gA is not g with fewer workgroups");
    if (p.gA.nb_rg != g.nb_rg && !p.wave_groups) bad("gA != g without wave_groups");
    if (p.fused && p.ld_g <= 0) bad("fused with ld_g <= 0");
    if (p.fused && (p.S < 1 || p.n_samp < 1)) bad("fused without a sample");
    if (!p.fused && p.ntiles > 0 && (p.n_samp != p.ntiles || p.S != 1)) bad("unfused: the dense launch walks every ranked tile");
    if (p.ld_s != (int64_t)p.n_samp * 32) bad("ld_s");
    if (p.cap != dae_filter_block_tiles(g, p.n_filter, p.dtype, in.Hp, p.mixed) * 32) bad("cap");
    if (p.n_filter != (p.whole_b ? p.ntiles : p.n_other)) bad("n_filter");
    if (p.build_live && !(p.dtype == DAE_DTYPE_F32 && !p.whole_b && p.n_filter > 0 && in.ub_valid && in.filter_skip)) bad("build_live");
    if (p.wave_groups && (p.use_band || !(p.gmax_per_wave == 3 || p.gmax_per_wave == 4) || p.ld_g != (p.gmax_per_wave == 4 ? 4 : 8) * p.gA.nb_rg * 32))
        bad("wave_groups: gmax shape");
    if (p.wave_groups && !(p.dtype == DAE_DTYPE_BF16 && !p.mixed && in.Hp == 256 && g.R_TILE == 128 && p.whole_b)) bad("wave_groups: kernel shape");
    if (p.whole_b && !(p.fused && p.dtype == DAE_DTYPE_BF16)) bad("whole_b");
    if (p.exact && p.ntiles > 0 && !(p.fused && p.whole_b)) bad("exact mode takes the threshold path, maxima only");
    if (p.ntiles > 0 && p.ld_g < (p.gmax_per_wave == 1 ? p.ld_s : 1)) bad("gmax_per_wave 1 keeps every sample element");
    const int32_t want[8] = {g.R_TILE, g.n_rg, g.nb_rg, p.fused ? p.S : 1, p.n_samp, p.whole_b ? p.ntiles : p.n_other, p.fused ? 1 : 0, p.ntiles};
    if (memcmp(want, p.last, sizeof(want)) != 0) bad("last[8]");
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
    for (int prefix = 0; prefix < 4; ++prefix) for (int ub = 0; ub < (dt == 0 ? 2 : 1); ++ub) {
        // ranked prefix of the image: all of it; the shipped 14 / 17; a short one; none (n_tracks <= col_lo)
        const int n_tracks = prefix == 0 ? col_lo + w : prefix == 1 ? col_lo + (int)((long long)w * 14 / 17)
                           : prefix == 2 ? col_lo + (w < 4000 ? (w + 1) / 2 : 2000 + w / 64) : col_lo;
        const dae_rowgeom g = dt == DAE_DTYPE_F32 ? dae_row_geometry(B, Hp) : dae_row_geometry_bf16(B, Hp);
        const dae_plan_in in{(w + 31) / 32, col_lo, col_lo + w, Hp, ub != 0, g, n_tracks, k, dt, mixed != 0, ov, 1};
        check_invariants(in, dae_plan_topk(in), "sweep");
        ++n;
    }
    return n;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: %s tests/golden/score_plans.txt\n", argv[0]); return 2; }
    const int n_table = check_table(argv[1]);
    if (n_table < 30) { printf("the table holds %d cases\n", n_table); return 1; }
    printf("table: %d plans\n", n_table);
    const long long n_sweep = sweep();
    printf("sweep: %lld plans\n", n_sweep);
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("all checks passed\n");
    return 0;
}
