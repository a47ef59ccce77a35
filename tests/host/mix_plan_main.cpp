// Stand-alone program (no device, no HIP): the plan of an exact title-mix call, csrc/mix_plan.h dae_plan_mix.
//   1. against tests/golden/mix_plans.txt (argv[1]): one line per branch of the plan, inputs | expected words.  The table was
//      written by the launch arithmetic of dae_mix_topk_exact_impl as it stood inline in mixexact.hip, before it became this
//      function.
//   2. over a grid of shapes, the conditions the kernels rely on (mixexact.hip reserves and launches by the plan unchecked),
//      each read from the kernel code: mix_filter.hip for the row groups, LDS, claiming and segments, mix_refine.hip for the
//      segment table and the fused selection.
// Exits 0 and prints "all checks passed".  Meant to be built with -fsanitize=address,undefined as well.
#include <stdio.h>
#include <string.h>

#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "mix_plan.h"

namespace {

int g_failed = 0;

void fail(const std::string& what)
{
    if (++g_failed <= 20) printf("FAILED: %s\n", what.c_str());
}

std::vector<long long> words(const dae_mix_plan& p)
{
    std::vector<long long> w = {p.status, p.shipped, p.NSD, p.NST, p.RB, p.R_TILE, p.n_rg, p.Bpad, p.nb, p.grid, p.n_valid_col, p.ntr,
                                p.n_samp, p.nb_s, p.ld_s, p.cap, (long long)p.lds_bytes, (long long)p.lds_attr, p.fuse};
    for (int i = 0; i < 8; ++i) w.push_back(p.last[i]);
    return w;
}

int check_table(const char* path, std::set<std::string>& names)
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
        if (in.size() != 9 || want.size() != 27) { fail(name + ": malformed line"); continue; }
        const dae_mix_plan_in pi{(int)in[0], (int)in[1], (int)in[2], (int)in[3], (int)in[4], (int)in[5], (int)in[6], (int)in[7], (int)in[8]};
        const std::vector<long long> got = words(dae_plan_mix(pi));
        if (got != want) {
            std::string s = name + ": got";
            for (long long x : got) s += " " + std::to_string(x);
            fail(s);
        }
        names.insert(name.substr(name.find('_') + 1));
        ++n;
    }
    fclose(f);
    return n;
}

// what mixexact.hip and the kernels take for granted of any plan
void check_invariants(const dae_mix_plan_in& in, const dae_mix_plan& p)
{
    auto bad = [&](const char* what) {
        char b[256];
        snprintf(b, sizeof(b), "%s (HD=%d/%d HT=%d/%d col_hi=%d B=%d k=%d n_tracks=%d overlap=%d)", what, in.HD, in.HpD, in.HT, in.HpT,
                 in.col_hi, in.B, in.k, in.n_tracks, in.overlap_hint);
        fail(b);
    };
    const bool shape = (in.HpD == 256 && in.HpT == 448 && in.HD == in.HpD && in.HT % 16 == 0) || dae_mix_shape_ok(in.HD, in.HT);
    const int nvc = in.n_tracks < in.col_hi ? in.n_tracks : in.col_hi;
    const int want_status = !shape ? DAE_MIX_BAD_SHAPE : in.B <= 0 ? DAE_MIX_NO_ROWS : in.B > 4096 ? DAE_MIX_TOO_MANY_ROWS
                          : nvc <= 0 ? DAE_MIX_NO_COLUMN : DAE_MIX_OK;
    if (p.status == DAE_MIX_TOO_MANY_SEGMENTS) { if (p.nb <= MR_MAX_SEG) bad("segments refused"); return; }
    if (p.status != want_status) bad("status");
    if (p.status != DAE_MIX_OK) return;
    const int NS = p.NSD + p.NST;
    // the instance and its LDS (mix_filter.hip: mix_lds_tail, the staging loops; dae_launch_mix_pass)
    if (!(p.RB == 2 || p.RB == 3) || p.R_TILE != 32 * p.RB || p.R_TILE > 512) bad("RB / R_TILE (one thread per row)");
    if (p.NSD != in.HpD / 16 || p.NST != in.HpT / 16) bad("NSD / NST");
    if (p.lds_bytes != (size_t)p.RB * 64 * NS * 16 + (size_t)p.R_TILE * 8 + 16) bad("lds_bytes");
    if (p.lds_bytes > p.lds_attr || p.lds_attr > 160 * 1024) bad("lds_bytes <= lds_attr <= 160 KiB");
    if (p.shipped && !(p.NSD == 16 && p.NST == 28 && p.RB == 3)) bad("shipped instance");
    if (!p.shipped && !(p.NSD >= 8 && p.NSD % 4 == 0 && p.NST >= 4 && p.NST % 4 == 0)) bad("steps instance: eight DAE steps, chunks of 4");
    // row groups and workgroups (mix_block_map; the refine launch's segment table)
    if (p.n_rg != (in.B + p.R_TILE - 1) / p.R_TILE || p.Bpad != p.n_rg * p.R_TILE) bad("n_rg / Bpad");
    if (p.nb % 8 != 0 || p.nb < 8 || p.nb > MR_MAX_SEG) bad("nb");
    if (p.grid != p.n_rg * p.nb) bad("grid");
    if (p.n_valid_col != nvc || p.ntr != (nvc + 31) / 32) bad("n_valid_col / ntr");
    if (!(p.nb == 8 || (p.nb - 8) * 8 < p.ntr)) bad("workgroups without a tile");
    // a workgroup walks the items congruent to its index mod nb, by position or by claim; each adds at most 32 entries to a row
    if (p.cap < 32 * ((p.ntr + p.nb - 1) / p.nb)) bad("cap");
    // the sample
    if (p.n_samp > p.ntr || p.n_samp < (p.ntr < 256 ? p.ntr : 256) || p.ld_s != 8 * (int64_t)p.n_samp) bad("n_samp / ld_s");
    if (p.nb_s % 8 != 0 || p.nb_s < 8 || p.nb_s > p.nb) bad("nb_s");
    if (!in.overlap_hint && p.nb_s != p.nb) bad("nb_s without the hint");
    // the fused selection: k within half the ordering stage, the seed bitmap behind its keys (mix_refine.hip)
    if (p.fuse != (in.k <= MR_RANK_MAX / 2 && (nvc + 31) / 32 + 2 * MR_RANK_MAX <= MR_STAGE)) bad("fuse");
    const int32_t want[8] = {p.R_TILE, p.n_rg, p.nb, 1, p.n_samp, p.ntr, 0, p.ntr};
    if (memcmp(want, p.last, sizeof(want)) != 0) bad("last[8]");
}

long long sweep()
{
    const int Bs[] = {1, 31, 32, 33, 64, 65, 96, 97, 150, 192, 193, 256, 750, 1024, 4096};
    const int ks[] = {1, 100, 500, 512, 513, 1024};
    std::set<int> cols;                                    // rankable columns: 1 tile .. 200 000, both sides of the multiples of 32
    for (int c = 1; c <= 130; ++c) cols.insert(c);
    for (int c = 199900; c <= 200000; ++c) cols.insert(c);
    for (double w = 150; w < 200000; w *= 1.09)
        for (int d = -1; d <= 1; ++d) { cols.insert((int)w / 32 * 32 + d); cols.insert((int)w); }
    for (int t : {63, 64, 256, 257, 2047, 2048, 2049, 4375, 6143, 6144, 6145})      // tiles: the sample's and the bitmap's thresholds
        for (int d = -1; d <= 1; ++d) cols.insert(t * 32 + d);
    long long n = 0;
    for (int B : Bs) for (int HD = 128; HD <= 512; HD += 64) for (int HT = 64; HT <= 512; HT += 64) for (int c : cols) for (int k : ks)
    for (int ov = 0; ov < 2; ++ov) {
        // the ranked columns: all of the image, or the shipped 14 / 17 of it
        const dae_mix_plan_in in{HD, (HD + 31) / 32 * 32, HT, (HT + 31) / 32 * 32, ov ? c : c + c * 3 / 14, B, k, c, ov};
        check_invariants(in, dae_plan_mix(in));
        ++n;
    }
    // the refusals' edges
    for (int HD : {0, 64, 96, 160, 256, 576}) for (int HT : {0, 32, 96, 400, 432, 448, 576}) for (int B : {-1, 0, 1, 4096, 4097})
    for (int n_tracks : {-5, 0, 1, 2000}) for (int col_hi : {0, 2300}) {
        const dae_mix_plan_in in{HD, (HD + 31) / 32 * 32, HT, (HT + 31) / 32 * 32, col_hi, B, 100, n_tracks, 0};
        check_invariants(in, dae_plan_mix(in));
        ++n;
    }
    return n;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: %s tests/golden/mix_plans.txt\n", argv[0]); return 2; }
    std::set<std::string> names;
    const int n_table = check_table(argv[1], names);
    // one case per branch of the plan
    for (const char* want : {"shipped", "steps_rb3", "steps_rb2", "hint_on", "hint_off", "small_image_nb_shrinks", "n_samp_clamped",
                             "fuse_on", "fuse_off_by_k", "fuse_off_by_bitmap", "refused_shape", "refused_rows", "refused_no_column",
                             "no_rows"})
        if (!names.count(want)) fail(std::string("the table has no case ") + want);
    printf("table: %d plans\n", n_table);
    const long long n_sweep = sweep();
    printf("sweep: %lld plans\n", n_sweep);
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("all checks passed\n");
    return 0;
}
