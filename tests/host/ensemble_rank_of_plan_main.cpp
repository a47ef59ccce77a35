// Stand-alone program (no device, no HIP): the scratch carve-up of dae_ensemble_rank_of / dae_ensemble_candidates,
// csrc/ensemble_rank_of_plan.h dae_plan_ensemble_scratch, swept over scorers, answers, seed slots and row groups (those of
// csrc/rank_of_plan.h dae_plan_rank_of for the rows and hidden sizes of the sweep):
//   1. every section lies inside the allocation, no two overlap, each starts where its alignment asks;
//   2. the buckets and the longest-row words are contiguous and exactly what the memset zeroes;
//   3. the scorers' arrays hold the LARGER pair list each, 16-byte aligned, without overlap; the total is the sum;
//   4. what is written through the offsets stays inside a buffer of `total` bytes (the sanitizer build's part);
//   5. bad arguments give total == 0.
// Exits 0 and prints "all checks passed".  Meant to be built with -fsanitize=address,undefined as well.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ensemble_rank_of_plan.h"
#include "rank_of_plan.h"

namespace {

int g_failed = 0;

void fail(const std::string& what)
{
    if (++g_failed <= 20) printf("FAILED: %s\n", what.c_str());
}

struct Sec { const char* name; size_t off, bytes, align; };

void check(int K, long long n_ans, long long n_seed, int n_rg)
{
    const dae_ens_scratch p = dae_plan_ensemble_scratch(K, n_ans, n_seed, n_rg);
    char at[160];
    snprintf(at, sizeof(at), " (K=%d n_ans=%lld n_seed=%lld n_rg=%d)", K, n_ans, n_seed, n_rg);
    auto bad = [&](const char* what) { fail(std::string(what) + at); };
    if (p.total == 0) { bad("a valid call has no plan"); return; }
    const size_t na = (size_t)n_ans, ns = (size_t)n_seed, np = std::max(na, ns);
    std::vector<Sec> secs = {
        {"thr", p.o_thr, na * 8, 16},       {"z", p.o_z, na * 4, 16},          {"inv", p.o_inv, na * 4, 16},
        {"gcnt", p.o_gcnt, na * 4, 16},     {"glen", p.o_glen, (size_t)n_rg * 4, 4}, {"seed_y", p.o_seed_y, ns * 4, 16},
    };
    for (int k = 0; k < K; ++k) secs.push_back({"s", p.o_s + (size_t)k * p.s_stride * 4, np * 4, 16});
    size_t sum = 0;
    for (const Sec& s : secs) {
        if (s.off % s.align) bad((std::string(s.name) + " is misaligned").c_str());
        if (s.off + s.bytes > p.total) bad((std::string(s.name) + " leaves the allocation").c_str());
        sum += s.bytes;
    }
    std::vector<Sec> by = secs;
    std::sort(by.begin(), by.end(), [](const Sec& a, const Sec& b) { return a.off < b.off || (a.off == b.off && a.bytes < b.bytes); });
    for (size_t i = 0; i + 1 < by.size(); ++i)
        if (by[i].off + by[i].bytes > by[i + 1].off) bad((std::string(by[i].name) + " overlaps " + by[i + 1].name).c_str());
    if (p.o_glen != p.o_gcnt + na * 4) bad("glen does not follow gcnt directly");
    if (p.zero_bytes != na * 4 + (size_t)n_rg * 4) bad("the memset is not gcnt + glen");
    if (p.s_stride < np || p.s_stride % 4) bad("s_stride");
    // the total: no more than the sections and their alignment padding (at most 15 bytes a section, 12 per scorer's array)
    if (p.total < sum || p.total > sum + 16 * 6 + 12 * (size_t)K + 16) bad("the total is not the sum of the sections");
    // write every section through its offset into a buffer of exactly `total` bytes, each with a value of its own, and read back
    if (p.total <= (size_t)1 << 22) {
        std::vector<unsigned char> buf(p.total, 0);
        for (size_t i = 0; i < secs.size(); ++i) memset(buf.data() + secs[i].off, (int)(i + 1), secs[i].bytes);
        for (size_t i = 0; i < secs.size(); ++i)
            for (size_t b = 0; b < secs[i].bytes; b += std::max<size_t>(1, secs[i].bytes / 7))
                if (buf[secs[i].off + b] != (unsigned char)(i + 1)) { bad("a section was overwritten by another"); break; }
    }
}

long long sweep()
{
    const int Ks[] = {1, 2, 3, 4, 5, 9, 17};
    const long long ans[] = {0, 1, 2, 3, 4, 5, 7, 8, 19, 20, 21, 125, 126, 255, 256, 257, 2570, 64250, 1000003};
    const long long seeds[] = {0, 1, 3, 4, 5, 250, 257, 25700, 2000001};
    const int Bs[] = {1, 5, 37, 128, 129, 257, 4096};
    const int Hs[] = {64, 96, 256, 320, 448, 1024};
    long long n = 0;
    for (int K : Ks) for (long long na : ans) for (long long ns : seeds) for (int B : Bs) for (int H : Hs) {
        const dae_ro_plan pl = dae_plan_rank_of(B, H, na);
        if (pl.C <= 0) continue;
        check(K, na, ns, pl.n_rg);
        ++n;
    }
    // the candidate call alone: no seeds, no row groups
    for (int K : Ks) for (long long na : ans) { check(K, na, 0, 0); ++n; }
    return n;
}

void bad_arguments()
{
    if (dae_plan_ensemble_scratch(0, 1, 1, 1).total) fail("K = 0 has a plan");
    if (dae_plan_ensemble_scratch(1, -1, 1, 1).total) fail("n_ans < 0 has a plan");
    if (dae_plan_ensemble_scratch(1, 1, -1, 1).total) fail("n_seed < 0 has a plan");
    if (dae_plan_ensemble_scratch(1, 1, 1, -1).total) fail("n_rg < 0 has a plan");
}

}  // namespace

int main()
{
    const long long n = sweep();
    printf("sweep: %lld carve-ups\n", n);
    bad_arguments();
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("all checks passed\n");
    return 0;
}
