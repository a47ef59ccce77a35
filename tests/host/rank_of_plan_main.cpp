// rank_of_plan_main.cpp -- drives csrc/rank_of_plan.h (the geometry of a dae_decode_rank_of call) as a stand-alone program:
// no device, no HIP.  For a sweep of (rows, hidden size, answers) the chosen geometry fits the CU's LDS beside nothing else
// (the counting kernel has no static LDS), the grid covers every row, and every answer of every row lands in exactly one pass.
// The LDS image of one workgroup is laid out in a heap block of exactly the planned size and every slot is touched, so a
// sanitized build sees a plan that overruns it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rank_of_plan.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); ++g_fail; } \
    } while (0)

static unsigned g_rng = 12345u;
static unsigned rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

// the LDS image as rank_of_count_kernel lays it out: hidden tile | thresholds (8 bytes) | counters | lengths | offsets
static void touch_lds_image(const dae_ro_plan& p)
{
    std::vector<unsigned char> lds(p.lds_bytes);
    unsigned char* base = lds.data();
    const size_t tile = (size_t)p.R_TILE * p.Hp * 4;
    CHECK(tile == (size_t)(p.R_TILE / 32) * 64 * p.G * 16, "hidden tile %zu vs the packed image's", tile);
    memset(base, 1, tile);
    unsigned long long* thr = reinterpret_cast<unsigned long long*>(base + tile);
    CHECK(tile % 16 == 0, "thresholds misaligned");
    unsigned* cnt = reinterpret_cast<unsigned*>(thr + (size_t)p.R_TILE * p.C);
    int* len = reinterpret_cast<int*>(cnt + (size_t)p.R_TILE * p.C);
    int* beg = len + p.R_TILE;
    for (int i = 0; i < p.R_TILE; ++i) {
        for (int t = 0; t < p.C; ++t) { thr[(size_t)i * p.C + t] = ~0ull; cnt[(size_t)i * p.C + t] = 0u; }
        len[i] = p.C; beg[i] = i;
    }
    CHECK(reinterpret_cast<unsigned char*>(beg + p.R_TILE) == base + p.lds_bytes, "the layout does not end at lds_bytes");
}

static void check_plan(int B, int H, long long n_ans, const std::vector<int>& row_len)
{
    const dae_ro_plan p = dae_plan_rank_of(B, H, n_ans);
    CHECK(p.C >= 1, "no plan for B=%d H=%d", B, H);
    if (p.C < 1) return;
    CHECK(p.R_TILE == 128 || p.R_TILE == 64 || p.R_TILE == 32, "R_TILE=%d", p.R_TILE);
    CHECK(p.Hp % 32 == 0 && p.Hp >= H && p.Hp < H + 32 && p.G * 8 == p.Hp && p.G % 4 == 0, "Hp=%d G=%d for H=%d", p.Hp, p.G, H);
    CHECK(p.lds_bytes == dae_rank_of_lds(p.R_TILE, p.Hp, p.C), "lds_bytes");
    CHECK(p.lds_bytes + DAE_RO_LDS_RESERVE <= (size_t)DAE_RO_LDS_BYTES, "B=%d H=%d: %zu bytes of LDS", B, H, p.lds_bytes);
    CHECK(p.C <= DAE_RO_MAX_C, "C=%d beyond the sorting launch's chunk", p.C);
    CHECK(p.n_rg * p.R_TILE >= B && (p.n_rg - 1) * p.R_TILE < B, "row groups %d x %d for %d rows", p.n_rg, p.R_TILE, B);
    CHECK(p.nb_rg >= DAE_RO_NUM_XCD && p.nb_rg % DAE_RO_NUM_XCD == 0 && p.grid == p.n_rg * p.nb_rg, "grid");
    // one more answer per pass would not fit (unless the chunk limit binds)
    CHECK(p.C == DAE_RO_MAX_C || dae_rank_of_lds(p.R_TILE, p.Hp, p.C + 1) + DAE_RO_LDS_RESERVE > (size_t)DAE_RO_LDS_BYTES,
          "C=%d is not the capacity", p.C);
    touch_lds_image(p);
    // every answer of every row in exactly one pass, every pass within the capacity, as the kernel's loop walks them:
    // pass q of a row of `len` answers holds positions [q C, min(len, (q + 1) C))
    int longest = 0;
    for (int len : row_len) longest = len > longest ? len : longest;
    for (int len : row_len) {
        std::vector<int> seen(len, 0);
        const int passes = dae_rank_of_passes(len, p.C);
        for (int q = 0; q * p.C < longest; ++q) {                 // (the launch walks the group's longest row)
            int n = len - q * p.C;
            n = n < 0 ? 0 : (n > p.C ? p.C : n);
            CHECK((n > 0) == (q < passes), "len=%d C=%d pass %d holds %d", len, p.C, q, n);
            for (int t = 0; t < n; ++t) {
                const int i = q * p.C + t;
                CHECK(dae_rank_of_pass(i, p.C) == q, "answer %d in pass %d", i, q);
                ++seen[i];
            }
        }
        for (int i = 0; i < len; ++i) CHECK(seen[i] == 1, "len=%d C=%d: answer %d taken %d times", len, p.C, i, seen[i]);
    }
}

int main()
{
    const int Bs[] = {1, 2, 31, 32, 33, 37, 40, 63, 64, 65, 127, 128, 129, 256, 257, 1000, 4095, 4096};
    const int Hs[] = {4, 36, 64, 100, 128, 256, 260, 512, 1000, 1024};
    const int Ls[] = {0, 1, 2, 19, 20, 21, 100, 125, 126, 127, 250, 600, 5000};
    int n = 0;
    for (int B : Bs)
        for (int H : Hs)
            for (int L : Ls) {
                // rows of every length around the average and the plan's own capacity
                std::vector<int> rows = {0, 1, L, L + 1, 3 * L + 5, (int)(rnd() % (unsigned)(2 * L + 2))};
                const dae_ro_plan p = dae_plan_rank_of(B, H, (long long)L * B);
                if (p.C > 0) { rows.push_back(p.C); rows.push_back(p.C + 1); rows.push_back(3 * p.C + 5); rows.push_back(p.C - 1); }
                check_plan(B, H, (long long)L * B, rows);
                ++n;
            }
    // the shapes the header names
    {
        const dae_ro_plan a = dae_plan_rank_of(256, 256, 256 * 10), b = dae_plan_rank_of(256, 256, 256 * 100);
        CHECK(a.R_TILE == 128 && a.C == 20, "hidden 256, 10 answers: %d rows, C=%d", a.R_TILE, a.C);
        CHECK(b.R_TILE == 64 && b.C >= 100 && b.passes_hint == 1, "hidden 256, 100 answers: %d rows, C=%d", b.R_TILE, b.C);
    }
    // refused sizes
    CHECK(dae_plan_rank_of(0, 256, 10).C == 0 && dae_plan_rank_of(4097, 256, 10).C == 0, "B out of range gets a plan");
    CHECK(dae_plan_rank_of(8, 0, 10).C == 0 && dae_plan_rank_of(8, 1025, 10).C == 0, "H out of range gets a plan");
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("%d plans: all checks passed\n", n);
    return 0;
}
