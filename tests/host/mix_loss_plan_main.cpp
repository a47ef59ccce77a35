// Stand-alone program (no device, no HIP): the panel walk and the scratch carve-up of dae_mix_loss_rows,
// csrc/mix_loss_plan.h dae_plan_mix_loss / dae_mixloss_panel / dae_mixloss_geometry, swept over rows, columns and title feature
// widths:
//   1. the panels are ceil(B / 256), hold at most 256 rows each, follow each other without gap or overlap and cover [0, B);
//   2. a panel's first row keeps a hidden row and a feature row 16-byte aligned (r0 * H * 4 and r0 * ld_feat * 4 bytes);
//   3. the term section holds every panel's [V][nb] buffer and is 4 * V32 * min(B, 256) bytes, whatever B;
//   4. the partial table holds every panel's [n_rg][nb_rg][R_TILE] table, and a row's workgroups are at most 256 (the finishing
//      kernel keeps them in 256 LDS slots);
//   5. every section lies inside the allocation, starts on a multiple of 256 bytes, and no two overlap; the row section is B
//      floats or absent;
//   6. what is written through the offsets stays inside a buffer of `total` bytes (the sanitizer build's part);
//   7. bad arguments give total == 0.
// Exits 0 and prints "all checks passed".  Meant to be built with -fsanitize=address,undefined as well.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mix_loss_plan.h"

namespace {

int g_failed = 0;

void fail(const std::string& what)
{
    if (++g_failed <= 20) printf("FAILED: %s\n", what.c_str());
}

struct Sec { const char* name; size_t off, bytes; };

void check(int B, int V, int Hp, bool want_rows)
{
    const dae_mixloss_plan p = dae_plan_mix_loss(B, V, Hp, want_rows);
    char at[160];
    snprintf(at, sizeof(at), " (B=%d V=%d Hp=%d rows=%d)", B, V, Hp, (int)want_rows);
    auto bad = [&](const char* what) { fail(std::string(what) + at); };
    if (p.total == 0) { bad("a valid call has no plan"); return; }
    // 1., 2. the panel walk
    if (p.n_panels != (B + 255) / 256) bad("the panel count is not ceil(B / 256)");
    if (p.panel_rows != std::min(B, 256)) bad("the largest panel is not min(B, 256) rows");
    int next = 0;
    size_t part_need = 0;
    for (int i = 0; i < p.n_panels; ++i) {
        int r0, nb;
        dae_mixloss_panel(B, i, &r0, &nb);
        if (r0 != next) bad("a panel does not start where the one before it ended");
        if (nb < 1 || nb > DAE_MIXLOSS_PANEL || nb > p.panel_rows) bad("a panel's row count");
        if (i + 1 < p.n_panels && nb != DAE_MIXLOSS_PANEL) bad("a panel that is not the last is short");
        // 2. the byte offsets of the panel's first hidden row and feature row, at the widths the call admits (H % 32 == 0,
        // ld_feat % 4 == 0, each at most 1024) and at the odd multiples of 4 among them
        for (int H = 32; H <= DAE_MIXLOSS_MAXH; H += 32)
            if (((size_t)r0 * H * sizeof(float)) % 16) bad("a panel's first hidden row is misaligned");
        for (int ld = 4; ld <= DAE_MIXLOSS_MAXH; ld += (ld < 64 ? 4 : 60))
            if (((size_t)r0 * ld * sizeof(float)) % 16) bad("a panel's first feature row is misaligned");
        next = r0 + nb;
        // 3. the panel's term buffer [V][nb]
        if ((size_t)V * nb * sizeof(float) > p.term_bytes) bad("a panel's term buffer leaves the term section");
        // 4. its partial table
        const dae_rowgeom g = dae_mixloss_geometry(nb, Hp);
        if (g.R_TILE != 32 && g.R_TILE != 64 && g.R_TILE != 128) bad("a row-group height the kernel is not instantiated for");
        if (g.n_rg * g.R_TILE < nb || g.grid != g.n_rg * g.nb_rg) bad("the geometry does not cover the panel");
        if (g.nb_rg < 1 || g.nb_rg > 256) bad("more workgroups per row group than the finishing kernel's 256 slots");
        if ((size_t)g.R_TILE * Hp * 4 > 128 * 1024) bad("the hidden tile leaves its 128 KiB of LDS");
        part_need = std::max(part_need, (size_t)g.grid * g.R_TILE);
    }
    if (next != B) bad("the panels do not cover [0, B)");
    int r0, nb;
    dae_mixloss_panel(B, p.n_panels, &r0, &nb);
    if (nb != 0) bad("a panel behind the last holds rows");
    if (p.V32 % 32 || p.V32 < (size_t)V || p.V32 >= (size_t)V + 32) bad("V32 is not V rounded up to 32");
    if (p.term_bytes != 4 * p.V32 * (size_t)p.panel_rows) bad("the term section is not 4 * V32 * min(B, 256) bytes");
    if (p.part_floats != part_need) bad("the partial table is not the largest panel's");
    if (p.row_floats != (want_rows ? (size_t)B : 0)) bad("the row section");
    // 5. the sections
    const std::vector<Sec> secs = {{"term", p.o_term, p.term_bytes}, {"part", p.o_part, p.part_floats * 4}, {"rows", p.o_rows, p.row_floats * 4}};
    size_t sum = 0;
    for (const Sec& s : secs) {
        if (s.off % DAE_MIXLOSS_ALIGN) bad((std::string(s.name) + " is misaligned").c_str());
        if (s.off + s.bytes > p.total) bad((std::string(s.name) + " leaves the allocation").c_str());
        sum += s.bytes;
    }
    for (size_t i = 0; i + 1 < secs.size(); ++i)
        if (secs[i].off + secs[i].bytes > secs[i + 1].off) bad((std::string(secs[i].name) + " overlaps " + secs[i + 1].name).c_str());
    if (p.total < sum || p.total > sum + 3 * DAE_MIXLOSS_ALIGN) bad("the total is not the sum of the sections");
    // 6. write every section through its offset into a buffer of exactly `total` bytes, each with a value of its own, read back
    if (p.total <= (size_t)1 << 24) {
        std::vector<unsigned char> buf(p.total, 0);
        for (size_t i = 0; i < secs.size(); ++i) memset(buf.data() + secs[i].off, (int)(i + 1), secs[i].bytes);
        for (size_t i = 0; i < secs.size(); ++i)
            for (size_t b = 0; b < secs[i].bytes; b += std::max<size_t>(1, secs[i].bytes / 7))
                if (buf[secs[i].off + b] != (unsigned char)(i + 1)) { bad("a section was overwritten by another"); break; }
    }
}

long long sweep()
{
    const int Bs[] = {1, 2, 31, 32, 33, 64, 65, 96, 128, 129, 150, 255, 256, 257, 300, 511, 512, 513, 1024, 1025, 4095, 4096};
    const int Vs[] = {1, 31, 32, 33, 2003, 170000, 2262292};
    const int Hps[] = {32, 64, 96, 256, 288, 448, 512, 544, 1024};
    long long n = 0;
    for (int B : Bs) for (int V : Vs) for (int Hp : Hps) for (int w = 0; w < 2; ++w) { check(B, V, Hp, w != 0); ++n; }
    return n;
}

void fixed_points()
{
    // the issue's figure: 174 MB of term buffer at V = 170 000, for 256 rows and for 1 024 alike
    const dae_mixloss_plan a = dae_plan_mix_loss(256, 170000, 448, false), b = dae_plan_mix_loss(1024, 170000, 448, false);
    if (a.term_bytes != (size_t)4 * 170016 * 256 || b.term_bytes != a.term_bytes) fail("the term buffer at V = 170 000");
    if (a.n_panels != 1 || b.n_panels != 4) fail("the panel counts at 256 and 1 024 rows");
    // ld_feat 448: 64-row groups, four of them a full panel, 64 workgroups each
    const dae_rowgeom g = dae_mixloss_geometry(256, 448);
    if (g.R_TILE != 64 || g.n_rg != 4 || g.nb_rg != 64) fail("the geometry of a full panel at ld_feat 448");
    const dae_mixloss_plan c = dae_plan_mix_loss(300, 2003, 448, true);
    int r0, nb;
    dae_mixloss_panel(300, 1, &r0, &nb);
    if (c.n_panels != 2 || r0 != 256 || nb != 44) fail("300 rows are 256 + 44");
}

void bad_arguments()
{
    if (dae_plan_mix_loss(0, 10, 64, false).total) fail("B = 0 has a plan");
    if (dae_plan_mix_loss(4097, 10, 64, false).total) fail("B = 4097 has a plan");
    if (dae_plan_mix_loss(4, 0, 64, false).total) fail("V = 0 has a plan");
    if (dae_plan_mix_loss(4, 10, 0, false).total) fail("Hp = 0 has a plan");
    if (dae_plan_mix_loss(4, 10, 48, false).total) fail("Hp = 48 has a plan");
    if (dae_plan_mix_loss(4, 10, 1056, false).total) fail("Hp = 1056 has a plan");
}

}  // namespace

int main()
{
    const long long n = sweep();
    printf("sweep: %lld plans\n", n);
    fixed_points();
    bad_arguments();
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("all checks passed\n");
    return 0;
}
