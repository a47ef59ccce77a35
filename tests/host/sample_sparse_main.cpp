// Stand-alone program (no device, no HIP): the decoded-tile table of the half-row-group sample (csrc/score_plan.h
// dae_sample_item_slot and its inverse: the ONE mapping decode_f32_kernel's HALF writes by and tau_select_kernel reads by;
// DESIGN.md section 4).  Over every (n_samp, nb_rg) the plan gives a sample that may skip:
//   1. every item below n_samp maps to a (word, byte) of its own with word < nb_rg and byte < 4, and back;
//   2. the writer's walk -- workgroup bir, wave w holds item dae_sample_slot_item(bir, w, nb_rg) and marks byte w of word bir only
//      where that item exists -- marks exactly the items below n_samp when nothing is skipped, so no item >= n_samp is ever marked;
//   3. the reader's walk -- float4 f of a row's dense sample belongs to item f >> 3, maximum i to word i >> 5 -- stays inside the
//      table, inside the bytes the threshold kernel spreads out in LDS (32 per key register of a thread) and sees every marked item;
//   4. the table of a launch fits the words reserved behind the sample's counters.
// Exits 0 and prints "all checks passed".  Meant to be built with -fsanitize=address,undefined as well.
#include <stdio.h>
#include <string.h>

#include <set>
#include <string>
#include <utility>
#include <vector>

#include "score_plan.h"

namespace {

int g_failed = 0;

void fail(const std::string& what)
{
    if (++g_failed <= 20) printf("FAILED: %s\n", what.c_str());
}

constexpr int SSKIP_SLOTS = 2 * DAE_NUM_CU;      // csrc/dae_internal.h DAE_SSKIP_SLOTS (a HIP header: restated)

void check_shape(int n_samp, int nb_rg, int n_rg, int64_t ld_g)
{
    char tag[96];
    snprintf(tag, sizeof(tag), " (n_samp %d, nb_rg %d, n_rg %d)", n_samp, nb_rg, n_rg);
    // the threshold kernel's shape for rows of ld_g maxima: TAU_PER key registers per thread, 8 words and 32 item bytes each
    const int per = ld_g <= 256 * 16 ? 16 : ld_g <= 256 * 32 ? 32 : 64;
    if (per > 32) fail(std::string("a sample with a table takes the 64-key threshold kernel") + tag);
    if (ld_g != (int64_t)nb_rg * 32) fail(std::string("maxima per row != 32 per table word") + tag);
    if (nb_rg > 256 || nb_rg > 8 * per || 4 * nb_rg > 32 * per) fail(std::string("the table of a half group does not fit the kernel's LDS copy") + tag);
    // 1. items -> slots
    std::set<std::pair<int, int>> seen;
    for (int item = 0; item < n_samp; ++item) {
        const dae_samp_slot s = dae_sample_item_slot(item, nb_rg);
        if (s.word < 0 || s.word >= nb_rg || s.byte < 0 || s.byte >= 4) fail(std::string("slot out of range") + tag);
        if (!seen.insert({s.word, s.byte}).second) fail(std::string("two items share a slot") + tag);
        if (dae_sample_slot_item(s.word, s.byte, nb_rg) != item) fail(std::string("slot -> item is not the inverse") + tag);
    }
    // 2. the writer: one word per workgroup, byte w = wave w's item, marked where the item exists (nothing skipped)
    std::vector<uint32_t> tab(nb_rg, 0u);
    for (int bir = 0; bir < nb_rg; ++bir)
        for (int w = 0; w < 4; ++w) {
            const int item = dae_sample_slot_item(bir, w, nb_rg);
            if (item < n_samp) tab[bir] |= 1u << (8 * w);
        }
    std::vector<unsigned char> marked(4 * (size_t)nb_rg, 0);      // the reader's LDS bytes, spread out as the kernel does
    for (int t = 0; t < nb_rg; ++t)
        for (int b = 0; b < 4; ++b) marked[dae_sample_slot_item(t, b, nb_rg)] = (unsigned char)((tab[t] >> (8 * b)) & 0xFFu);
    for (int item = 0; item < 4 * nb_rg; ++item)
        if ((marked[item] != 0) != (item < n_samp)) fail(std::string(item < n_samp ? "a decoded item is not marked" : "an item >= n_samp is marked") + tag);
    // 3. the reader
    const int n4 = n_samp * 8;
    for (int f = 0; f < n4; ++f) {
        const int item = dae_sample_f4_item(f);
        if (item != f >> 3 || item < 0 || item >= n_samp || item >= 4 * nb_rg) fail(std::string("float4 -> item") + tag);
        const dae_samp_slot s = dae_sample_item_slot(item, nb_rg);
        if (((tab[s.word] >> (8 * s.byte)) & 0xFFu) != marked[item]) fail(std::string("the spread bytes disagree with the words") + tag);
    }
    for (int64_t i = 0; i < ld_g; ++i)
        if ((i >> 5) >= nb_rg) fail(std::string("a maximum without a table word") + tag);
    // 4. the launch's table: word (half group, workgroup) of [2 n_rg][nb_rg] lies inside the reserved words
    for (int hg = 0; hg < 2 * n_rg; ++hg)
        if ((size_t)hg * nb_rg + (nb_rg - 1) >= (size_t)SSKIP_SLOTS) fail(std::string("a table word behind the reserved ones") + tag);
}

}  // namespace

int main()
{
    // the sweep of tests/host/sample_skip_main.cpp: every plan whose sample may skip
    const int Bs[] = {1, 32, 64, 65, 128, 129, 130, 192, 256, 257, 512, 1024, 4096};
    const int Hps[] = {32, 128, 224, 256, 512};
    const int ks[] = {1, 100, 500, 1024, 1025, 2048, 4096};
    const int widths[] = {32, 2048, 8000, 16384, 36000, 65536, 100000, 170000, 300000};
    long long n = 0, n_tab = 0;
    std::set<std::pair<int, int>> shapes;
    for (int B : Bs) for (int Hp : Hps) for (int w : widths) for (int k : ks) for (int part = 0; part < 2; ++part) for (int own = 0; own < 2; ++own) {
        const int n_tracks = part ? (int)((long long)w * 14 / 17) : w;
        const dae_rowgeom g = dae_row_geometry(B, Hp);
        const dae_plan_in in{(w + 31) / 32, 0, w, Hp, true, g, n_tracks, k, DAE_DTYPE_F32, false, 0, 1, own != 0, B};
        const dae_score_plan p = dae_plan_topk(in);
        ++n;
        if (!p.sample_skip || 2 * g.grid > SSKIP_SLOTS) continue;           // (score.hip topk_phase_a: the launch skips only then)
        if (dae_tau_wave_per_row(B, p.ld_g, p.ld_s)) continue;             // (the wave-per-row kernel keeps the dense exchange: no table)
        ++n_tab;
        shapes.insert({p.n_samp, g.nb_rg});
        check_shape(p.n_samp, g.nb_rg, g.n_rg, p.ld_g);
    }
    // ... and around them: every n_samp of one round for the workgroup counts the geometry can give
    for (int nb_rg = 8; nb_rg <= 256; nb_rg += 8)
        for (int n_samp : {1, 2, nb_rg - 1, nb_rg, nb_rg + 1, 2 * nb_rg + 5, 3 * nb_rg, 4 * nb_rg - 1, 4 * nb_rg})
            check_shape(n_samp, nb_rg, 1, (int64_t)nb_rg * 32);
    check_shape(469, 128, 2, 4096);                                        // tests/test_gpu_sample_sparse.py at 130 / 256 rows
    check_shape(469, 256, 1, 8192);                                        // ... at 65
    check_shape(487, 128, 2, 4096);                                        // bench.py's headline
    if (n_tab == 0) fail("the sweep never met a plan with a table");
    printf("plans: %lld, %lld with a decoded-tile table, %zu distinct (n_samp, nb_rg)\n", n, n_tab, shapes.size());
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("all checks passed\n");
    return 0;
}
