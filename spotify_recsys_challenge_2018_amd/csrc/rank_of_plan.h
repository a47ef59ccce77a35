// rank_of_plan.h -- how a dae_decode_rank_of call is cut: the row-group height of the counting launch and how many answers of a
// row one pass of the GEMM takes.  Host only and free of HIP, like score_plan.h, so that a plain C++ program can exercise it
// (tests/host/rank_of_plan_main.cpp).  rank_of.hip launches by what dae_plan_rank_of returns.
//
// LDS of a counting workgroup (all of it dynamic; a CU has 160 KiB):
//   the hidden tile             R_TILE x Hp fp32
//   per (row, answer slot)      8 bytes threshold (the composite key, see rank_of.hip) + 4 bytes counter
//   per row                     4 bytes chunk length + 4 bytes chunk offset
// A row with more answers than C takes ceil(len / C) passes; the passes are a loop INSIDE the launch (the longest row of a row
// group is known on the device only), so the plan fixes C and the grid, never a number of launches.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int DAE_RO_LDS_BYTES = 160 * 1024;      // per CU (gfx950)
constexpr int DAE_RO_LDS_RESERVE = 1024;          // left free: alignment, and room for a compiler-made static word or two
constexpr int DAE_RO_SLOT_BYTES = 12;             // threshold + counter of one (row, answer slot)
constexpr int DAE_RO_ROW_BYTES = 8;               // chunk length + chunk offset of one row
constexpr int DAE_RO_MAX_C = 512;                 // the sorting launch holds one chunk in LDS (rank_of.hip rank_of_prep_kernel)
constexpr int DAE_RO_NUM_CU = 256, DAE_RO_NUM_XCD = 8;
constexpr int DAE_RO_MAX_B = 4096, DAE_RO_MAX_HP = 1024;

struct dae_ro_plan {
    int R_TILE;             // rows per group: 128, 64 or 32
    int C;                  // answers of a row per pass (0: no geometry fits -- the call is refused)
    int n_rg, nb_rg, grid;  // row groups, workgroups per row group, workgroups
    int Hp, G;              // hidden size padded to 32; k groups of 8
    size_t lds_bytes;       // dynamic LDS of the counting launch
    int passes_hint;        // passes a row of the AVERAGE length takes (what the choice of R_TILE was made by)
};

// bytes of LDS a counting workgroup of this geometry takes
inline size_t dae_rank_of_lds(int R_TILE, int Hp, int C)
{
    return (size_t)R_TILE * Hp * 4 + (size_t)R_TILE * C * DAE_RO_SLOT_BYTES + (size_t)R_TILE * DAE_RO_ROW_BYTES;
}

// answers of a row per pass at this row-group height (<= 0: the hidden tile alone does not fit)
inline int dae_rank_of_capacity(int R_TILE, int Hp)
{
    const long long left = (long long)DAE_RO_LDS_BYTES - DAE_RO_LDS_RESERVE - (long long)R_TILE * Hp * 4 -
                           (long long)R_TILE * DAE_RO_ROW_BYTES;
    if (left <= 0) return 0;
    long long c = left / ((long long)DAE_RO_SLOT_BYTES * R_TILE);
    if (c > DAE_RO_MAX_C) c = DAE_RO_MAX_C;
    return (int)c;
}

// which pass takes answer `i` of a row (0-based position in the row), and the passes a row of `len` answers takes
inline int dae_rank_of_pass(int i, int C) { return i / C; }
inline int dae_rank_of_passes(int len, int C) { return len <= 0 ? 0 : (len + C - 1) / C; }

// B rows, hidden size H, n_ans answers in all.  The longest row is not known to the host (nothing is read back), so the choice
// between row-group heights goes by the average row: halving the height (128 -> 64 at hidden 256: 20 -> 125 answers per pass)
// streams the decoder image once more per pass and is taken where it saves passes.
inline dae_ro_plan dae_plan_rank_of(int B, int H, long long n_ans)
{
    dae_ro_plan p{};
    if (B < 1 || B > DAE_RO_MAX_B || H < 1) return p;
    const int Hp = (H + 31) / 32 * 32;
    if (Hp > DAE_RO_MAX_HP) return p;
    int rt = 128;
    while (rt > 32 && (size_t)rt * Hp * 4 > 128 * 1024) rt >>= 1;     // the ranking calls' rule (score_plan.h dae_row_geometry_elt)
    while (rt > 32 && B <= rt / 2) rt >>= 1;
    const int avg = (int)((n_ans + B - 1) / B);
    int C = dae_rank_of_capacity(rt, Hp);
    if (rt > 32) {
        const int C2 = dae_rank_of_capacity(rt / 2, Hp);
        if (C <= 0 || dae_rank_of_passes(avg, C2) < dae_rank_of_passes(avg, C)) { rt >>= 1; C = C2; }
    }
    if (C <= 0) return p;
    p.R_TILE = rt; p.C = C; p.Hp = Hp; p.G = Hp / 8;
    p.n_rg = (B + rt - 1) / rt;
    int nb = (DAE_RO_NUM_CU / p.n_rg) / DAE_RO_NUM_XCD * DAE_RO_NUM_XCD;
    if (nb < DAE_RO_NUM_XCD) nb = DAE_RO_NUM_XCD;
    p.nb_rg = nb; p.grid = p.n_rg * nb;
    p.lds_bytes = dae_rank_of_lds(rt, Hp, C);
    p.passes_hint = dae_rank_of_passes(avg, C);
    return p;
}
