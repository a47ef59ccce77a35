// mix_loss_plan.h -- how a dae_mix_loss_rows call is cut into panels of rows and where its scratch lies inside ONE allocation of
// the title context (dae_ctx::mix_loss).  Host only and free of HIP, like score_plan.h, so that a plain C++ program can sweep it
// (tests/host/mix_loss_plan_main.cpp).  mix_loss.hip reserves, carves and walks by what dae_plan_mix_loss returns.
//
// The call walks panels of at most DAE_MIXLOSS_PANEL rows, one after the other on one stream; panel i holds the rows
// [i * 256, min(B, (i + 1) * 256)) and has the row geometry of a batch of that many rows.  The panels share
//
//   term   [V32][panel_rows] fp32   the DAE's term of ONE panel, transposed: element (column c, row r of the panel) at
//                                   c * nb + r with nb the PANEL's rows (a short last panel uses the head of the section)
//   part   [part_floats]     fp32   the partial table [n_rg][nb_rg][R_TILE] of ONE panel's GEMM launch (the larger of a full
//                                   panel's and the last panel's)
//   rows   [B]               fp32   the row losses, when the caller gave no row_loss (the cost launch reads all B at the end)
//
// V32 = V rounded up to whole 32-column tiles, panel_rows = min(B, 256): the term is 4 * V32 * 256 bytes at most (174 MB at
// V = 170 000), whatever B.  Every section starts on a multiple of 256 bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "score_plan.h"

constexpr int DAE_MIXLOSS_PANEL = 256;
constexpr int DAE_MIXLOSS_MAX_B = 4096;
constexpr int DAE_MIXLOSS_MAXH = 1024;         // hidden size of the DAE and feature width of the title scorer (one LDS row each)
constexpr size_t DAE_MIXLOSS_ALIGN = 256;

struct dae_mixloss_plan {
    int n_panels;           // ceil(B / 256) (0: bad arguments)
    int panel_rows;         // rows of the largest panel: min(B, 256)
    size_t V32;             // columns of the term section
    size_t o_term, o_part, o_rows;            // byte offsets
    size_t term_bytes, part_floats, row_floats;
    size_t total;           // bytes of the allocation (0: bad arguments)
};

inline size_t dae_mixloss_up(size_t x) { return (x + DAE_MIXLOSS_ALIGN - 1) / DAE_MIXLOSS_ALIGN * DAE_MIXLOSS_ALIGN; }

// the rows [r0, r0 + nb) of panel i
inline void dae_mixloss_panel(int B, int i, int* r0, int* nb)
{
    *r0 = i * DAE_MIXLOSS_PANEL;
    const int left = B - *r0;
    *nb = left < DAE_MIXLOSS_PANEL ? (left > 0 ? left : 0) : DAE_MIXLOSS_PANEL;
}

// the row geometry of a panel of nb rows over the title image (Hp_title = its K padded to 32): what the GEMM launch and the
// finishing launch of that panel index the partial table by
inline dae_rowgeom dae_mixloss_geometry(int nb, int Hp_title) { return dae_row_geometry(nb, Hp_title); }

// B rows, V columns, the title image's padded K; want_rows: the caller gave no row_loss
inline dae_mixloss_plan dae_plan_mix_loss(int B, int V, int Hp_title, bool want_rows)
{
    dae_mixloss_plan p{};
    if (B < 1 || B > DAE_MIXLOSS_MAX_B || V < 1 || Hp_title < 32 || Hp_title % 32 != 0 || Hp_title > DAE_MIXLOSS_MAXH) return p;
    p.n_panels = (B + DAE_MIXLOSS_PANEL - 1) / DAE_MIXLOSS_PANEL;
    p.panel_rows = B < DAE_MIXLOSS_PANEL ? B : DAE_MIXLOSS_PANEL;
    p.V32 = ((size_t)V + 31) / 32 * 32;
    p.term_bytes = p.V32 * (size_t)p.panel_rows * sizeof(float);
    // the panels are full ones but the last: two geometries at most
    int r0, nb_last;
    dae_mixloss_panel(B, p.n_panels - 1, &r0, &nb_last);
    const dae_rowgeom gf = dae_mixloss_geometry(p.panel_rows, Hp_title), gl = dae_mixloss_geometry(nb_last, Hp_title);
    const size_t pf = (size_t)gf.grid * gf.R_TILE, pl = (size_t)gl.grid * gl.R_TILE;
    p.part_floats = pf > pl ? pf : pl;
    p.row_floats = want_rows ? (size_t)B : 0;
    size_t o = 0;
    p.o_term = o; o = dae_mixloss_up(o + p.term_bytes);
    p.o_part = o; o = dae_mixloss_up(o + p.part_floats * sizeof(float));
    p.o_rows = o; o = dae_mixloss_up(o + p.row_floats * sizeof(float));
    p.total = o;
    return p;
}
