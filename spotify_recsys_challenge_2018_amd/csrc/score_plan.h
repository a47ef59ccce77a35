// score_plan.h -- how a ranking call is cut into launches: the row geometry, the threshold sample, the filter launch.
// Host only and free of HIP, so that a plain C++ program can exercise it (tests/host/score_plan_main.cpp).  score.hip
// (topk_phase_a / _b) reserves and launches by what dae_plan_topk returns; the launchers of decode_f32.hip ask the same
// predicates which kernel a geometry takes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/dae_hip.h"
#include "tau_search.h"           // DAE_HD

constexpr int DAE_KG = 8;         // k values per packed group (4 MFMA 32x32x2 steps)
constexpr int DAE_MAX_K = 1024;   // largest top-k of the paths that keep one 2048-key sort buffer: the exact mode, the title mix, the pipeline, the metrics kernel
constexpr int DAE_MAX_K_DEEP = 4096;   // largest top-k of the selection itself and of the fp32 / bf16 ranking calls (topk.hip: the 8192-key instantiation)
constexpr int DAE_NUM_CU = 256;   // MI355X
constexpr int DAE_NUM_XCD = 8;

struct dae_rowgeom {        // how B rows are cut into row groups for the decode kernels
    int R_TILE;             // rows per group: 128, 64 or 32 (LDS-resident h tile)
    int n_rg;               // ceil(B / R_TILE)
    int Bpad;               // n_rg * R_TILE
    int nb_rg;              // thread blocks per row group
    int grid;               // n_rg * nb_rg
    int waves;              // waves per workgroup (4 or 8)
};

// Rows are cut into groups of R_TILE playlists whose hidden tile (R_TILE x Hp elements of `elt` bytes) stays in LDS.
inline dae_rowgeom dae_row_geometry_elt(int B, int Hp, int elt)
{
    dae_rowgeom g;
    int rt = 128;
    while (rt > 32 && (size_t)rt * Hp * elt > 128 * 1024) rt >>= 1;   // <= 128 KiB of LDS
    while (rt > 32 && B <= rt / 2) rt >>= 1;                          // small batches
    g.R_TILE = rt;
    g.n_rg = (B + rt - 1) / rt;
    g.Bpad = g.n_rg * rt;
    int nb = (DAE_NUM_CU / g.n_rg) / DAE_NUM_XCD * DAE_NUM_XCD;
    if (nb < DAE_NUM_XCD) nb = DAE_NUM_XCD;
    g.nb_rg = nb;
    g.grid = g.n_rg * nb;
    g.waves = 4;
    return g;
}
// fp32: one wave per SIMD -- with 4 independent accumulators it saturates the fp32 matrix pipe (two per SIMD measured
// slower, profiles/r01_notes.md)
inline dae_rowgeom dae_row_geometry(int B, int Hp) { return dae_row_geometry_elt(B, Hp, 4); }
// bf16: 128-playlist tiles (64 KiB of LDS at H = 256).  256-playlist tiles fit LDS too but need 394 registers per wave,
// which rules out the second wave per SIMD that hides the epilogue (and measured the same kernel time but a slower phase A).
inline dae_rowgeom dae_row_geometry_bf16(int B, int Hp) { return dae_row_geometry_elt(B, Hp, 2); }

// the dedicated bf16 phase-B kernel: hidden = 256 (16 steps), 128-row groups
inline bool bf16_fast_filter(const dae_rowgeom& g, int dtype, int G)
{
    return dtype == DAE_DTYPE_BF16 && G == 16 && g.waves == 4 && g.R_TILE == 128;
}

// most tiles one workgroup of the filter launch can walk (sizes its private candidate lists)
inline int dae_filter_block_tiles(const dae_rowgeom& g, int n_items, int dtype, int Hp, bool mixed = false)
{
    const int n_ws = g.nb_rg * g.waves;
    if (bf16_fast_filter(g, dtype, Hp / 16) && !mixed) {
        const int n_ws8 = g.nb_rg * 8;                       // (decode_bf16_h256_filter_kernel<1, 4, 8, 8>: 8 waves, a tile each)
        return 8 * ((n_items + n_ws8 - 1) / n_ws8);
    }
    return g.waves * ((n_items + n_ws - 1) / n_ws);
}

// phase A with per-WAVE group maxima (decode_bf16_h256_wavemax_kernel): bf16 image of hidden 256, 128-row groups, and a sample
// that gives each of the 8 wave slots per workgroup at least two tiles
inline bool dae_sample_wave_groups(const dae_rowgeom& g, int Hp, int n_samp)
{
    return Hp == 256 && g.R_TILE == 128 && g.waves == 4 && n_samp >= 2 * g.nb_rg * 8;
}

// does the filter launch run decode_f32_h256_filter_kernel<0>, the one kernel that can walk live lists?
inline bool dae_filter_takes_live(const dae_rowgeom& g, int dtype, int Hp, bool mixed)
{
    return dtype == DAE_DTYPE_F32 && g.R_TILE == 128 && Hp / DAE_KG == 32 && g.waves == 4 && !mixed;
}

// does the threshold sample run in HALF row groups (decode_generic.hip decode_f32_kernel's HALF: fp32, hidden 256, 128-row groups,
// cross-wave group maxima, ONE round of tiles)?  The launcher (decode_f32.hip dae_launch_decode_dense_f32) asks the same.
inline bool dae_sample_takes_half(const dae_rowgeom& g, int dtype, int Hp, bool mixed, int gmax_per_wave, int n_samp)
{
    return dtype == DAE_DTYPE_F32 && g.R_TILE == 128 && Hp / DAE_KG == 32 && g.waves == 4 && !gmax_per_wave && !mixed &&
           n_samp <= g.nb_rg * 4;
}

// THE DECODED-TILE TABLE of a half-row-group sample that skips (decode_f32_kernel's HALF -> tau_select_kernel):
// one 32-bit word per workgroup of the sample launch, [2 n_rg][nb_rg]; byte w of word bir of half group hg is 1 iff wave w of that
// workgroup decoded its item w * nb_rg + bir (items are wave-major: decode_f32_kernel).  The sample launch stores a row's maxima
// [bir * 32, bir * 32 + 32) only where the word is non-zero and the 32 dense logits of an item only where its byte is; the
// threshold launch takes every other slot as -inf without reading it.  The ONE mapping both kernels and the host test
// (tests/host/sample_sparse_main.cpp) use:
struct dae_samp_slot { int word, byte; };
DAE_HD dae_samp_slot dae_sample_item_slot(int item, int nb_rg) { return dae_samp_slot{item % nb_rg, item / nb_rg}; }
DAE_HD int dae_sample_slot_item(int word, int byte, int nb_rg) { return byte * nb_rg + word; }
// float4 f of a row's dense sample (32 logits = 8 float4 per item) belongs to item ...
DAE_HD int dae_sample_f4_item(int f) { return f >> 3; }

struct dae_plan_in {
    int ntiles, col_lo, col_hi, Hp;   // the decoder image (dae_packed)
    bool ub_valid;                    // ... holds per-tile logit bounds of its own (dae_packed::tile_ub)
    dae_rowgeom g;                    // the geometry the hidden rows are packed for
    int n_tracks, k, dtype_in;
    bool mixed;                       // dae_set_score_mix: the launches rank the MIXED score
    int overlap_hint, filter_skip;    // dae_set_overlap_hint, dae_set_filter_skip
    bool own_tau = false;             // the thresholds this call computes are the ones its filter launch takes (no exchange between)
    int B = 0;                        // rows of the call (which threshold kernel runs: dae_tau_wave_per_row)
};

// does the threshold launch take tau_select_wave_kernel (tau_select.hip: a WAVE per row, for launches of many short rows) instead of
// the workgroup-per-row kernel?  n_g maxima and n_s dense sample logits per row
inline bool dae_tau_wave_per_row(int B, int64_t n_g, int64_t n_s)
{
    return B >= 1024 && n_g <= 64 * 32 && (n_s >> 2) <= 64 * 8;
}

struct dae_score_plan {
    bool bad_mix;           // DAE_DTYPE_BF16_EXACT under dae_set_score_mix: no launch sequence exists (only `last` is filled)
    int dtype;              // the arithmetic of the GEMM launches
    bool exact, mixed;
    int n_valid_col, nrank; // global bound of the ranked columns; ranked columns of this image
    int ntiles;             // ceil(nrank / 32): the tiles the call walks (a prefix of the image's); 0 = nothing to rank
    int S, n_samp, n_other; // sample stride; sample tiles; the others
    bool fused;             // sample + tau + filter (else: dense logits of every ranked tile, then one selection)
    dae_rowgeom gA;         // the sample launch's own geometry (!= g only with wave_groups)
    bool wave_groups;       // phase A takes per-WAVE group maxima (decode_bf16_h256_wavemax_kernel)
    bool use_band;          // the sample walks the band-dealt list (dae_launch_tile_band)
    int64_t ld_s, ld_g;     // row strides of the sample logits and of the group maxima
    int gmax_per_wave;      // dae_launch_decode_dense_f32
    bool whole_b;           // the filter launch decodes the sample tiles again: phase A stores maxima only
    int n_filter, cap;      // tiles of the filter launch; candidates one of its workgroups can emit per row
    bool build_live;        // the filter launch walks per-row-group live lists (dae_launch_live_tiles: tiles skipped by their bound)
    int32_t last[8];        // what dae_last_plan reports
    bool live_in_tau;       // build_live, and the threshold launch builds the lists itself (tau_select_kernel's tail, tau_select.hip): no
                            // launch of live_tiles_kernel
    bool sample_skip;       // the sample runs in half row groups (dae_sample_takes_half) on an image that holds bounds: its waves
                            // may skip the tiles a bound puts below every row's threshold (under dae_set_filter_skip)
};

inline dae_score_plan dae_plan_topk(const dae_plan_in& in)
{
    dae_score_plan p{};
    const dae_rowgeom& g = in.g;
    const int k = in.k;
    const bool exact = in.dtype_in == DAE_DTYPE_BF16_EXACT;
    const int dtype = exact ? DAE_DTYPE_BF16 : in.dtype_in;
    const bool mixed = in.mixed;
    const int n_valid_col = in.n_tracks < in.col_hi ? in.n_tracks : in.col_hi;
    int nrank = n_valid_col - in.col_lo;
    if (nrank < 0) nrank = 0;
    // the ranked columns are a prefix of the image: a ranking call walks the tiles that hold one and no other (the tiles behind
    // them -- the artist columns of the shipped vocabulary -- can return nothing; only dae_decode_dense needs their logits).
    // Offsets laid out by the image (eps_max behind pk->ntiles * 32 bounds) keep pk->ntiles.
    const int ntiles = (nrank + 31) / 32;

    // ---- how many tiles form the threshold sample (phase A) ---------------------------------
    // phase A decodes one tile per SIMD of the row group's workgroups (a full, short round on the
    // matrix pipes whatever the wave count), i.e. every S-th tile; at least ntiles/8 for a tight tau
    const int n_simd = g.nb_rg * 4;
    int rounds = (int)(((double)ntiles / 8.0) / n_simd + 0.5);
    if (rounds < 1) rounds = 1;
    int S = (ntiles + rounds * n_simd - 1) / (rounds * n_simd);
    // WHICH shapes take the threshold path stays what it was when the calls walked the whole image: an image of more tiles than a
    // round of SIMD slots is scored through sample + filter (callers and tests count on `fused` for such shapes).  Where its ranked
    // tiles alone fit one round, the sample is every second one of them: the same decode work as the dense launch, and a
    // selection over the survivors instead of over every ranked column.
    if (S < 2 && ntiles >= 2) {
        int rounds_img = (int)(((double)in.ntiles / 8.0) / n_simd + 0.5);
        if (rounds_img < 1) rounds_img = 1;
        if ((in.ntiles + rounds_img * n_simd - 1) / (rounds_img * n_simd) >= 2) S = 2;
    }
    // exact mode: the same launches whatever the size (a small problem's "sample" is every tile: S = 1)
    if (exact && S < 2) S = 1;
    const bool fused = (S >= 2 || exact) && nrank > 0;
    const int n_samp = fused ? (ntiles + S - 1) / S : ntiles;
    const int n_other = ntiles - n_samp;
    const int32_t last[8] = {g.R_TILE, g.n_rg, g.nb_rg, fused ? S : 1, n_samp, n_other, fused ? 1 : 0, ntiles};
    for (int i = 0; i < 8; ++i) p.last[i] = last[i];
    p.dtype = dtype; p.exact = exact; p.mixed = mixed; p.n_valid_col = n_valid_col; p.nrank = nrank; p.ntiles = ntiles;
    p.gA = g;
    if (mixed && exact) { p.bad_mix = true; return p; }
    if (ntiles == 0) { p.S = 1; return p; }                // no ranked column in this image (n_tracks <= col_lo): no GEMM launch
    p.S = S; p.n_samp = n_samp; p.n_other = n_other; p.fused = fused;

    // ---- the sample launch's OWN geometry ---------------------------------------------------------------------------------------
    // Phase A decodes 1 / 11 of the tiles the filter launch decodes, yet on the filter launch's grid (a workgroup per CU) it held
    // every CU for 8 - 15 us: one or two tiles per wave behind a 64 KB hidden-tile fill, with registers / LDS that let nothing of
    // another batch in.  With several batches in flight the step is the SUM of such chip-wide launches (filter + sample + refine:
    // profiles/r06_notes.md).  So the sample takes fewer workgroups per row group -- ~4 tiles per wave slot of the per-wave-maxima
    // kernel (decode_bf16_h256_wavemax_kernel), 8 nbA x 32 maxima per row -- and leaves the other CUs to the other batches' launches.
    // Same sample tiles, same logits; the groups (the tiles one wave decodes, n_ws places apart in the bias order) change, i.e.
    // only how tight tau is.  Only where that kernel applies (bf16 image of hidden 256, 128-row groups, no title mix).
    // does a launch of geometry gg take per-WAVE groups?
    auto takes_wave_groups = [&](const dae_rowgeom& gg) {
        const int n_ws = gg.nb_rg * gg.waves;
        const bool enough = (int64_t)((n_samp + n_ws - 1) / n_ws) * gg.nb_rg * 32 >= 4 * (int64_t)k;      // (else: one value per wave slot)
        return fused && enough && dtype == DAE_DTYPE_BF16 && !mixed && dae_sample_wave_groups(gg, in.Hp, n_samp);
    };
    dae_rowgeom gA = g;
    {
        // measured (profiles/r06_notes.md 2, four batches in flight / alone, M playlists/s, exact mode): 256 rows 6.28 -> 6.62 / 3.92 ->
        // 3.59 at 16 workgroups per row group; 1 024 rows 9.10 -> 9.86 / 7.10 -> 6.53 at 8; 2 048 rows 10.85 -> 11.50 / 8.0 -> 8.0 at 8
        // -- a gain only when other batches' launches can use the CUs: taken under dae_set_overlap_hint, ~4 tiles per wave slot for
        // launches of few row groups, ~8 from 8 row groups on
        const int per_slot = g.n_rg >= 8 ? 8 : 4;
        int nbA = in.overlap_hint ? ((n_samp + 8 * per_slot - 1) / (8 * per_slot) + DAE_NUM_XCD - 1) / DAE_NUM_XCD * DAE_NUM_XCD : g.nb_rg;
        if (nbA < DAE_NUM_XCD) nbA = DAE_NUM_XCD;
        if (nbA < g.nb_rg) {
            dae_rowgeom t = g;
            t.nb_rg = nbA; t.grid = g.n_rg * nbA;
            if (takes_wave_groups(t) && (int64_t)8 * nbA * 32 >= 4 * (int64_t)k) gA = t;
        }
    }
    const int64_t ld_s = (int64_t)n_samp * 32;
    // one maximum per (workgroup of the row group, round of sample tiles, position in the tile)
    const int n_ws_a = gA.nb_rg * gA.waves;
    int64_t ld_g = (int64_t)((n_samp + n_ws_a - 1) / n_ws_a) * gA.nb_rg * 32;
    // ... unless that leaves too few maxima for the rank tau needs (k + seeds): small samples -- vocabulary shards,
    // large batches -- keep one value per wave slot and position, i.e. every sample element
    int gmax_per_wave = ld_g < 4 * (int64_t)k ? 1 : 0;
    if (gmax_per_wave) ld_g *= gA.waves;
    // the groups are the tiles ONE wave of the filter kernel's shape decodes (decode_bf16_h256_wavemax_kernel: no exchange
    // through LDS, two waves per SIMD) -- 8 nb_rg x 32 maxima per row
    const bool wave_groups = takes_wave_groups(gA);
    if (wave_groups) {
        // (fewer than four tiles per wave slot: waves w and w + 4 share a group -- value 4 -- so that a row has 4 nb_rg x 32 maxima:
        // 4 096 at 1 024 rows, the threshold kernel's 16-key shape)
        const bool pair = n_samp < 4 * gA.nb_rg * 8 && (int64_t)4 * gA.nb_rg * 32 >= 4 * (int64_t)k;
        gmax_per_wave = pair ? 4 : 3;
        ld_g = (int64_t)(pair ? 4 : 8) * gA.nb_rg * 32;
    }
    // bf16 launches whose sample takes several rounds of the phase-A workgroups (many rows: few workgroups per row group): the
    // sample re-dealt so that a workgroup's tiles of a round come from different popularity bands (prepack.hip
    // tile_band_kernel) -- not when the launch takes per-WAVE groups: there the plain order IS band-dealt
    p.use_band = fused && dtype == DAE_DTYPE_BF16 && n_samp > n_ws_a && !wave_groups;
    // bf16: the filter launch decodes the sample tiles AGAIN instead of phase A storing their dense logits for the
    // threshold kernel to scan: 483 more tiles cost its matrix cores 1.5 us, the 15.8 MB dense buffer (written by phase
    // A through LDS, read back by the threshold kernel, its survivors compacted there) costs more.  Phase A then leaves
    // the group maxima only, the threshold kernel emits no survivors, and every candidate comes from the filter launch.
    // (fp32 keeps the buffer: the same tiles are 13.6 us of its matrix time.)
    // exact mode (DAE_DTYPE_BF16_EXACT): always so, on BOUNDS -- phase A decodes with the bias b - eps (its maxima are
    // lower bounds of fp32 logits, so tau is a valid threshold for the fp32 ranking), the filter launch with b + eps
    // (nothing whose fp32 logit reaches tau is dropped), and the refine step recomputes every survivor in fp32
    const bool whole_b = fused && dtype == DAE_DTYPE_BF16 && ((gmax_per_wave != 1 && !mixed) || exact);
    if (whole_b) p.last[5] = ntiles;
    p.gA = gA; p.wave_groups = wave_groups; p.ld_s = ld_s; p.ld_g = ld_g; p.gmax_per_wave = gmax_per_wave; p.whole_b = whole_b;
    p.sample_skip = fused && in.ub_valid && dae_sample_takes_half(gA, dtype, in.Hp, mixed, gmax_per_wave, n_samp);

    // ---- phase B: everything else through the threshold filter ----------------------------------------------------------------
    p.n_filter = whole_b ? ntiles : n_other;
    p.cap = dae_filter_block_tiles(g, p.n_filter, dtype, in.Hp, mixed) * 32;      // worst case: everything passes
    // SKIPPED TILES (fp32, hidden 256, 128-row groups, no score mix: decode_f32_h256_filter_kernel): with the thresholds and a
    // bound of every tile's logits (dae_packed::tile_ub) known, the launch walks per row group only the tiles that can hold a
    // logit >= tau.  What that leaves out the filter epilogue would have dropped element by element: the lists cannot change
    // (DESIGN.md section 2).  Every other filter launch (generic fp32, bf16, exact bf16, the mixed score) walks all its tiles.
    p.build_live = in.filter_skip && p.n_filter > 0 && !whole_b && in.ub_valid && dae_filter_takes_live(g, dtype, in.Hp, mixed);
    // WHO builds them: the threshold launch itself, where the thresholds it computes are the filter launch's (no exchange between
    // the two halves) and it is the workgroup-per-row kernel, whose workgroups count themselves per row group; else a launch of
    // live_tiles_kernel on the thresholds the filter launch is given
    p.live_in_tau = p.build_live && in.own_tau && !dae_tau_wave_per_row(in.B, ld_g, whole_b ? 0 : ld_s);
    return p;
}
