// mix_plan.h -- how a call of the exact title mix (dae_mix_topk_exact) is cut into launches: which filter instance, the row
// groups, the workgroups per row group, the threshold sample, the candidate segments, whether the refine launch ends the call.
// Host only and free of HIP, as score_plan.h is, so that a plain C++ program can exercise it (tests/host/mix_plan_main.cpp).
// mixexact.hip reserves and launches by what dae_plan_mix returns; the launchers of mix_prep.hip, mix_filter.hip and
// mix_refine.hip read the same struct.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "score_plan.h"            // DAE_NUM_CU, DAE_NUM_XCD

constexpr int MX_RB = 3;            // row blocks of 32 playlists per row group: 96 rows x 704 k x 2 B = 132 KiB of LDS
constexpr int MX_NW = 8;            // waves per workgroup (two per SIMD: one's epilogue under the other's MFMAs)
constexpr int MX_REF_CAP = 8192;    // survivors per row the refine launch's compact lists hold
constexpr int MX_MAX_STEPS = 32;    // MFMA steps of one image at the largest supported shape (hidden / row length 512)
constexpr size_t MX_LDS_BYTES = 160 * 1024;      // LDS of a CU: what one workgroup can be given
constexpr size_t MX_FRAG_BYTES = 16;             // a lane's operand of one MFMA step: a uint4 of 8 bf16
constexpr int MR_MAX_SEG = 1024;    // candidate segments per row the refine launch's prefix table holds
constexpr int MR_STAGE = 8192;      // candidates of a row whose two keys fit LDS (next to the 16 waves' 80 KiB of buffers)
constexpr int MR_RANK_MAX = 1024;   // = DAE_RANK_MAX (rank_lds.h, which is device code; mix_refine.hip asserts the equality)

// THE rule for "does this model have an exact title mix" (models/DAEs.py asks it through the ABI, dae_mix_exact_shape_ok):
// multiples of 64, so that both images are whole chunks of 4 steps (mix_bf16_steps_kernel); hidden 64 is left to the fp32
// kernels -- a DAE GEMM of 4 steps
inline bool dae_mix_shape_ok(int hidden, int ld_feat)
{
    return hidden >= 128 && hidden <= 16 * MX_MAX_STEPS && hidden % 64 == 0 &&
           ld_feat >= 64 && ld_feat <= 16 * MX_MAX_STEPS && ld_feat % 64 == 0;
}

struct dae_mix_plan_in {
    int HD, HpD;            // the DAE's bf16 image: hidden size, padded (dae_packed::H, ::Hp)
    int HT, HpT;            // the title scorer's: feature row length, padded
    int col_hi;             // columns both images hold (from 0)
    int B, k, n_tracks;
    int overlap_hint;       // dae_set_overlap_hint on the title context
};

enum dae_mix_refusal {      // in the order the call tests them
    DAE_MIX_OK = 0,
    DAE_MIX_BAD_SHAPE,      // neither the shipped shape nor one of dae_mix_shape_ok
    DAE_MIX_NO_ROWS,        // B <= 0: nothing to do, no error
    DAE_MIX_TOO_MANY_ROWS,  // B > 4096
    DAE_MIX_NO_COLUMN,      // no rankable column
    DAE_MIX_TOO_MANY_SEGMENTS,
};

struct dae_mix_plan {
    int status;             // dae_mix_refusal; the fields below a refusal's own test are not filled
    bool shipped;           // hidden 256, rows of 448: mix_bf16_kernel<16, 28, 3>, unrolled; else mix_bf16_steps_kernel<RB>
    int NSD, NST;           // MFMA steps of the two images
    int RB, R_TILE;         // row blocks of 32 playlists per row group (3 or 2); playlists per row group
    int n_rg, Bpad;         // row groups; n_rg * R_TILE
    int nb, grid;           // workgroups per row group of the filter launch (= candidate segments per row); n_rg * nb
    int n_valid_col, ntr;   // rankable columns; tiles that hold one
    int n_samp, nb_s;       // tiles of the threshold sample (the head of the bias order); workgroups per row group of its launch
    int64_t ld_s;           // row stride of the sample's maxima: 8 per tile
    int cap;                // entries one workgroup can append to a row's segment
    size_t lds_bytes;       // dynamic LDS of a sample / filter launch
    size_t lds_attr;        // what the chosen instance's LDS limit is raised to, once: the largest row group it can be given
    bool fuse;              // the refine launch ends the call (no selection launch)
    int32_t last[8];        // what dae_last_plan reports (dae_note_plan)
};

inline dae_mix_plan dae_plan_mix(const dae_mix_plan_in& in)
{
    dae_mix_plan p{};
    constexpr int NW = MX_NW;
    // the shipped shape (hidden 256, rows of 448) keeps its unrolled instance; every other shape of dae_mix_shape_ok runs
    // mix_bf16_steps_kernel
    const bool shipped = in.HpD == 16 * 16 && in.HpT == 28 * 16 && in.HD == in.HpD && !(in.HT & 15);
    p.shipped = shipped;
    if (!shipped && !dae_mix_shape_ok(in.HD, in.HT)) { p.status = DAE_MIX_BAD_SHAPE; return p; }
    const int NSD = in.HpD / 16, NST = in.HpT / 16, NS = NSD + NST;
    // row groups of 96 playlists while their hidden rows (RB x NS KiB) and the kernel's tail fit the CU's 160 KiB of LDS -- up to
    // 52 steps (hidden 384 + rows of 448) -- and of 64 beyond (at most 128 KiB at hidden 512 + rows of 512)
    const int RB = shipped || (size_t)MX_RB * 64 * NS * MX_FRAG_BYTES + MX_RB * 32 * 8 + 16 <= MX_LDS_BYTES ? MX_RB : 2;
    const int R_TILE = RB * 32;
    p.NSD = NSD; p.NST = NST; p.RB = RB; p.R_TILE = R_TILE;
    const int B = in.B, k = in.k;
    if (B <= 0) { p.status = DAE_MIX_NO_ROWS; return p; }
    if (B > 4096) { p.status = DAE_MIX_TOO_MANY_ROWS; return p; }
    const int n_valid_col = in.n_tracks < in.col_hi ? in.n_tracks : in.col_hi;
    const int ntr = (n_valid_col + 31) / 32;                      // tiles with rankable columns
    p.n_valid_col = n_valid_col; p.ntr = ntr;
    if (ntr <= 0) { p.status = DAE_MIX_NO_COLUMN; return p; }

    // geometry: row groups of R_TILE playlists; the workgroups of a row group in multiples of the XCD count
    const int n_rg = (B + R_TILE - 1) / R_TILE;
    const int Bpad = n_rg * R_TILE;
    int nb = (DAE_NUM_CU / n_rg) / DAE_NUM_XCD * DAE_NUM_XCD;
    if (nb < DAE_NUM_XCD) nb = DAE_NUM_XCD;
    while (nb > DAE_NUM_XCD && (nb - DAE_NUM_XCD) * NW >= ntr) nb -= DAE_NUM_XCD;     // small images: no workgroups without a tile
    const int grid = n_rg * nb;
    p.n_rg = n_rg; p.Bpad = Bpad; p.nb = nb; p.grid = grid;
    // (the refine launch walks a row's nb segments through a table in LDS)
    if (nb > MR_MAX_SEG) { p.status = DAE_MIX_TOO_MANY_SEGMENTS; return p; }

    // tiles by their largest DAE bias (the popularity prior): the head of the list is the threshold sample
    // (an eighth of the tiles, in whole rounds of 64, at least 256)
    int n_samp = (ntr / 8) / 64 * 64;
    if (n_samp < 256) n_samp = 256;
    if (n_samp > ntr) n_samp = ntr;
    p.n_samp = n_samp;
    // a row group's hidden rows of both scorers | per row a candidate count and a threshold | the claim counter
    p.lds_bytes = (size_t)RB * 64 * NS * MX_FRAG_BYTES + (size_t)R_TILE * 8 + 16;
    // the shipped instance takes exactly its row group; a steps instance the largest it can be given (RB = 3 was chosen because
    // its row group fits MX_LDS_BYTES; RB = 2 holds at most 2 x 64 steps: 128 KiB)
    p.lds_attr = shipped ? p.lds_bytes
               : RB == MX_RB ? MX_LDS_BYTES : (size_t)2 * 64 * (2 * MX_MAX_STEPS) * MX_FRAG_BYTES + 2 * 32 * 8 + 16;
    p.ld_s = (int64_t)n_samp * 8;
    // the sample pass on a grid of its own when other launches are in flight (round 6, as the plain path's sample launch:
    // score_plan.h dae_plan_topk): an eighth of the tiles does not need a workgroup on every CU -- ~8 items per wave slot; its
    // maxima are stored per ITEM, so the geometry changes nothing but where they are computed
    int nb_s = nb;
    if (in.overlap_hint) {
        nb_s = ((n_samp + 8 * NW - 1) / (8 * NW) + DAE_NUM_XCD - 1) / DAE_NUM_XCD * DAE_NUM_XCD;
        if (nb_s > nb) nb_s = nb;
    }
    if (nb_s < DAE_NUM_XCD) nb_s = DAE_NUM_XCD;
    p.nb_s = nb_s;
    // a workgroup walks the tiles congruent to its index mod nb, by position or by claim: each appends at most 32 entries to a row
    p.cap = ((ntr + nb - 1) / nb) * 32;
    // k <= 512 and a seed bitmap that fits behind the ordering keys: the refine launch ends the call (no selection launch)
    p.fuse = k <= MR_RANK_MAX / 2 && ((size_t)((n_valid_col + 31) >> 5) + 2 * MR_RANK_MAX) <= (size_t)MR_STAGE;
    const int32_t last[8] = {R_TILE, n_rg, nb, 1, n_samp, ntr, 0, ntr};      // (S = 1, fused = 0: score.hip dae_last_plan)
    for (int i = 0; i < 8; ++i) p.last[i] = last[i];
    return p;
}
