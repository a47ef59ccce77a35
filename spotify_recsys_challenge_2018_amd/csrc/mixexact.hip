// mixexact.hip -- DAE_DTYPE_BF16_EXACT under the title mix (`--challenge` with titles: main_challenge.py:80-90 of the
// reference always scores through DAE_title, DAEs.py:153-181):
//
//     y[r, c] = sigmoid(z_t[r, c]) * w_title[r] + sigmoid(z_d[r, c]) * w_playlist[r]                      (DAEs.py:180)
//     z_d = h[r, :] . W_dec[c, :] + b_dec[c]            (hidden 256: the frozen DAE, DAEs.py:165-171)
//     z_t = feat[r, :] . Output_W[:, c] + Output_b[c]   (400 title features in rows of 448, Char_CNN.py:64-72)
//
// The fp32 path runs both vocabulary-wide GEMMs on v_mfma_f32_32x32x2_f32 (the canonical fmaf chains) and ranks y.  Here
// BOTH run on v_mfma_f32_32x32x16_bf16 in ONE launch per pass -- a wave decodes a 32-column tile against a row group's
// hidden rows of both scorers (704 k values, two accumulator sets) -- on BOUNDS of the two logits, and only the survivors are
// recomputed in fp32:
//   sample launch (mix_filter.hip, MODE 1): biases shifted DOWN by the bounds -> lower bounds l of y over the head of the
//          bias-ordered tile list; their maxima over groups of 4 columns go to the threshold kernel (tau_select_kernel, tau_select.hip),
//          whose tau is a valid lower bound of the row's k-th largest rankable non-seed y;
//   filter launch (mix_filter.hip, MODE 0): biases shifted UP -> upper logits (u_t, u_d); a column is listed with them when
//          its upper bound can reach tau.  The test needs no sigmoid and no division: with E = exp(-z),
//              w_t / (1 + E_t) + w_p / (1 + E_d) >= tau   <=>   w_t (1 + E_d) + w_p (1 + E_t) >= tau (1 + E_t)(1 + E_d),
//          two v_exp_f32 and a handful of multiply-adds per element, compared with 2^-15 of slack (mix_common.h mix_can_reach).
//          The lane's pair of MAXIMA over its 16 columns takes the test first: most (row block, tile) pairs of the low-bias
//          tiles stop there.  (The canonical sigmoid in the epilogue -- ~35 VALU instructions, twice per element -- made the
//          launch VALU-bound at 316 us for 750 rows; two logit thresholds per row, u_t >= thT or u_d >= thD, cost 3
//          instructions but list EVERY column when one scorer is a flat background, e.g. an untrained title model.)
//   refine launch (mix_refine.hip), one 1024-thread workgroup per row: (1) the mixed bounds [l, u] of every listed column,
//          densely (a lane per candidate, hardware exp2 / rcp, 2^-15 wider); the need-th largest l is a threshold tau' that
//          `need` columns provably reach, so only columns with u >= tau' can be among the k best -- both keys staged in LDS for
//          rows of up to 8 192 candidates, three streamed passes with a two-level fixed-bin histogram beyond; (2) the survivors
//          are recomputed: z_t, z_d with the canonical chains, mixed with the operations of mix_scores_kernel (title.hip) in
//          their order -- the value the fp32 path ranks -- tested against the promise (bound guard, as refine.hip) and left
//          as one compact (y, column) list per row for the selection kernel.  Rows with both weights 0 (no input, no title)
//          have y = +0 everywhere: they list nothing and get the first k + n_seeds columns directly.
// The bounds are derived in mix_common.h; the geometry of the launches is mix_plan.h's dae_plan_mix; what the title image
// and a call's rows need beforehand is mix_prep.hip; the audit of the columns the filter dropped is audit.hip's.
#include "dae_internal.h"

extern "C" int dae_mix_exact_shape_ok(int hidden, int ld_feat) { return dae_mix_shape_ok(hidden, ld_feat); }

int dae_mix_topk_exact_impl(dae_ctx* tc, dae_ctx* dc, const float* feat, int64_t ld_feat, const float* h, int64_t ld_h, int B,
                            const float* w_title, const float* w_playlist, int n_tracks, const int32_t* seed_row_ptr,
                            const int32_t* seed_col, int k, float* out_score, int32_t* out_idx)
{
    dae_packed& pt = tc->pk_bf16;
    dae_packed& pd = dc->pk_bf16;
    if (!pt.valid || !pt.exact || !pd.valid || !pd.exact)
        return dae_fail(tc, DAE_ERR_STATE, "both contexts need their weights prepacked with DAE_DTYPE_BF16_EXACT");

    // ---- plan
    const dae_mix_plan pl = dae_plan_mix(dae_mix_plan_in{pd.H, pd.Hp, pt.H, pt.Hp, pt.col_hi, B, k, n_tracks, tc->overlap_hint});
    if (pl.status == DAE_MIX_BAD_SHAPE)
        return dae_fail(tc, DAE_ERR_ARG, "the exact title mix takes hidden 128..512 (DAE) and feature rows of 64..512, both in steps "
                        "of 64 (got %d and %d): use DAE_DTYPE_F32", pd.H, pt.H);
    if (pt.col_lo != 0 || pd.col_lo != 0 || pt.col_hi != pd.col_hi)
        return dae_fail(tc, DAE_ERR_ARG, "both images must hold the same columns, starting at 0");
    if (pl.status == DAE_MIX_NO_ROWS) return DAE_OK;
    if (pl.status == DAE_MIX_TOO_MANY_ROWS) return dae_fail(tc, DAE_ERR_ARG, "at most 4096 rows per call (got %d)", B);
    if (pl.status == DAE_MIX_NO_COLUMN) return dae_fail(tc, DAE_ERR_ARG, "no rankable column");
    if (dc->stream != tc->stream) return dae_fail(tc, DAE_ERR_STATE, "both contexts must be bound to the same stream");
    if (pl.status == DAE_MIX_TOO_MANY_SEGMENTS) return dae_fail(tc, DAE_ERR_ARG, "too many candidate segments (%d)", pl.nb);
    const dae_mix_call c{feat, ld_feat, h, ld_h, B, w_title, w_playlist, seed_row_ptr, seed_col, k, out_score, out_idx};
    const size_t Bpad = (size_t)pl.Bpad;
    int rc;
    // tiles by their largest DAE bias (the popularity prior): the head of the list is the threshold sample
    if (!(pd.order.p && pd.order_nrank == pl.n_valid_col && dae_tile_order_sorted(pl.ntr))) {      // (the bias order does not depend on the sample size)
        rc = dae_launch_tile_order(dc, pd, pl.n_valid_col, pl.n_samp, 1);
        if (rc) return dae_fail(tc, rc, "%s", dc->err.c_str());
    }
    const int* order = static_cast<const int*>(pd.order.p);

    // ---- reserves: per row F_r and the preconditions, the packed hidden rows; the sample's maxima, tau; the candidate segments;
    // the refined lists with their counts
    const struct { dae_buf& b; size_t bytes; } bufs[] = {
        {tc->row_bad, Bpad * sizeof(int)},
        {tc->mix_fhat, Bpad * sizeof(unsigned)},
        {tc->h_packed16, (size_t)pl.n_rg * (pl.NSD + pl.NST) * pl.RB * 64 * sizeof(uint4)},
        {tc->gmax, Bpad * pl.ld_s * sizeof(float)},
        {tc->tau, Bpad * sizeof(float)},
        {tc->sample_top, Bpad * (sizeof(uint2) + sizeof(int))},
        {tc->cand, (size_t)pl.nb * Bpad * pl.cap * sizeof(uint4)},
        {tc->cand_cnt, (size_t)pl.nb * Bpad * sizeof(int)},
        {tc->refined, Bpad * MX_REF_CAP * sizeof(uint2) + Bpad * sizeof(int)},
        {tc->refstat, Bpad * 2 * sizeof(int)},
    };
    for (const auto& r : bufs) { rc = dae_reserve(tc, r.b, r.bytes); if (rc) return rc; }
    rc = dae_ensure_guard(tc); if (rc) return rc;
    tc->h16_geom_key = -1;                                       // (the buffer no longer holds a plain image's pad region)
    tc->refstat_rows = B;

    // ---- prep / pack
    rc = dae_launch_mix_prep_pack(tc, pl, pd.H, pt.H, c); if (rc) return rc;
    // ---- sample: lower bounds over the head of the list ...
    rc = dae_launch_mix_pass(tc, pl, true, pd, pt, order, c); if (rc) return rc;
    // ---- ... -> tau
    float* samp = static_cast<float*>(tc->gmax.p);
    uint2* top = static_cast<uint2*>(tc->sample_top.p);
    rc = dae_launch_tau_select(tc, samp, pl.ld_s, (int)pl.ld_s, samp, 0, 0, order, 0, B, k, seed_row_ptr, static_cast<float*>(tc->tau.p),
                               top, 1, reinterpret_cast<int*>(top + Bpad), nullptr);         // (no sample list: count 0; no live lists)
    if (rc) return rc;
    // ---- filter: upper bounds over every rankable tile
    dae_note_plan(pl.last);
    rc = dae_launch_mix_pass(tc, pl, false, pd, pt, order, c); if (rc) return rc;
    // ---- refine (+ selection, when it fits the launch: pl.fuse)
    rc = dae_launch_mix_refine(tc, pl, pd, pt, c); if (rc) return rc;
    // ---- selection over the refined lists
    if (!pl.fuse) {
        uint2* rf = static_cast<uint2*>(tc->refined.p);
        dae_topk_args ta;
        memset(&ta, 0, sizeof(ta));
        ta.B = B; ta.k = k;
        ta.bitmap_base = 0; ta.bitmap_n = pl.n_valid_col;
        ta.seed_row_ptr = seed_row_ptr; ta.seed_col = seed_col;
        ta.out_kind = DAE_OUT_LOGIT;                             // the mixed score is a probability already: it goes out as it is
        ta.out_score = out_score; ta.out_idx = out_idx;
        dae_pair_group gr{rf, reinterpret_cast<int*>(rf + Bpad * MX_REF_CAP), 0, MX_REF_CAP, 0, 1, 0};
        dae_pair_group g_none{nullptr, nullptr, 0, 0, 0, 0, 0};
        rc = dae_launch_topk_pairs(tc, gr, g_none, ta);
        if (rc) return rc;
    }
    // ---- audit
    return dae_launch_mix_audit(tc, dc, pl.n_valid_col, c);
}
