// score.hip -- the launch sequences of the scoring path behind dae_decode_dense / dae_decode_topk / dae_score_topk* and the
// titled calls: pack or encode the hidden rows, plan the call (score_plan.h dae_plan_topk), reserve scratch, launch.  The
// kernels are those of decode_*.hip, tau_select.hip, topk.hip, refine.hip, audit.hip and mix_*.hip; here live only the two fill kernels.
#include <climits>

#include "dae_internal.h"

namespace {

thread_local int32_t g_last_plan[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // dae_last_plan: dae_score_plan::last of this thread's last call

int prof_begin(dae_ctx* ctx)
{
    if (!ctx->prof_on) return DAE_OK;
    if (ctx->prof_used + 2 > ctx->prof_ev.size()) {
        for (int i = 0; i < 2; ++i) {
            hipEvent_t ev;
            DAE_HIP_CHECK(ctx, hipEventCreate(&ev));
            ctx->prof_ev.push_back(ev);
        }
    }
    // The pair is handed to the next decode launch (hipExtLaunchKernelGGL start / stop events): it then
    // times the kernel itself, like rocprofv3's kernel trace.  Events recorded on the stream around the
    // launch would add the dispatch gap on both sides (measured 167 vs 154 us for the same launches).  The launch that takes
    // the pair disarms (dae_take_profile_events); the callers disarm behind a launch that took none.
    ctx->prof_armed = true;
    return DAE_OK;
}

dae_rowgeom geom_for(int dtype, int B, int Hp)
{
    return dtype == DAE_DTYPE_F32 ? dae_row_geometry(B, Hp) : dae_row_geometry_bf16(B, Hp);
}

// The pad rows / pad k of a packed hidden image are never written by the encode kernel: zero them once per (B, H, R_TILE) and
// buffer.  bytes = 0: the caller has just rewritten the whole image, pads included (pack_hidden) -- only noted.
int hidden_pads_zeroed(dae_ctx* ctx, long long& key, void*& ptr, const dae_buf& img, size_t bytes, int B, int H, int R_TILE)
{
    const long long want = dae_hidden_geom_key(B, H, R_TILE);
    if (key == want && ptr == img.p) return DAE_OK;
    if (bytes) DAE_HIP_CHECK(ctx, hipMemsetAsync(img.p, 0, bytes, ctx->stream));
    key = want; ptr = img.p;
    return DAE_OK;
}

// the rows' max |h - 0.5| by quarters, published by whoever writes the packed fp32 hidden image (dae_ctx::row_d)
int reserve_row_d(dae_ctx* ctx, const dae_rowgeom& g)
{
    ctx->row_d_fresh = false;
    return dae_reserve(ctx, ctx->row_d, (size_t)g.Bpad * 4 * sizeof(float));
}

// want_d: the call ranks (dae_decode_topk) -- the packing launch also publishes the rows' d for the threshold sample's skip
int pack_hidden(dae_ctx* ctx, int dtype, const float* h, int B, int H, const dae_rowgeom& g, bool want_d = false)
{
    if (dtype == DAE_DTYPE_BF16_EXACT) {
        // the bound behind the exact mode holds for hidden rows in [0, 1]: the packing pass flags the others
        int rc = dae_reserve(ctx, ctx->row_bad, (size_t)g.Bpad * sizeof(int));
        if (rc) return rc;
        return dae_launch_pack_h_bf16(ctx, h, B, H, g, static_cast<int*>(ctx->row_bad.p));
    }
    if (dtype == DAE_DTYPE_F32) {
        int rc = want_d ? reserve_row_d(ctx, g) : DAE_OK;
        if (rc) return rc;
        ctx->row_d_fresh = false;
        rc = dae_launch_pack_h(ctx, h, B, H, g, want_d ? static_cast<float*>(ctx->row_d.p) : nullptr);   // rewrites the whole image incl. zero pads
        if (rc) return rc;
        ctx->row_d_fresh = want_d;
        return hidden_pads_zeroed(ctx, ctx->h_geom_key, ctx->h_geom_ptr, ctx->h_packed, 0, B, H, g.R_TILE);
    }
    return dae_launch_pack_h_bf16(ctx, h, B, H, g);
}

const dae_packed* packed_for(dae_ctx* ctx, int dtype, int H)
{
    const dae_packed* pk = dtype == DAE_DTYPE_F32 ? &ctx->pk_f32 : &ctx->pk_bf16;
    if (!pk->valid) { dae_fail(ctx, DAE_ERR_STATE, "decoder weights not prepacked for dtype %d", dtype); return nullptr; }
    if (dtype == DAE_DTYPE_BF16_EXACT && !pk->exact) {
        dae_fail(ctx, DAE_ERR_STATE, "decoder weights not prepacked with DAE_DTYPE_BF16_EXACT"); return nullptr;
    }
    if (pk->H != H) { dae_fail(ctx, DAE_ERR_ARG, "H=%d does not match prepacked H=%d", H, pk->H); return nullptr; }
    return pk;
}

}  // namespace

// dae_mix_topk_exact leaves its geometry in the same words (mix_plan.h dae_plan_mix): S = 1, fused = 0; ntiles = the ranked tiles it walks
void dae_note_plan(const int32_t last[8])
{
    memcpy(g_last_plan, last, 8 * sizeof(int32_t));
}

extern "C" {

namespace {      // (inside extern "C": kernel traces show the two by their plain names)
__global__ __launch_bounds__(256) void fill_f32_kernel(float* dst, int n, float v)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = v;
}

// what the selection kernels leave in the slots of a list with no entry: score -inf, index -1
__global__ __launch_bounds__(256) void fill_pad_kernel(float* score, int32_t* idx, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) { score[i] = -__builtin_inff(); idx[i] = -1; }
}
}  // namespace

/* geometry of the last dae_decode_topk / dae_mix_topk_exact on this thread:
 * {R_TILE, n_rg, nb_rg, S, n_sample_tiles, n_filter_tiles, fused(0/1), ntiles}; ntiles = the tiles the call walks, i.e. those
 * with a ranked column (topk_phase_a), not the image's */
int dae_last_plan(int32_t out[8])
{
    if (!out) return DAE_ERR_ARG;
    memcpy(out, g_last_plan, sizeof(g_last_plan));
    return DAE_OK;
}

int dae_decode_dense(dae_ctx* ctx, const float* h, int B, int H, int dtype, int apply_sigmoid,
                     float* out, int64_t ld_out)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!h || !out) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (dtype != DAE_DTYPE_F32 && dtype != DAE_DTYPE_BF16) return dae_fail(ctx, DAE_ERR_ARG, "unknown dtype %d", dtype);
    const dae_packed* pk = packed_for(ctx, dtype, H);
    if (!pk) return DAE_ERR_STATE;
    const int ncols = pk->col_hi - pk->col_lo;
    if (ld_out < ncols) return dae_fail(ctx, DAE_ERR_ARG, "ld_out=%lld < %d columns", (long long)ld_out, ncols);
    if (B <= 0) return DAE_OK;
    const dae_rowgeom g = geom_for(dtype, B, pk->Hp);
    int rc = pack_hidden(ctx, dtype, h, B, H, g);
    if (rc) return rc;
    dae_tileset ts{pk->ntiles, 1, 0, static_cast<const int*>(pk->ident.p)};
    rc = prof_begin(ctx); if (rc) return rc;
    rc = dae_launch_decode_dense_f32(ctx, g, B, ts, apply_sigmoid, INT_MAX, out, ld_out, 0, dtype);
    if (rc) return rc;
    ctx->prof_armed = false;
    return DAE_OK;
}

}  // extern "C"

static int fill_tau_neg_inf(dae_ctx* ctx, float* tau_dst, int B)
{
    if (!tau_dst) return DAE_OK;
    // (-inf: 0xFF800000 is not a byte pattern hipMemset can write)
    hipLaunchKernelGGL(fill_f32_kernel, dim3((B + 255) / 256), dim3(256), 0, ctx->stream, tau_dst, B, -__builtin_inff());
    DAE_CHECK_LAUNCH(ctx, "fill_f32_kernel");
    return DAE_OK;
}

// the live lists of a filter launch of n_filter tiles (dae_score_plan::build_live): ctx->live = [n_rg] counts, padded | [n_rg]
// [n_filter] tile ids, and the context's skip counters (zeroed when first reserved)
static int reserve_live(dae_ctx* ctx, const dae_rowgeom& g, int n_filter, int** live_cnt, int** live_list)
{
    const size_t cnt_ints = (size_t)dae_round_up(g.n_rg, 64);
    int rc = dae_reserve(ctx, ctx->live, (cnt_ints + (size_t)g.n_rg * n_filter) * sizeof(int));
    if (rc) return rc;
    if (!ctx->skip_stat.p) {
        rc = dae_reserve(ctx, ctx->skip_stat, 4 * sizeof(unsigned long long));
        if (rc) return rc;
        DAE_HIP_CHECK(ctx, hipMemsetAsync(ctx->skip_stat.p, 0, 4 * sizeof(unsigned long long), ctx->stream));
    }
    *live_cnt = static_cast<int*>(ctx->live.p);
    *live_list = *live_cnt + cnt_ints;
    return DAE_OK;
}

// ---- decode + rank with the hidden tile already packed in the context for geometry g, in two halves -----------------
// topk_phase_a: the plan, the threshold sample (phase A) and tau_select -> tau_dst[B] (a valid lower bound, per row, of
//   the k-th largest rankable non-seed logit among THIS image's columns); small problems: the dense logits, tau = -inf.
//   own_tau: phase B will be given exactly these thresholds (decode_topk_core; not dae_score_topk_begin, whose caller may
//   pass exchanged, raised ones to dae_score_topk_finish) -- the threshold launch may then build the filter launch's live
//   lists itself (dae_score_plan::live_in_tau).
// topk_phase_b: the filter launch with tau_src[B] (the same values, or larger ones that are still lower bounds of the
//   row's k-th largest logit over ALL shards: dae_score_topk_finish), the exact mode's refine step, the final selection.
// What phase B needs from phase A travels in ctx->tk.
// dtype_in == DAE_DTYPE_BF16_EXACT: h32 = the fp32 hidden rows [B][H] the packed bf16 image was rounded from,
// row_bad (nullable) = rows of h32 outside [0, 1]
static int topk_phase_a(dae_ctx* ctx, const dae_packed* pk, const dae_rowgeom& g, int B, int n_tracks,
                        const int32_t* seed_row_ptr, int k, int dtype_in, float* tau_dst, bool own_tau)
{
    int rc;
    dae_topk_state& tk = ctx->tk;
    tk.valid = false;
    const dae_plan_in in{pk->ntiles, pk->col_lo, pk->col_hi, pk->Hp, pk->ub_valid && pk->tile_ub.p, g, n_tracks, k, dtype_in,
                         ctx->mixT != nullptr, ctx->overlap_hint, ctx->filter_skip, own_tau, B};
    const dae_score_plan pl = dae_plan_topk(in);
    memcpy(g_last_plan, pl.last, sizeof(pl.last));
    if (pl.bad_mix) return dae_fail(ctx, DAE_ERR_ARG, "DAE_DTYPE_BF16_EXACT is not available with dae_set_score_mix");
    tk.pk = pk; tk.g = g; tk.B = B; tk.k = k; tk.plan = pl; tk.order = nullptr; tk.sample_cnt = nullptr; tk.live_built = false;
    if (pl.ntiles == 0) {                                  // no GEMM launch; tau = -inf, and phase B pads every slot
        rc = fill_tau_neg_inf(ctx, tau_dst, B);
        tk.valid = rc == DAE_OK;
        return rc;
    }

    // phase A (or the whole problem when it is small): dense logits of the sampled tiles
    rc = dae_reserve(ctx, ctx->sample, (size_t)B * pl.ld_s * sizeof(float));
    if (rc) return rc;
    float* sample = static_cast<float*>(ctx->sample.p);
    const int* order = static_cast<const int*>(pk->ident.p);
    if (pl.fused) {
        dae_packed& pkm = pl.dtype == DAE_DTYPE_F32 ? ctx->pk_f32 : ctx->pk_bf16;
        rc = dae_launch_tile_order(ctx, pkm, pl.nrank, pl.n_samp, pl.S);
        if (rc) return rc;
        order = static_cast<const int*>(pkm.order.p);
        if (pl.use_band) {                                 // the list is this context's, rebuilt when the order or the geometry changes
            const dae_rowgeom& gA = pl.gA;
            const void* band_was = ctx->tile_band.p;
            rc = dae_reserve(ctx, ctx->tile_band, (size_t)pl.ntiles * sizeof(int));
            if (rc) return rc;
            if (ctx->tile_band.p != band_was) ctx->band_gen = -1;
            if (ctx->band_gen != pkm.order_gen || ctx->band_nsamp != pl.n_samp || ctx->band_nbrg != gA.nb_rg || ctx->band_waves != gA.waves) {
                rc = dae_launch_tile_band(ctx, order, pl.ntiles, pl.n_samp, gA.nb_rg, gA.waves, static_cast<int*>(ctx->tile_band.p));
                if (rc) return rc;
                ctx->band_gen = pkm.order_gen; ctx->band_nsamp = pl.n_samp; ctx->band_nbrg = gA.nb_rg; ctx->band_waves = gA.waves;
            }
            order = static_cast<const int*>(ctx->tile_band.p);
        }
    }
    tk.order = order;
    dae_tileset tsA{pl.n_samp, pl.fused ? pl.S : 1, pl.fused ? 3 : 0, order};
    float* gmax = nullptr;
    if (pl.fused || pl.mixed) {                            // (the mix lives in the GMAX / FILTER epilogues)
        rc = dae_reserve(ctx, ctx->gmax, (size_t)B * pl.ld_g * sizeof(float));
        if (rc) return rc;
        gmax = static_cast<float*>(ctx->gmax.p);
    }
    // SKIPPED SAMPLE TILES (dae_score_plan::sample_skip, under dae_set_filter_skip): the sample in half row groups knows, before it
    // decodes anything, a lower bound of every row's threshold (from the columns' lower bounds lo_c) and skips the tiles whose upper
    // bound stays below it.  The bound table belongs to the tile order and the launch geometry, like the band list; the rows' d comes
    // from the launch that wrote the packed hidden image (none published for this image: the full walk).
    dae_sample_skip sk{};
    float* env = nullptr;
    const bool d_fresh = ctx->row_d_fresh;
    ctx->row_d_fresh = false;                              // (taken: the next sample needs its own image's)
    if (pl.sample_skip && ctx->filter_skip) {
        const int n_beta = g.nb_rg * 32 < 4096 ? g.nb_rg * 32 : 4096;
        const void* tab_was = ctx->samp_tab.p;
        rc = dae_reserve(ctx, ctx->samp_tab, (4 + (size_t)2 * pl.n_samp + n_beta + DAE_PROOF_ENV) * sizeof(float));
        if (rc) return rc;
        if (ctx->samp_tab.p != tab_was) ctx->tab_gen = -1;
        if (!ctx->sskip_stat.p) {                          // (the counter words | the decoded-tile table and the half groups' pairs, which nobody clears)
            rc = dae_reserve(ctx, ctx->sskip_stat, DAE_SSKIP_SLOTS * (sizeof(unsigned long long) + sizeof(unsigned)) + DAE_SSKIP_PAIRS * sizeof(float2));
            if (rc) return rc;
            DAE_HIP_CHECK(ctx, hipMemsetAsync(ctx->sskip_stat.p, 0, DAE_SSKIP_SLOTS * sizeof(unsigned long long), ctx->stream));
        }
        float* head = static_cast<float*>(ctx->samp_tab.p);
        float2* ub = reinterpret_cast<float2*>(head + 4);
        float* beta = head + 4 + (size_t)2 * pl.n_samp;
        env = beta + n_beta;                               // the envelope of the filter list: the same table, the same size in every call
        if (ctx->tab_gen != pk->order_gen || ctx->tab_nsamp != pl.n_samp || ctx->tab_nbrg != g.nb_rg || ctx->tab_waves != g.waves ||
            ctx->tab_nfilter != pl.n_filter || ctx->tab_nrank != pl.nrank) {
            rc = dae_launch_sample_bounds(ctx, *pk, order, pl.n_samp, g.nb_rg, g.waves, pl.nrank, head, ub, beta, n_beta, pl.n_filter, env);
            if (rc) return rc;
            ctx->tab_gen = pk->order_gen; ctx->tab_nsamp = pl.n_samp; ctx->tab_nbrg = g.nb_rg; ctx->tab_waves = g.waves;
            ctx->tab_nfilter = pl.n_filter; ctx->tab_nrank = pl.nrank;
        }
        if (d_fresh && 2 * g.grid <= DAE_SSKIP_SLOTS && ctx->row_d.p && ctx->row_d.bytes >= (size_t)g.Bpad * 4 * sizeof(float)) {
            // SKIPPED TILES ARE NOT STORED: with the workgroup-per-row threshold kernel behind it, the launch writes which wave-tiles
            // it decoded into a table (2 g.grid <= DAE_SSKIP_SLOTS words behind the counters) and leaves the others' maxima and
            // dense slots as they stand; the threshold launch takes the table and reads the decoded ones only.  The wave-per-row
            // kernel keeps the dense exchange (-inf stored and read back)
            unsigned long long* const stat = static_cast<unsigned long long*>(ctx->sskip_stat.p);
            unsigned* const tab = dae_tau_wave_per_row(B, pl.ld_g, pl.ld_s) ? nullptr : reinterpret_cast<unsigned*>(stat + DAE_SSKIP_SLOTS);
            // ... and every half group's {dq, tau_safe} behind the table (2 n_rg <= DAE_SSKIP_PAIRS: nb_rg >= DAE_NUM_XCD)
            float2* const pair = reinterpret_cast<float2*>(reinterpret_cast<unsigned*>(stat + DAE_SSKIP_SLOTS) + DAE_SSKIP_SLOTS);
            sk = dae_sample_skip{ub, beta, n_beta, head, static_cast<const float*>(ctx->row_d.p), seed_row_ptr, k, stat, tab, pair};
            ctx->sskip_launches += 1;
            ctx->sskip_planned += (unsigned long long)((B + 63) / 64) * (unsigned long long)pl.n_samp;   // half groups with a real row
        }
    }
    if (!pl.fused) { rc = prof_begin(ctx); if (rc) return rc; }
    // (gA != g only with per-wave groups: the generic kernels run on the filter launch's geometry)
    rc = dae_launch_decode_dense_f32(ctx, pl.wave_groups ? pl.gA : g, B, tsA, 0, pl.n_valid_col, pl.whole_b ? nullptr : sample, pl.ld_s,
                                     1, pl.dtype, gmax, pl.ld_g, pl.gmax_per_wave, pl.exact ? 1 : 0, sk.ub ? &sk : nullptr);
    if (rc) return rc;
    if (!pl.fused) {                                       // phase B ranks the dense rows; no threshold exists
        ctx->prof_armed = false;
        rc = fill_tau_neg_inf(ctx, tau_dst, B);
        tk.valid = rc == DAE_OK;
        return rc;
    }

    // tau: the (k + n_seeds)-th largest of the sample's group maxima (written by the phase-A launch: the maximum
    // over the tiles a workgroup decodes together, per position in the tile) -- a valid lower bound of the row's k-th
    // largest rankable non-seed logit -- and, from the same launch, the sample logits >= tau as one flat list per row.
    // No selection over the 15 k dense sample logits of a row happens any more.
    const int64_t pstride = pl.ld_s;                       // worst case (tau = -inf): every sample logit survives
    rc = dae_reserve(ctx, ctx->sample_top, ((size_t)g.Bpad * pstride) * sizeof(uint2) + (size_t)g.Bpad * sizeof(int));
    if (rc) return rc;
    tk.sample_cnt = reinterpret_cast<int*>(static_cast<uint2*>(ctx->sample_top.p) + (size_t)g.Bpad * pstride);
    // SKIPPED TILES, the thresholds being phase B's own (dae_score_plan::live_in_tau): the threshold launch compacts, per row
    // group, the filter launch's tiles that can hold a logit >= tau for one of its rows -- in the workgroup of the group's
    // last row to finish, so the step's chain of launches carries no launch for it
    dae_tau_live lv{};
    if (pl.live_in_tau) {
        constexpr size_t n_arrive = 64;                        // (a slab is at most DAE_ROW_SLAB = 4096 rows: 32 groups of 128)
        if ((size_t)g.n_rg > n_arrive) return dae_fail(ctx, DAE_ERR_STATE, "%d row groups in one threshold launch", g.n_rg);
        int* lc; int* ll;
        rc = reserve_live(ctx, g, pl.n_filter, &lc, &ll);
        if (rc) return rc;
        rc = dae_reserve(ctx, ctx->live_sync, n_arrive * sizeof(unsigned) + (size_t)g.Bpad * sizeof(double));
        if (rc) return rc;
        if (ctx->live_sync_zeroed != ctx->live_sync.p || ctx->live_sync_zeroed_bytes != ctx->live_sync.bytes) {
            DAE_HIP_CHECK(ctx, hipMemsetAsync(ctx->live_sync.p, 0, n_arrive * sizeof(unsigned), ctx->stream));
            ctx->live_sync_zeroed = ctx->live_sync.p; ctx->live_sync_zeroed_bytes = ctx->live_sync.bytes;
        }
        unsigned* arrive = static_cast<unsigned*>(ctx->live_sync.p);
        lv = dae_tau_live{static_cast<const float4*>(ctx->h_packed.p), B, pk->H, pk->Hp / DAE_KG,
                          static_cast<const float*>(pk->tile_ub.p), pk->ntiles, pl.nrank, order + pl.n_samp, pl.n_filter,
                          reinterpret_cast<unsigned long long*>(arrive + n_arrive), arrive, lc, ll,
                          static_cast<unsigned long long*>(ctx->skip_stat.p), nullptr, nullptr};
        // THE EMPTY LIST PROVED: where this call's sample ran with the skip and the table, the launch has the half groups' pairs and
        // the list's envelope, and a row group they prove empty runs no arrival tail (tau_select.hip; DESIGN.md sections 2 and 4)
        if (sk.ub && sk.tab) { lv.pair = sk.pair; lv.env = env; }
    }
    rc = dae_launch_tau_select(ctx, gmax, pl.ld_g, (int)pl.ld_g, pl.whole_b ? gmax : sample, pl.whole_b ? 0 : pl.ld_s,
                               pl.whole_b ? 0 : (int)pl.ld_s, order, pk->col_lo, B, k,
                               seed_row_ptr, tau_dst, static_cast<uint2*>(ctx->sample_top.p),
                               pstride, tk.sample_cnt, pl.live_in_tau ? &lv : nullptr, sk.ub ? sk.tab : nullptr, g.nb_rg);
    if (rc) return rc;
    tk.live_built = pl.live_in_tau;
    if (pl.live_in_tau) ctx->live_n_rg = g.n_rg;
    tk.valid = true;
    return DAE_OK;
}

static int topk_phase_b(dae_ctx* ctx, const float* tau_src, const int32_t* seed_row_ptr, const int32_t* seed_col,
                        int out_kind, float* out_score, int32_t* out_idx, const float* h32, const int* row_bad,
                        bool tau_is_foreign = false)
{
    int rc;
    dae_topk_state& tk = ctx->tk;
    if (!tk.valid) return dae_fail(ctx, DAE_ERR_STATE, "no scoring call in progress on this context");
    tk.valid = false;
    if (!tk.live_built) ctx->live_n_rg = 0;                // (dae_filter_skip_last: no live lists unless phase A's launch or the one below builds them)
    const dae_packed* pk = tk.pk;
    const dae_rowgeom& g = tk.g;
    const dae_score_plan& pl = tk.plan;
    const int B = tk.B, k = tk.k, dtype = pl.dtype;
    if (pl.mixed) out_kind = DAE_OUT_LOGIT;                // the mixed score is a probability already: it goes out as it is
    dae_topk_args ta;
    memset(&ta, 0, sizeof(ta));
    ta.B = B; ta.k = k;
    ta.bitmap_base = pk->col_lo; ta.bitmap_n = pl.nrank;
    ta.seed_row_ptr = seed_row_ptr; ta.seed_col = seed_col;
    ta.out_kind = out_kind; ta.out_score = out_score; ta.out_idx = out_idx;
    // an exchanged threshold (dae_score_topk_finish) also cuts what the sample left behind under the image's own, lower
    // one; with the own threshold nothing below it was ever kept.  (Exact mode: the lists hold recomputed fp32 logits
    // by then, and tau bounds the fp32 ranking.)
    ta.row_min = (tau_is_foreign && !pl.mixed) ? tau_src : nullptr;
    // batches in flight on other streams (dae_set_overlap_hint), bf16 arithmetic: the filter launch leaves ~112 registers
    // per SIMD lane and 94 KB of LDS on every CU -- the 256-thread selection fits there and runs UNDER the other batch's
    // launch (alone it is slower: 14 vs 11 us); the fp32 launches fill the LDS, nothing fits next to them
    ta.prefer_small = (ctx->overlap_hint && dtype == DAE_DTYPE_BF16) ? 1 : 0;
    if (pl.ntiles == 0) {                            // nothing to rank: the padding of a short list in every slot
        const int n = B * k;                               // (B <= DAE_ROW_SLAB, k <= DAE_MAX_K_DEEP: at most 2^24)
        hipLaunchKernelGGL(fill_pad_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, out_score, out_idx, n);
        DAE_CHECK_LAUNCH(ctx, "fill_pad_kernel");
        return DAE_OK;
    }
    if (!pl.fused) {
        dae_dense_src ds{static_cast<const float*>(ctx->sample.p), pl.ld_s, (int)pl.ld_s, pk->col_lo, 1, nullptr};
        return dae_launch_topk_dense(ctx, ds, ta);
    }

    // phase B: everything else through the threshold filter
    const int n_filter = pl.n_filter, cap = pl.cap;
    rc = dae_reserve(ctx, ctx->cand, (size_t)g.nb_rg * g.Bpad * cap * sizeof(uint2));
    if (rc) return rc;
    rc = dae_reserve(ctx, ctx->cand_cnt, (size_t)g.nb_rg * g.Bpad * sizeof(int));
    if (rc) return rc;
    dae_tileset tsB{n_filter, pl.S, 3, pl.whole_b ? tk.order : tk.order + pl.n_samp};
    // SKIPPED TILES (dae_score_plan::build_live): the filter launch walks, per row group, the tiles of tsB that can hold a logit
    // >= tau for one of its rows.  Where the thresholds are the ones phase A computed for this very launch (live_in_tau), its
    // threshold launch has built the lists already and they are only handed on.  Otherwise -- thresholds from elsewhere
    // (dae_score_topk_finish), or the wave-per-row threshold kernel -- they are known here and one small launch compacts the
    // lists from them.  Issued before the gate: it runs while the other batch's filter launch holds the matrix cores.
    const int* live_cnt = nullptr; const int* live_list = nullptr;
    if (pl.build_live) {
        int* lc; int* ll;
        rc = reserve_live(ctx, g, n_filter, &lc, &ll);     // (live_built: the same pointers phase A gave its launch)
        if (rc) return rc;
        if (!tk.live_built) {
            rc = dae_launch_live_tiles(ctx, *pk, g, B, tsB.list, n_filter, tau_src, pl.nrank, lc, ll,
                                       static_cast<unsigned long long*>(ctx->skip_stat.p));
            if (rc) return rc;
        }
        live_cnt = lc; live_list = ll; ctx->live_n_rg = g.n_rg;
    }
    // dae_set_decode_gate: the dominant launch takes every CU, so two of them in flight on two streams only queue
    // behind each other; the gate makes this one wait for the other context's and announces its own end
    if (ctx->gate_wait) DAE_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, ctx->gate_wait, 0));
    rc = prof_begin(ctx); if (rc) return rc;
    rc = dae_launch_decode_filter_f32(ctx, g, B, tsB, tau_src, pl.n_valid_col, static_cast<uint2*>(ctx->cand.p),
                                      static_cast<int*>(ctx->cand_cnt.p), cap, dtype, pl.exact ? 2 : 0, live_cnt, live_list);
    if (rc) return rc;
    ctx->prof_armed = false;
    if (ctx->gate_record) DAE_HIP_CHECK(ctx, hipEventRecord(ctx->gate_record, ctx->stream));

    // final: exact top-k of (sample survivors) U (phase-B survivors), seeds removed
    dae_pair_group g0{static_cast<const uint2*>(ctx->sample_top.p), tk.sample_cnt, 0, pl.ld_s, 0, 1, 0};
    dae_pair_group g1{static_cast<const uint2*>(ctx->cand.p), static_cast<const int*>(ctx->cand_cnt.p),
                      (int64_t)g.Bpad * cap, cap, g.Bpad, g.nb_rg, 0};
    if (pl.exact) {
        rc = dae_ensure_guard(ctx);                        // the guard words of this context, zero until a bound fails
        if (rc) return rc;
        dae_exact_src xs{h32, (int64_t)pk->H, pk->H, static_cast<const float*>(pk->W32.p),
                         static_cast<const float*>(pk->bias.p), pk->col_lo, row_bad,
                         static_cast<const float*>(pk->eps.p) + (size_t)pk->ntiles * 32,
                         static_cast<const float*>(pk->eps.p), static_cast<int*>(ctx->guard.p)};
        // the survivors of a row leave the refine launch as ONE compact list (group 0 of the selection: the threshold kernel
        // emits no sample survivors in this mode), the per-workgroup lists of the row are emptied
        rc = dae_reserve(ctx, ctx->refined, (size_t)g.Bpad * DAE_REFINED_CAP * sizeof(uint2) + (size_t)g.Bpad * sizeof(int));
        if (rc) return rc;
        uint2* rf = static_cast<uint2*>(ctx->refined.p);
        int* rf_cnt = reinterpret_cast<int*>(rf + (size_t)g.Bpad * DAE_REFINED_CAP);
        rc = dae_reserve(ctx, ctx->refstat, (size_t)g.Bpad * 2 * sizeof(int));
        if (rc) return rc;
        ctx->refstat_rows = B;
        // k <= 512: the refine launch ends the call itself -- a row's workgroup has its recomputed survivors in LDS, takes the
        // seeds out and orders the k best there (round 5: the selection launch that read them back was 10.6 / 24.0 us of the
        // step at 256 / 1024 rows); larger k keeps the two launches
        const bool fuse = dae_exact_refine_can_fuse(ta);
        rc = dae_launch_exact_refine(ctx, g1, xs, B, k, seed_row_ptr, rf, rf_cnt, DAE_REFINED_CAP, static_cast<int*>(ctx->refstat.p),
                                     fuse ? &ta : nullptr);
        // every audit_every-th launch: a sample of the columns the filter launch DROPPED against its own promise (audit.hip) --
        // behind the refine launch, so that the lists are not held up; its verdict lands in the guard words the callers fetch
        if (!rc && ctx->audit_every > 0 && ctx->audit_tiles > 0 && (++ctx->audit_seq % (uint64_t)ctx->audit_every) == 0)
            rc = dae_launch_exact_audit(ctx, g, B, xs, pl.nrank, ctx->audit_tiles);
        if (rc || fuse) return rc;
        dae_pair_group gr{rf, rf_cnt, 0, DAE_REFINED_CAP, 0, 1, 0};
        return dae_launch_topk_pairs(ctx, gr, g1, ta);
    }
    return dae_launch_topk_pairs(ctx, g0, g1, ta);
}

static int decode_topk_core(dae_ctx* ctx, const dae_packed* pk, const dae_rowgeom& g, int B,
                            int n_tracks, const int32_t* seed_row_ptr, const int32_t* seed_col,
                            int k, int out_kind, float* out_score, int32_t* out_idx, int dtype_in,
                            const float* h32 = nullptr, const int* row_bad = nullptr)
{
    int rc = dae_reserve(ctx, ctx->tau, (size_t)g.Bpad * sizeof(float));
    if (rc) return rc;
    rc = topk_phase_a(ctx, pk, g, B, n_tracks, seed_row_ptr, k, dtype_in, static_cast<float*>(ctx->tau.p), true);
    if (rc) return rc;
    return topk_phase_b(ctx, static_cast<const float*>(ctx->tau.p), seed_row_ptr, seed_col, out_kind, out_score, out_idx,
                        h32, row_bad);
}

// k of a ranking call: DAE_MAX_K_DEEP for fp32 / bf16 arithmetic; the exact mode (its refine launch holds DAE_MAX_K winners) and
// a context under dae_set_score_mix keep DAE_MAX_K
static int check_k(dae_ctx* ctx, int dtype, int k)
{
    const bool keeps = dtype == DAE_DTYPE_BF16_EXACT || ctx->mixT != nullptr;
    const int k_max = keeps ? DAE_MAX_K : DAE_MAX_K_DEEP;
    if (k < 1 || k > k_max)
        return dae_fail(ctx, DAE_ERR_ARG, "k=%d out of [1,%d]%s", k, k_max,
                        !keeps ? "" : dtype == DAE_DTYPE_BF16_EXACT ? " (DAE_DTYPE_BF16_EXACT)" : " (dae_set_score_mix)");
    return DAE_OK;
}

int dae_check_topk_args(dae_ctx* ctx, int dtype, int k, const int32_t* seed_row_ptr,
                        const int32_t* seed_col, const void* out_score, const void* out_idx)
{
    if (!out_score || !out_idx) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (!dae_known_dtype(dtype)) return dae_fail(ctx, DAE_ERR_ARG, "unknown dtype %d", dtype);
    const int rc_k = check_k(ctx, dtype, k);
    if (rc_k) return rc_k;
    if ((seed_row_ptr == nullptr) != (seed_col == nullptr))
        return dae_fail(ctx, DAE_ERR_ARG, "seed_row_ptr and seed_col must both be given or both null");
    return DAE_OK;
}

// Batches are processed in slabs of DAE_ROW_SLAB rows: the worst-case candidate capacity grows with
// (rows x tiles per workgroup), and a slab keeps it at a few GB whatever batch the caller passes.
constexpr int DAE_ROW_SLAB = 4096;

// slab(r0, nb, seed_row_ptr, out_score, out_idx): rows [r0, r0 + nb) of a call of B rows, with its per-row arguments shifted
// (seed_row_ptr holds ABSOLUTE offsets into seed_col, so a slab is a pointer shift)
template <class Slab>
static int for_row_slabs(int B, int k, const int32_t* seed_row_ptr, float* out_score, int32_t* out_idx, Slab&& slab)
{
    for (int r0 = 0; r0 < B; r0 += DAE_ROW_SLAB) {
        const int rc = slab(r0, B - r0 < DAE_ROW_SLAB ? B - r0 : DAE_ROW_SLAB, seed_row_ptr ? seed_row_ptr + r0 : nullptr,
                            out_score + (size_t)r0 * k, out_idx + (size_t)r0 * k);
        if (rc) return rc;
    }
    return DAE_OK;
}

// encode a slab's rows straight into the packed hidden image of `dtype` (+ the fp32 rows in the exact mode)
static int score_encode(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val,
                        const float* W_enc, const float* b_enc, int V, int H, int B, int dtype,
                        const dae_packed** pk_out, dae_rowgeom* g_out, const float** h32_out)
{
    if (!row_ptr || !W_enc || !b_enc) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (H <= 0 || (H % 4) != 0) return dae_fail(ctx, DAE_ERR_ARG, "H=%d must be a positive multiple of 4", H);
    if ((reinterpret_cast<uintptr_t>(W_enc) | reinterpret_cast<uintptr_t>(b_enc)) % 16)
        return dae_fail(ctx, DAE_ERR_ARG, "W_enc, b_enc must be 16-byte aligned");
    const dae_packed* pk = packed_for(ctx, dtype, H);
    if (!pk) return DAE_ERR_STATE;
    *pk_out = pk; *h32_out = nullptr;
    int rc;
    if (dtype != DAE_DTYPE_F32) {
        // encode stays fp32 (north_star: bf16 decode GEMM + fp32 encode / top-k); the hidden rows leave the encode
        // kernel rounded to bf16, already in the MFMA operand order (no [B,H] round trip, no re-tiling launch)
        const dae_rowgeom g16 = dae_row_geometry_bf16(B, pk->Hp);
        const int NS = pk->Hp / 16, RB16 = g16.R_TILE / 32;
        const size_t bytes16 = (size_t)g16.n_rg * NS * RB16 * 64 * sizeof(uint4);
        rc = dae_reserve(ctx, ctx->h_packed16, bytes16);
        if (rc) return rc;
        rc = hidden_pads_zeroed(ctx, ctx->h16_geom_key, ctx->h16_geom_ptr, ctx->h_packed16, bytes16, B, H, g16.R_TILE);
        if (rc) return rc;
        // exact mode: the fp32 rows as well -- the survivors of the bf16 filter are recomputed from them (the encoder's
        // sigmoid keeps them in [0, 1], the precondition of the bound: no row check needed)
        float* h32 = nullptr;
        if (dtype == DAE_DTYPE_BF16_EXACT) {
            rc = dae_reserve(ctx, ctx->h_scratch, (size_t)B * H * sizeof(float));
            if (rc) return rc;
            h32 = static_cast<float*>(ctx->h_scratch.p);
        }
        rc = dae_launch_encode(ctx, row_ptr, col, val, W_enc, b_enc, V, H, B, 1.0f, 1.0f, 0U, h32, nullptr, 0, RB16,
                               nullptr, nullptr, static_cast<unsigned short*>(ctx->h_packed16.p), NS);
        if (rc) return rc;
        *g_out = g16; *h32_out = h32;
        return DAE_OK;
    }
    const dae_rowgeom g = dae_row_geometry(B, pk->Hp);
    const int G = pk->Hp / DAE_KG, RB = g.R_TILE / 32;
    const size_t bytes = (size_t)g.n_rg * G * RB * 64 * sizeof(float4);
    rc = dae_reserve(ctx, ctx->h_packed, bytes);
    if (rc) return rc;
    rc = hidden_pads_zeroed(ctx, ctx->h_geom_key, ctx->h_geom_ptr, ctx->h_packed, bytes, B, H, g.R_TILE);
    if (rc) return rc;
    rc = reserve_row_d(ctx, g);
    if (rc) return rc;
    rc = dae_launch_encode(ctx, row_ptr, col, val, W_enc, b_enc, V, H, B, 1.0f, 1.0f, 0U, nullptr,
                           static_cast<float*>(ctx->h_packed.p), G, RB, nullptr, nullptr, nullptr, 0, static_cast<float*>(ctx->row_d.p));
    if (rc) return rc;
    ctx->row_d_fresh = true;
    *g_out = g;
    return DAE_OK;
}

extern "C" {

int dae_decode_topk(dae_ctx* ctx, const float* h, int B, int H, int dtype, int n_tracks,
                    const int32_t* seed_row_ptr, const int32_t* seed_col, int k, int out_kind,
                    float* out_score, int32_t* out_idx)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!h) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    int rc = dae_check_topk_args(ctx, dtype, k, seed_row_ptr, seed_col, out_score, out_idx);
    if (rc) return rc;
    const dae_packed* pk = packed_for(ctx, dtype, H);
    if (!pk) return DAE_ERR_STATE;
    return for_row_slabs(B, k, seed_row_ptr, out_score, out_idx, [&](int r0, int nb, const int32_t* srp, float* os, int32_t* oi) {
        const float* hs = h + (size_t)r0 * H;
        const dae_rowgeom g = geom_for(dtype, nb, pk->Hp);
        const int rc = pack_hidden(ctx, dtype, hs, nb, H, g, ctx->mixT == nullptr);      // (the mixed score never skips)
        if (rc) return rc;
        return decode_topk_core(ctx, pk, g, nb, n_tracks, srp, seed_col, k, out_kind, os, oi, dtype, hs,
                                static_cast<const int*>(ctx->row_bad.p));
    });
}

int dae_score_topk(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val,
                   const float* W_enc, const float* b_enc, int V, int H, int B, int dtype,
                   int n_tracks, const int32_t* seed_row_ptr, const int32_t* seed_col,
                   int k, int out_kind, float* out_score, int32_t* out_idx)
{
    if (!ctx) return DAE_ERR_ARG;
    int rc = dae_check_topk_args(ctx, dtype, k, seed_row_ptr, seed_col, out_score, out_idx);
    if (rc) return rc;
    if (B <= 0) return packed_for(ctx, dtype, H) ? DAE_OK : DAE_ERR_STATE;
    return for_row_slabs(B, k, seed_row_ptr, out_score, out_idx, [&](int r0, int nb, const int32_t* srp, float* os, int32_t* oi) {
        const dae_packed* pk; dae_rowgeom g; const float* h32;     // (row_ptr: absolute offsets into col / val, as the seeds')
        const int rc = score_encode(ctx, row_ptr ? row_ptr + r0 : row_ptr, col, val, W_enc, b_enc, V, H, nb, dtype, &pk, &g, &h32);
        if (rc) return rc;
        return decode_topk_core(ctx, pk, g, nb, n_tracks, srp, seed_col, k, out_kind, os, oi, dtype, h32, nullptr);
    });
}

int dae_score_topk_begin(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val,
                         const float* W_enc, const float* b_enc, int V, int H, int B, int dtype,
                         int n_tracks, const int32_t* seed_row_ptr, int k, float* tau_out)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!tau_out) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (!dae_known_dtype(dtype)) return dae_fail(ctx, DAE_ERR_ARG, "unknown dtype %d", dtype);
    if (const int rc_k = check_k(ctx, dtype, k)) return rc_k;
    if (B < 1 || B > DAE_ROW_SLAB) return dae_fail(ctx, DAE_ERR_ARG, "dae_score_topk_begin takes 1..%d rows (B=%d)", DAE_ROW_SLAB, B);
    if (ctx->mixT) return dae_fail(ctx, DAE_ERR_ARG, "dae_score_topk_begin is not available with dae_set_score_mix");
    const dae_packed* pk; dae_rowgeom g; const float* h32;
    int rc = score_encode(ctx, row_ptr, col, val, W_enc, b_enc, V, H, B, dtype, &pk, &g, &h32);
    if (rc) return rc;
    rc = topk_phase_a(ctx, pk, g, B, n_tracks, seed_row_ptr, k, dtype, tau_out, false);
    if (rc) return rc;
    ctx->tk.pend_h32 = h32;
    return DAE_OK;
}

int dae_score_topk_finish(dae_ctx* ctx, const float* tau, const int32_t* seed_row_ptr, const int32_t* seed_col,
                          int out_kind, float* out_score, int32_t* out_idx)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!tau || !out_score || !out_idx) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if ((seed_row_ptr == nullptr) != (seed_col == nullptr))
        return dae_fail(ctx, DAE_ERR_ARG, "seed_row_ptr and seed_col must both be given or both null");
    return topk_phase_b(ctx, tau, seed_row_ptr, seed_col, out_kind, out_score, out_idx, ctx->tk.pend_h32, nullptr, true);
}

}  // extern "C"

// dae_decode_mix_term (add = false) and dae_decode_mix_term_add: the same checks, tiles and launch geometry; the second runs the
// read-modify-write instances of the kernel (decode_generic.hip EPI_TERM_ADD)
static int decode_mix_term(dae_ctx* ctx, const float* h, int B, int H, int dtype, const float* row_scale, int n_cols,
                           float* outT, int64_t ldT, bool add)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!h || !row_scale || !outT) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (dtype != DAE_DTYPE_F32 && dtype != DAE_DTYPE_BF16) return dae_fail(ctx, DAE_ERR_ARG, "unknown dtype %d", dtype);
    const dae_packed* pk = packed_for(ctx, dtype, H);
    if (!pk) return DAE_ERR_STATE;
    if (ldT < B) return dae_fail(ctx, DAE_ERR_ARG, "ldT=%lld < %d rows", (long long)ldT, B);
    if (B <= 0) return DAE_OK;
    int n_loc = n_cols - pk->col_lo;                       // columns of the image below the global bound
    if (n_loc > pk->col_hi - pk->col_lo) n_loc = pk->col_hi - pk->col_lo;
    if (n_loc <= 0) return DAE_OK;
    const dae_rowgeom g = geom_for(dtype, B, pk->Hp);
    int rc = pack_hidden(ctx, dtype, h, B, H, g);
    if (rc) return rc;
    dae_tileset ts{(n_loc + 31) / 32, 1, 0, static_cast<const int*>(pk->ident.p)};
    return dae_launch_decode_scaled_T(ctx, g, B, ts, row_scale, outT, ldT, dtype, add);
}

extern "C" {

int dae_decode_mix_term(dae_ctx* ctx, const float* h, int B, int H, int dtype, const float* row_scale, int n_cols,
                        float* outT, int64_t ldT)
{
    return decode_mix_term(ctx, h, B, H, dtype, row_scale, n_cols, outT, ldT, false);
}

int dae_decode_mix_term_add(dae_ctx* ctx, const float* h, int B, int H, int dtype, const float* row_scale, int n_cols,
                            float* accT, int64_t ldT)
{
    return decode_mix_term(ctx, h, B, H, dtype, row_scale, n_cols, accT, ldT, true);
}

int dae_set_score_mix(dae_ctx* ctx, const float* mixT, int64_t ld, int n_cols, const float* w_title)
{
    if (!ctx) return DAE_ERR_ARG;
    if ((mixT == nullptr) != (w_title == nullptr)) return dae_fail(ctx, DAE_ERR_ARG, "mixT and w_title go together");
    ctx->mixT = mixT; ctx->mix_ld = ld; ctx->mix_w = w_title; ctx->mix_ncols = mixT ? n_cols : 0;
    return DAE_OK;
}

int dae_mix_topk_exact(dae_ctx* title_ctx, dae_ctx* dae_ctx_, const float* feat, int64_t ld_feat, const float* h, int64_t ld_h,
                       int B, const float* w_title, const float* w_playlist, int n_tracks, const int32_t* seed_row_ptr,
                       const int32_t* seed_col, int k, float* out_score, int32_t* out_idx, int32_t* guard_out)
{
    if (!title_ctx) return DAE_ERR_ARG;
    if (!dae_ctx_ || dae_ctx_ == title_ctx) return dae_fail(title_ctx, DAE_ERR_ARG, "dae_mix_topk_exact: needs the DAE's context");
    if (title_ctx->device != dae_ctx_->device) return dae_fail(title_ctx, DAE_ERR_ARG, "dae_mix_topk_exact: contexts on different devices");
    if (!feat || !h || !w_title || !w_playlist) return dae_fail(title_ctx, DAE_ERR_ARG, "null pointer");
    if (B < 0 || n_tracks <= 0) return dae_fail(title_ctx, DAE_ERR_ARG, "bad shape B=%d n_tracks=%d", B, n_tracks);
    int rc = dae_check_topk_args(title_ctx, DAE_DTYPE_BF16_EXACT, k, seed_row_ptr, seed_col, out_score, out_idx);
    if (rc) return rc;
    if (title_ctx->mixT) return dae_fail(title_ctx, DAE_ERR_STATE, "dae_mix_topk_exact takes the DAE's hidden rows itself: clear dae_set_score_mix");
    rc = dae_mix_topk_exact_impl(title_ctx, dae_ctx_, feat, ld_feat, h, ld_h, B, w_title, w_playlist, n_tracks, seed_row_ptr,
                                 seed_col, k, out_score, out_idx);
    if (rc) return rc;
    if (guard_out) {                                       // the guard words as they stand after this launch, in stream order
        rc = dae_ensure_guard(title_ctx);                  // (B == 0: nothing ran yet)
        if (rc) return rc;
        DAE_HIP_CHECK(title_ctx, hipMemcpyAsync(guard_out, title_ctx->guard.p, DAE_GUARD_BYTES, hipMemcpyDeviceToDevice, title_ctx->stream));
    }
    return DAE_OK;
}

}  // extern "C"

// dae_title_score in two halves (round 6): everything of a titled launch that does not depend on the lane's previous launch --
// title features, the feed -> CSR + seed lists, the DAE's hidden rows, the mixing weights -- and the ranking itself.
// dae_title_score runs them back to back on one stream; dae_pipeline runs the first half of launch n + 1 on its prep stream
// (contexts of its own) while the lane still ranks launch n.  What travels between the halves (dae_title_bufs), for the calls that
// run both themselves (dae_title_score, dae_title_score_catalogue), is carved out of one buffer of the title context:
int dae_title_bufs_reserve(dae_ctx* tc, int64_t nnz, int B, int H, int ld_feat, dae_title_bufs& b)
{
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t nz = (size_t)(nnz > 0 ? nnz : 1);
    const size_t o_rp = 0, o_col = o_rp + up((size_t)(B + 1) * 4), o_val = o_col + up(nz * 4), o_srp = o_val + up(nz * 4),
                 o_sc = o_srp + up((size_t)(B + 1) * 4), o_h = o_sc + up(nz * 4), o_ft = o_h + up((size_t)B * H * 4),
                 o_wt = o_ft + up((size_t)B * ld_feat * 4), o_wp = o_wt + up((size_t)B * 4), total = o_wp + up((size_t)B * 4);
    const int rc = dae_reserve(tc, tc->title_scratch, total);
    if (rc) return rc;
    char* base = static_cast<char*>(tc->title_scratch.p);
    b.rp = reinterpret_cast<int32_t*>(base + o_rp); b.col = reinterpret_cast<int32_t*>(base + o_col);
    b.val = reinterpret_cast<float*>(base + o_val); b.srp = reinterpret_cast<int32_t*>(base + o_srp);
    b.sc = reinterpret_cast<int32_t*>(base + o_sc); b.h = reinterpret_cast<float*>(base + o_h);
    b.feat = reinterpret_cast<float*>(base + o_ft); b.wt = reinterpret_cast<float*>(base + o_wt);
    b.wp = reinterpret_cast<float*>(base + o_wp);
    return DAE_OK;
}

int dae_title_prepare(dae_ctx* tc, dae_ctx* dc, const int64_t* positions, const float* values, int values_broadcast, int64_t nnz,
                      int B, int V, const float* W_enc, const float* b_enc, int H, const int32_t* titles, int L, const float* emb,
                      int n_char, int E, const float* conv_w, const float* conv_b, const int32_t* filter_sizes, int n_sizes, int F,
                      int ld_feat, const float* titles_use, int n_tracks, const dae_title_bufs& b, int32_t* csr_status)
{
    int rc = dae_title_features(tc, titles, B, L, emb, n_char, E, conv_w, conv_b, filter_sizes, n_sizes, F, 1.0f, 0u, b.feat, ld_feat,
                                nullptr, nullptr);
    if (rc) return rc;
    auto from_dc = [&](int r) { return r ? dae_fail(tc, r, "%s", dc->err.c_str()) : DAE_OK; };
    // the feed -> CSR AND the seed lists (the playlist's own tracks) from one group of four launches (round 6: csr.hip)
    rc = from_dc(dae_launch_coo64_to_csr_seeds(dc, positions, values, values_broadcast, nnz, B, V, b.rp, b.col, b.val, csr_status,
                                               n_tracks, b.srp, b.sc));
    if (rc) return rc;
    rc = from_dc(dae_encode(dc, b.rp, b.col, b.val, W_enc, b_enc, V, H, B, 1.0f, 1.0f, 0u, b.h));
    if (rc) return rc;
    return from_dc(dae_mix_weights(dc, b.rp, b.col, b.val, B, 1.0f, 0u, titles_use, b.wt, b.wp));
}

int dae_title_rank(dae_ctx* tc, dae_ctx* dc, int dtype, int B, int V, int H, int ld_feat, const dae_title_bufs& b, int n_tracks, int k,
                   float* out_score, int32_t* out_idx, int32_t* guard_out)
{
    if (dtype == DAE_DTYPE_BF16_EXACT)
        return dae_mix_topk_exact(tc, dc, b.feat, ld_feat, b.h, H, B, b.wt, b.wp, n_tracks, b.srp, b.sc, k, out_score, out_idx, guard_out);
    // fp32 / plain bf16: the fused mix of dae_set_score_mix -- the DAE term transposed, then the title context's threshold path
    // ranks sigmoid(z_title) * w_title + term (the operations and order of dae_mix_scores)
    auto from_dc = [&](int r) { return r ? dae_fail(tc, r, "%s", dc->err.c_str()) : DAE_OK; };
    const size_t nt32 = (size_t)((n_tracks + 31) / 32 * 32 < V ? (n_tracks + 31) / 32 * 32 : V);
    int rc = dae_reserve(tc, tc->title_y1, nt32 * (size_t)B * sizeof(float));
    if (rc) return rc;
    float* y1T = static_cast<float*>(tc->title_y1.p);
    rc = from_dc(dae_decode_mix_term(dc, b.h, B, H, dtype, b.wp, n_tracks, y1T, B));
    if (rc) return rc;
    rc = dae_set_score_mix(tc, y1T, B, (int)nt32, b.wt);
    if (rc) return rc;
    rc = dae_decode_topk(tc, b.feat, B, ld_feat, dtype, n_tracks, b.srp, b.sc, k, DAE_OUT_LOGIT, out_score, out_idx);
    (void)dae_set_score_mix(tc, nullptr, 0, 0, nullptr);
    if (rc) return rc;
    if (guard_out) DAE_HIP_CHECK(tc, hipMemsetAsync(guard_out, 0, DAE_GUARD_BYTES, tc->stream));      // (no bound to guard)
    return DAE_OK;
}

extern "C" {

// An ensemble's ranking half (include/dae_hip.h): the members' weighted sigmoids summed in the transposed
// term buffer of the ranking context -- member 0 writes it, the others add to it -- and the ranking context's threshold path on
// its own weighted sigmoid plus that buffer (dae_set_score_mix), cleared afterwards as dae_title_rank clears it.  Every refusal
// comes before the first launch.
int dae_ensemble_topk(dae_ctx* const* members, int M, const float* const* h, const int* H, const float* const* row_scale,
                      dae_ctx* title_ctx, const float* feat, int ld_feat, const float* w_title, int B, int dtype, int n_tracks,
                      const int32_t* seed_row_ptr, const int32_t* seed_col, int k, float* out_score, int32_t* out_idx)
{
    if (!members || M < 1 || !members[M - 1]) return dae_fail(title_ctx, DAE_ERR_ARG, "dae_ensemble_topk: needs M >= 1 member contexts");
    const bool titled = title_ctx != nullptr;
    dae_ctx* rc_ctx = titled ? title_ctx : members[M - 1];                 // the ranking context: it takes the messages too
    if (!h || !H || !row_scale || !out_score || !out_idx) return dae_fail(rc_ctx, DAE_ERR_ARG, "null pointer");
    if (titled ? (!feat || !w_title) : (feat || w_title))
        return dae_fail(rc_ctx, DAE_ERR_ARG, titled ? "null pointer (feat / w_title of the title context)"
                                                    : "dae_ensemble_topk: feat / w_title without a title context");
    if ((seed_row_ptr == nullptr) != (seed_col == nullptr))
        return dae_fail(rc_ctx, DAE_ERR_ARG, "seed_row_ptr and seed_col must both be given or both null");
    if (dtype == DAE_DTYPE_BF16_EXACT)
        return dae_fail(rc_ctx, DAE_ERR_ARG, "DAE_DTYPE_BF16_EXACT is not available with dae_ensemble_topk: rank with DAE_DTYPE_F32 (the same lists)");
    if (dtype != DAE_DTYPE_F32 && dtype != DAE_DTYPE_BF16) return dae_fail(rc_ctx, DAE_ERR_ARG, "unknown dtype %d", dtype);
    if (k < 1 || k > DAE_MAX_K) return dae_fail(rc_ctx, DAE_ERR_ARG, "k=%d out of [1,%d] (dae_ensemble_topk)", k, DAE_MAX_K);
    if (B < 0 || B > DAE_ROW_SLAB || n_tracks <= 0)
        return dae_fail(rc_ctx, DAE_ERR_ARG, "bad shape B=%d (at most %d rows a call) n_tracks=%d", B, DAE_ROW_SLAB, n_tracks);
    // every context: its rows and weights, one device and stream, no mix of its own, an image of `dtype` over the whole vocabulary
    // (ensemble.hip: the checks every ensemble call shares)
    int V = 0;
    int rc = dae_ensemble_check("dae_ensemble_topk", rc_ctx, members, M, h, H, row_scale, title_ctx, ld_feat, dtype, &V);
    if (rc) return rc;
    if (n_tracks > V) return dae_fail(rc_ctx, DAE_ERR_ARG, "n_tracks=%d exceeds the images' %d columns", n_tracks, V);
    if (B == 0) return DAE_OK;

    const size_t nt32 = (size_t)((n_tracks + 31) / 32 * 32 < V ? (n_tracks + 31) / 32 * 32 : V);
    rc = dae_reserve(rc_ctx, rc_ctx->title_y1, nt32 * (size_t)B * sizeof(float));
    if (rc) return rc;
    float* accT = static_cast<float*>(rc_ctx->title_y1.p);
    const int n_acc = titled ? M : M - 1;                  // members summed in the buffer (untitled: the last one ranks)
    if (n_acc == 0) {
        // one member alone: y = t_0.  The mix epilogue adds the buffer's element; -0.0f is the one value that leaves every t_0,
        // a zero of either sign included, as it is
        DAE_HIP_CHECK(rc_ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(accT), (int)0x80000000u, nt32 * (size_t)B, rc_ctx->stream));
    }
    for (int m = 0; m < n_acc; ++m) {
        dae_ctx* c = members[m];
        rc = decode_mix_term(c, h[m], B, H[m], dtype, row_scale[m], n_tracks, accT, B, m > 0);
        if (rc) return c == rc_ctx ? rc : dae_fail(rc_ctx, rc, "%s", c->err.c_str());
    }
    rc = dae_set_score_mix(rc_ctx, accT, B, (int)nt32, titled ? w_title : row_scale[M - 1]);
    if (rc) return rc;
    rc = dae_decode_topk(rc_ctx, titled ? feat : h[M - 1], B, titled ? ld_feat : H[M - 1], dtype, n_tracks, seed_row_ptr, seed_col, k,
                         DAE_OUT_LOGIT, out_score, out_idx);
    (void)dae_set_score_mix(rc_ctx, nullptr, 0, 0, nullptr);
    return rc;
}

int dae_title_score(dae_ctx* tc, dae_ctx* dc, int dtype, const int64_t* positions, const float* values, int values_broadcast,
                    int64_t nnz, int n_rows, int V, const float* W_enc, const float* b_enc, int H,
                    const int32_t* titles, int L, const float* emb, int n_char, int E, const float* conv_w,
                    const float* conv_b, const int32_t* filter_sizes, int n_sizes, int F, int ld_feat,
                    const float* titles_use, int n_tracks, int k, float* out_score, int32_t* out_idx,
                    int32_t* guard_out, int32_t* csr_status)
{
    if (!tc) return DAE_ERR_ARG;
    if (!dc || dc == tc) return dae_fail(tc, DAE_ERR_ARG, "dae_title_score: needs the DAE's context");
    if (!dae_known_dtype(dtype)) return dae_fail(tc, DAE_ERR_ARG, "unknown dtype %d", dtype);
    // (every dtype: the exact mix, and the fp32 / bf16 mix under dae_set_score_mix, keep DAE_MAX_K -- refused before any launch)
    if (k < 1 || k > DAE_MAX_K) return dae_fail(tc, DAE_ERR_ARG, "k=%d out of [1,%d] (titled scoring)", k, DAE_MAX_K);
    if (!titles || !titles_use || !W_enc || !b_enc || !csr_status || (nnz > 0 && (!positions || !values)))
        return dae_fail(tc, DAE_ERR_ARG, "null pointer");
    if (n_rows <= 0) return DAE_OK;
    if (nnz < 0 || nnz >= (int64_t)1 << 31 || V < 1 || H < 1 || ld_feat < n_sizes * F)
        return dae_fail(tc, DAE_ERR_ARG, "bad shape");
    if (dc->stream != tc->stream) return dae_fail(tc, DAE_ERR_STATE, "both contexts must be bound to the same stream");
    const int B = n_rows;
    dae_title_bufs b;
    int rc = dae_title_bufs_reserve(tc, nnz, B, H, ld_feat, b);
    if (rc) return rc;
    rc = dae_title_prepare(tc, dc, positions, values, values_broadcast, nnz, B, V, W_enc, b_enc, H, titles, L, emb, n_char, E, conv_w,
                           conv_b, filter_sizes, n_sizes, F, ld_feat, titles_use, n_tracks, b, csr_status);
    if (rc) return rc;
    return dae_title_rank(tc, dc, dtype, B, V, H, ld_feat, b, n_tracks, k, out_score, out_idx, guard_out);
}

int dae_title_score_exact(dae_ctx* tc, dae_ctx* dc, const int64_t* positions, const float* values, int values_broadcast,
                          int64_t nnz, int n_rows, int V, const float* W_enc, const float* b_enc, int H,
                          const int32_t* titles, int L, const float* emb, int n_char, int E, const float* conv_w,
                          const float* conv_b, const int32_t* filter_sizes, int n_sizes, int F, int ld_feat,
                          const float* titles_use, int n_tracks, int k, float* out_score, int32_t* out_idx,
                          int32_t* guard_out, int32_t* csr_status)
{
    return dae_title_score(tc, dc, DAE_DTYPE_BF16_EXACT, positions, values, values_broadcast, nnz, n_rows, V, W_enc, b_enc, H, titles,
                           L, emb, n_char, E, conv_w, conv_b, filter_sizes, n_sizes, F, ld_feat, titles_use, n_tracks, k, out_score,
                           out_idx, guard_out, csr_status);
}

}  // extern "C"
