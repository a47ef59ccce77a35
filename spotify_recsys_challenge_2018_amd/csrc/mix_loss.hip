// mix_loss.hip -- the loss of the title scorer's MIXED score without a step: the cost of a batch and the
// loss of each of its rows under
//   yp = sigmoid(z_title) * w_title + sigmoid(z_dae) * w_playlist,   L = -sum_v [y ln(yp + 1e-10) + 0.55 (1 - y) ln(1 - yp + 1e-10)]
// (reference DAEs.py:176-196), with no gradient, no [B, V] matrix of either scorer, no dense target matrix and no dz^T.
// dae_mix_loss_rows walks panels of at most 256 rows (mix_loss_plan.h); per panel, on the stream both contexts share:
//
//   1. dae_decode_mix_term on the DAE's context over ALL V columns: w_playlist[r] * sigmoid(z_dae[r][c]), transposed, into the
//      panel's term buffer;
//   2. decode_f32_kernel's EPI_MIXROWLOSS (decode_generic.hip) over the title scorer's prepacked fp32 image: every element of the
//      panel's mixed scores taken as a negative in the title step's operations (title.hip title_loss_kernel), summed per row
//      inside each workgroup -> the partial table [n_rg][nb_rg][R_TILE];
//   3. mix_loss_finish_kernel, one workgroup per row: the row's targets redone from their own two chains (the positives' chain of
//      train_common.h over Output_W^T and over W_dec -- in fp32 the bits the GEMMs saw for that element), each adding
//      L(y) - L(0); the row's partials summed in double in ascending order of the workgroup's place -> row_loss[row].
//
// Behind the last panel one loss_cost_kernel launch (loss_rows.hip): cost = sum of the rows / n_batch; the title cost has no
// lambda term.  Every sum runs in an order fixed by indices alone (no atomics): the same inputs give the same bits, call after
// call.  The call writes its outputs, ctx->mix_loss and the two packed hidden images -- never a parameter, an Adam moment, the
// title trainer's state, a prepacked image or what dae_set_score_mix left in either context.
#include "mix_loss_plan.h"
#include "train_common.h"

namespace {

__global__ __launch_bounds__(256) void mix_loss_finish_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                              const float* __restrict__ val, int V,
                                                              const float* __restrict__ h, int H,           // [nb, H]
                                                              const float* __restrict__ Wd,                 // [V, H] row-major
                                                              const float* __restrict__ bd,                 // [V]
                                                              const float* __restrict__ feat, int64_t ld_feat,   // [nb, ld_feat]
                                                              const float* __restrict__ WT,                 // Output_W^T [V, ld_feat]
                                                              const float* __restrict__ bT,                 // Output_b [V]
                                                              const float* __restrict__ w_title, const float* __restrict__ w_playlist,
                                                              const float* __restrict__ part,               // [n_rg][nb_rg][R_TILE]
                                                              int nb_rg, int R_TILE, float* __restrict__ row_loss)
{
    __shared__ float4 sh[DAE_MIXLOSS_MAXH / 4];
    __shared__ float4 sf[DAE_MIXLOSS_MAXH / 4];
    __shared__ float wsum[4];
    __shared__ float negp[256];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int H4 = H >> 2, F4 = (int)(ld_feat >> 2);
    for (int i = tid; i < H4; i += 256) sh[i] = reinterpret_cast<const float4*>(h + (size_t)row * H)[i];
    for (int i = tid; i < F4; i += 256) sf[i] = reinterpret_cast<const float4*>(feat + (size_t)row * ld_feat)[i];
    // the row's negative partials, one per workgroup of its row group (nb_rg <= DAE_NUM_CU = 256 of them)
    const int rg = row / R_TILE, rloc = row % R_TILE;
    if (tid < nb_rg) negp[tid] = part[((size_t)rg * nb_rg + tid) * R_TILE + rloc];
    __syncthreads();
    const float wt = w_title[row], wp = w_playlist[row];
    // thread t takes the entries t, t + 256, ... of the row, in that order (a row may hold any number)
    float corr = 0.0f;
    const int beg = row_ptr[row], end = row_ptr[row + 1];
    for (int i = beg + tid; i < end; i += 256) {
        const int c = col[i];
        if (c < 0 || c >= V) continue;                              // (the caller's error: never read past the matrices)
        const float zt = dae_positive_logit<false>(reinterpret_cast<const float4*>(WT + (size_t)c * ld_feat), sf, F4, bT + c);
        const float zd = dae_positive_logit<false>(reinterpret_cast<const float4*>(Wd + (size_t)c * H), sh, H4, bd + c);
        // the element as the two launches in front saw it: the term dae_decode_mix_term stored, the GEMM epilogue's yp
        const float pd = dae_sigmoidf(zd) * wp;
        const float yp = dae_title_step_sigmoid(zt) * wt + pd;
        dae_loss_pos_corr_mixed(yp, val[i], corr);
    }
    // fixed order: lanes (shuffle tree), then the four waves in wave order
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) corr += __shfl_xor(corr, d);
    if ((tid & 63) == 0) wsum[tid >> 6] = corr;
    __syncthreads();
    if (tid == 0) {
        double neg = 0.0;
        for (int b = 0; b < nb_rg; ++b) neg += (double)negp[b];
        const double pos = (double)(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
        row_loss[row] = (float)(neg + pos);
    }
}

// a plain fp32 image (no catalogue's) of all V columns with K = H
int mix_loss_image(dae_ctx* ctx, const dae_packed& pk, int V, int H, const char* whose)
{
    if (!pk.valid || pk.cat_id != 0 || pk.col_lo != 0 || pk.col_hi != V)
        return dae_fail(ctx, DAE_ERR_STATE, "dae_mix_loss_rows: no prepacked fp32 image over columns [0, %d) on %s (dae_prepack_decoder)", V, whose);
    if (pk.H != H) return dae_fail(ctx, DAE_ERR_ARG, "dae_mix_loss_rows: %d does not match the prepacked H=%d of %s", H, pk.H, whose);
    return DAE_OK;
}

}  // namespace

extern "C" {

int dae_mix_loss_rows(dae_ctx* title_ctx, dae_ctx* dae, const float* h, int64_t ld_h, int H, const float* W_dec,
                      const float* b_dec, const float* feat, int64_t ld_feat, const float* OutW_T, const float* Out_b,
                      const float* w_title, const float* w_playlist, int B, int V, int n_batch,
                      const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val, float* row_loss, float* cost_out)
{
    static const char* fn = "dae_mix_loss_rows";
    dae_ctx* ctx = title_ctx;
    if (!ctx) return DAE_ERR_ARG;
    if (!dae || dae == ctx) return dae_fail(ctx, DAE_ERR_ARG, "%s: needs the DAE's context", fn);
    if (!row_loss && !cost_out) return dae_fail(ctx, DAE_ERR_ARG, "%s: both outputs are null", fn);
    if (!h || !W_dec || !b_dec || !feat || !OutW_T || !Out_b || !w_title || !w_playlist || !y_row_ptr)
        return dae_fail(ctx, DAE_ERR_ARG, "%s: null pointer", fn);
    if (ctx->device != dae->device) return dae_fail(ctx, DAE_ERR_ARG, "%s: contexts on different devices", fn);
    if (ctx->stream != dae->stream) return dae_fail(ctx, DAE_ERR_STATE, "%s: both contexts must be bound to the same stream", fn);
    if (B < 1 || B > DAE_MIXLOSS_MAX_B) return dae_fail(ctx, DAE_ERR_ARG, "%s: B=%d outside [1, %d]", fn, B, DAE_MIXLOSS_MAX_B);
    if (H <= 0 || (H % 32) != 0 || H > DAE_MIXLOSS_MAXH)
        return dae_fail(ctx, DAE_ERR_ARG, "%s: needs H %% 32 == 0 and H <= %d (H=%d)", fn, DAE_MIXLOSS_MAXH, H);
    if (ld_h != H) return dae_fail(ctx, DAE_ERR_ARG, "%s: ld_h=%lld: contiguous hidden rows (ld_h == H = %d) are required", fn, (long long)ld_h, H);
    if (ld_feat <= 0 || (ld_feat % 4) != 0 || ld_feat > DAE_MIXLOSS_MAXH)
        return dae_fail(ctx, DAE_ERR_ARG, "%s: ld_feat=%lld must be a multiple of 4 in [4, %d]", fn, (long long)ld_feat, DAE_MIXLOSS_MAXH);
    if (V <= 0) return dae_fail(ctx, DAE_ERR_ARG, "%s: V=%d", fn, V);
    if (n_batch <= 0) return dae_fail(ctx, DAE_ERR_ARG, "%s: n_batch=%d", fn, n_batch);
    if ((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(W_dec) | reinterpret_cast<uintptr_t>(feat) |
         reinterpret_cast<uintptr_t>(OutW_T)) % 16)
        return dae_fail(ctx, DAE_ERR_ARG, "%s: h, W_dec, feat and Output_W^T must be 16-byte aligned", fn);
    int rc = mix_loss_image(ctx, ctx->pk_f32, V, (int)ld_feat, "the title context");
    if (rc) return rc;
    if ((rc = mix_loss_image(ctx, dae->pk_f32, V, H, "the DAE's context"))) return rc;

    const int Hp = ctx->pk_f32.Hp;
    const dae_mixloss_plan pl = dae_plan_mix_loss(B, V, Hp, !row_loss);
    if (pl.total == 0) return dae_fail(ctx, DAE_ERR_ARG, "%s: no plan for B=%d V=%d Hp=%d", fn, B, V, Hp);
    if ((rc = dae_reserve(ctx, ctx->mix_loss, pl.total))) return rc;        // (grows only: reserved once at the largest panel seen)
    char* base = static_cast<char*>(ctx->mix_loss.p);
    float* term = reinterpret_cast<float*>(base + pl.o_term);
    float* part = reinterpret_cast<float*>(base + pl.o_part);
    float* const rows = row_loss ? row_loss : reinterpret_cast<float*>(base + pl.o_rows);

    for (int i = 0; i < pl.n_panels; ++i) {
        int r0, nb;
        dae_mixloss_panel(B, i, &r0, &nb);
        const dae_rowgeom g = dae_mixloss_geometry(nb, Hp);
        const float* hp_ = h + (size_t)r0 * H;
        const float* fp_ = feat + (size_t)r0 * ld_feat;
        // 1. the DAE's term of every column, transposed [V][nb]
        rc = dae_decode_mix_term(dae, hp_, nb, H, DAE_DTYPE_F32, w_playlist + r0, V, term, nb);
        if (rc) return dae_fail(ctx, rc, "%s", dae->err.c_str());
        // 2. the title GEMM over its image, the negatives per row
        if ((rc = dae_launch_pack_h(ctx, fp_, nb, (int)ld_feat, g))) return rc;      // (rewrites the whole image, pads included)
        dae_note_hidden_repacked(ctx, nb, (int)ld_feat, g.R_TILE);
        if ((rc = dae_launch_decode_mixrowloss(ctx, g, nb, term, nb, w_title + r0, part))) return rc;
        // 3. the targets and the row sums
        hipLaunchKernelGGL(mix_loss_finish_kernel, dim3(nb), dim3(256), 0, ctx->stream, y_row_ptr + r0, y_col, y_val, V, hp_, H, W_dec,
                           b_dec, fp_, ld_feat, OutW_T, Out_b, w_title + r0, w_playlist + r0, part, g.nb_rg, g.R_TILE, rows + r0);
        DAE_CHECK_LAUNCH(ctx, "mix_loss_finish_kernel");
    }
    if (!cost_out) return DAE_OK;
    return dae_launch_loss_cost(ctx, rows, B, n_batch, nullptr, 0, 0.0f, cost_out);
}

}  // extern "C"
