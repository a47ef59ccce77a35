// loss_rows.hip -- the loss without a step: the cost of a batch and the loss of each of its rows, with
// no gradient, no dz^T and no logits in memory.  Three launches behind dae_decode_loss_rows / dae_score_loss:
//
//   1. decode_f32_kernel's EPI_ROWLOSS (decode_generic.hip) over the context's prepacked image: every element of the B x V
//      logits taken as a negative, summed per row inside each workgroup -> the partial table [n_rg][nb_rg][R_TILE];
//   2. loss_rows_finish_kernel, one workgroup per row: the row's targets redone from their own dot products (THE positives'
//      chain of train_common.h, as loss_fixup_kernel of the step), each adding L(y) - L(0); the row's partials summed in double
//      in ascending order of the workgroup's place -> row_loss[row];
//   3. loss_cost_kernel, one wave: cost = sum of the rows / n_batch + lambda * l2 (l2: train.hip's l2_partial_kernel).
//
// Every sum runs in an order fixed by indices alone (no atomics): the same inputs give the same bits, call after call.
// The calls write their outputs and ctx->loss_rows (and the packed hidden image, which every decode call rewrites) -- never a
// parameter, an Adam moment, the armed-Adam state or a prepacked image.
#include "train_common.h"

namespace {

constexpr int LR_MAXH = 1024;
constexpr int LR_MAX_B = 4096;

template <bool BF16>
__global__ __launch_bounds__(256) void loss_rows_finish_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                               const float* __restrict__ val, int H, int V,
                                                               const float* __restrict__ h,       // [B, H]
                                                               const float* __restrict__ Wd,      // [V, H] row-major
                                                               const float* __restrict__ bias,    // [V]
                                                               const float* __restrict__ part,    // [n_rg][nb_rg][R_TILE]
                                                               int nb_rg, int R_TILE, float* __restrict__ row_loss)
{
    __shared__ float4 sh[LR_MAXH / 4];
    __shared__ float wsum[4];
    __shared__ float negp[256];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int H4 = H >> 2;
    for (int i = tid; i < H4; i += 256) {
        float4 v = reinterpret_cast<const float4*>(h + (size_t)row * H)[i];
        if (BF16) v = make_float4(dae_bf16_value(v.x), dae_bf16_value(v.y), dae_bf16_value(v.z), dae_bf16_value(v.w));
        sh[i] = v;
    }
    // the row's negative partials, one per workgroup of its row group (nb_rg <= DAE_NUM_CU = 256 of them)
    const int rg = row / R_TILE, rloc = row % R_TILE;
    if (tid < nb_rg) negp[tid] = part[((size_t)rg * nb_rg + tid) * R_TILE + rloc];
    __syncthreads();
    // thread t takes the entries t, t + 256, ... of the row, in that order (a row may hold any number)
    float corr = 0.0f;
    const int beg = row_ptr[row], end = row_ptr[row + 1];
    for (int i = beg + tid; i < end; i += 256) {
        const int c = col[i];
        if (c < 0 || c >= V) continue;                              // (the caller's error: never read past the matrix)
        const float z = dae_positive_logit<BF16>(reinterpret_cast<const float4*>(Wd + (size_t)c * H), sh, H4, bias + c);
        dae_loss_pos_corr(dae_train_sigmoid(z), val[i], corr);
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

// cost = (float)(sum_r (double)row_loss[r] / n_batch + lambda * l2): one wave, lane-strided sums, then a shuffle tree
__global__ __launch_bounds__(64) void loss_cost_kernel(const float* __restrict__ row_loss, int B, int n_batch,
                                                       const double* __restrict__ l2_part, int n_l2, float lambda,
                                                       float* __restrict__ cost)
{
    const int lane = threadIdx.x;
    double s = 0.0, l2 = 0.0;
    for (int i = lane; i < B; i += 64) s += (double)row_loss[i];
    for (int i = lane; i < n_l2; i += 64) l2 += l2_part[i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { s += __shfl_xor(s, d); l2 += __shfl_xor(l2, d); }
    if (lane == 0) *cost = (float)(s / (double)n_batch + (double)lambda * l2);
}

// what one call keeps in ctx->loss_rows, sized by its own shape
struct LossPlan {
    dae_rowgeom g;
    float *hbuf, *part, *rows;
    double* l2_part;
};

// want_h: the call encodes into hbuf (dae_score_loss); want_rows: the caller gave no row_loss; want_l2: lambda != 0
int loss_plan(dae_ctx* ctx, const dae_packed& pk, int dtype, int B, int H, bool want_h, bool want_rows, bool want_l2, LossPlan& t)
{
    t.g = dtype == DAE_DTYPE_F32 ? dae_row_geometry(B, pk.Hp) : dae_row_geometry_bf16(B, pk.Hp);
    const size_t h_floats = want_h ? (size_t)B * H : 0;
    const size_t part_floats = (size_t)t.g.grid * t.g.R_TILE;
    const size_t row_floats = want_rows ? (size_t)B : 0;
    const size_t floats = (h_floats + part_floats + row_floats + 15) / 16 * 16;      // (hbuf first: 16-byte aligned rows; l2 behind: 64-byte aligned)
    const int rc = dae_reserve(ctx, ctx->loss_rows, floats * sizeof(float) + (want_l2 ? 4096 * sizeof(double) : 0));
    if (rc) return rc;
    t.hbuf = static_cast<float*>(ctx->loss_rows.p);
    t.part = t.hbuf + h_floats;
    t.rows = t.part + part_floats;
    t.l2_part = reinterpret_cast<double*>(t.hbuf + floats);
    return DAE_OK;
}

// the image of `dtype` the call runs over: a plain one (no catalogue's) of all V columns
int loss_image(dae_ctx* ctx, int dtype, int V, int H, const dae_packed** out)
{
    const dae_packed& pk = dtype == DAE_DTYPE_F32 ? ctx->pk_f32 : ctx->pk_bf16;
    if (!pk.valid || pk.cat_id != 0 || pk.col_lo != 0 || pk.col_hi != V)
        return dae_fail(ctx, DAE_ERR_STATE, "no prepacked image of dtype %d over columns [0, %d) (dae_prepack_decoder)", dtype, V);
    if (pk.H != H) return dae_fail(ctx, DAE_ERR_ARG, "H=%d does not match prepacked H=%d", H, pk.H);
    *out = &pk;
    return DAE_OK;
}

int loss_check_shape(dae_ctx* ctx, const char* fn, int B, int H, int V)
{
    if (B < 1 || B > LR_MAX_B) return dae_fail(ctx, DAE_ERR_ARG, "%s: B=%d outside [1, %d]", fn, B, LR_MAX_B);
    if (H <= 0 || (H % 32) != 0 || H > LR_MAXH) return dae_fail(ctx, DAE_ERR_ARG, "%s: needs H %% 32 == 0 and H <= %d (H=%d)", fn, LR_MAXH, H);
    if (V <= 0) return dae_fail(ctx, DAE_ERR_ARG, "%s: V=%d", fn, V);
    return DAE_OK;
}

// launches 1 and 2 on the hidden rows h [B][H]: row_loss[B]
int loss_rows_launch(dae_ctx* ctx, const LossPlan& t, const float* h, int B, int H, int dtype, const int32_t* y_row_ptr,
                     const int32_t* y_col, const float* y_val, const float* W_dec, const float* b_dec, int V, float* row_loss)
{
    int rc;
    if (dtype == DAE_DTYPE_F32) {
        if ((rc = dae_launch_pack_h(ctx, h, B, H, t.g))) return rc;          // (rewrites the whole image, pads included)
        dae_note_hidden_repacked(ctx, B, H, t.g.R_TILE);
    } else {
        if ((rc = dae_launch_pack_h_bf16(ctx, h, B, H, t.g))) return rc;
        ctx->tk.valid = false;                                               // (a pending dae_score_topk_begin's hidden image is gone)
    }
    if ((rc = dae_launch_decode_rowloss(ctx, t.g, B, dtype, t.part))) return rc;
    auto finish = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(B), dim3(256), 0, ctx->stream, y_row_ptr, y_col, y_val, H, V, h, W_dec, b_dec, t.part,
                           t.g.nb_rg, t.g.R_TILE, row_loss);
    };
    if (dtype == DAE_DTYPE_BF16) finish(&loss_rows_finish_kernel<true>);
    else finish(&loss_rows_finish_kernel<false>);
    DAE_CHECK_LAUNCH(ctx, "loss_rows_finish_kernel");
    return DAE_OK;
}

}  // namespace

int dae_launch_loss_cost(dae_ctx* ctx, const float* row_loss, int B, int n_batch, const double* l2_part, int n_l2, float lambda,
                         float* cost_out)
{
    hipLaunchKernelGGL(loss_cost_kernel, dim3(1), dim3(64), 0, ctx->stream, row_loss, B, n_batch, l2_part, n_l2, lambda, cost_out);
    DAE_CHECK_LAUNCH(ctx, "loss_cost_kernel");
    return DAE_OK;
}

extern "C" {

int dae_decode_loss_rows(dae_ctx* ctx, const float* h, int B, int H, int dtype, const int32_t* y_row_ptr, const int32_t* y_col,
                         const float* y_val, const float* W_dec, const float* b_dec, int V, float* row_loss)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!h || !y_row_ptr || !W_dec || !b_dec || !row_loss) return dae_fail(ctx, DAE_ERR_ARG, "dae_decode_loss_rows: null pointer");
    if (dtype != DAE_DTYPE_F32 && dtype != DAE_DTYPE_BF16) return dae_fail(ctx, DAE_ERR_ARG, "dae_decode_loss_rows: unknown dtype %d", dtype);
    int rc = loss_check_shape(ctx, "dae_decode_loss_rows", B, H, V);
    if (rc) return rc;
    if ((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(W_dec)) % 16)
        return dae_fail(ctx, DAE_ERR_ARG, "dae_decode_loss_rows: h and W_dec must be 16-byte aligned");
    const dae_packed* pk = nullptr;
    if ((rc = loss_image(ctx, dtype, V, H, &pk))) return rc;
    LossPlan t;
    if ((rc = loss_plan(ctx, *pk, dtype, B, H, false, false, false, t))) return rc;
    return loss_rows_launch(ctx, t, h, B, H, dtype, y_row_ptr, y_col, y_val, W_dec, b_dec, V, row_loss);
}

int dae_score_loss(dae_ctx* ctx, const int32_t* x_row_ptr, const int32_t* x_col, const float* x_val, const int32_t* y_row_ptr,
                   const int32_t* y_col, const float* y_val, const float* W_enc, const float* b_enc, const float* W_dec,
                   const float* b_dec, int V, int H, int B, int n_batch, int tied, float ikp, float kp, uint32_t seed,
                   float reg_lambda, float* row_loss, float* cost_out)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!row_loss && !cost_out) return dae_fail(ctx, DAE_ERR_ARG, "dae_score_loss: both outputs are null");
    if (!x_row_ptr || !y_row_ptr || !W_enc || !b_enc || !b_dec || (!tied && !W_dec))
        return dae_fail(ctx, DAE_ERR_ARG, "dae_score_loss: null pointer");
    int rc = loss_check_shape(ctx, "dae_score_loss", B, H, V);
    if (rc) return rc;
    if (n_batch <= 0) return dae_fail(ctx, DAE_ERR_ARG, "dae_score_loss: n_batch=%d", n_batch);
    if (!(ikp > 0.f && ikp <= 1.f) || !(kp > 0.f && kp <= 1.f))
        return dae_fail(ctx, DAE_ERR_ARG, "dae_score_loss: keep probabilities must be in (0,1]");
    const float* Wd = tied ? W_enc : W_dec;
    if ((reinterpret_cast<uintptr_t>(W_enc) | reinterpret_cast<uintptr_t>(b_enc) | reinterpret_cast<uintptr_t>(Wd)) % 16)
        return dae_fail(ctx, DAE_ERR_ARG, "dae_score_loss: W_enc, b_enc, W_dec must be 16-byte aligned");
    const int dtype = ctx->train_dtype;
    const dae_packed* pk = nullptr;
    if ((rc = loss_image(ctx, dtype, V, H, &pk))) return rc;
    LossPlan t;
    if ((rc = loss_plan(ctx, *pk, dtype, B, H, true, !row_loss, reg_lambda != 0.0f && cost_out, t))) return rc;
    // the step's encode: the same dropout streams for the same seed (encode.hip; masks keyed by the row's index in the batch)
    if ((rc = dae_launch_encode(ctx, x_row_ptr, x_col, x_val, W_enc, b_enc, V, H, B, ikp, kp, seed, t.hbuf, nullptr, 0, 0))) return rc;
    float* const rows = row_loss ? row_loss : t.rows;
    if ((rc = loss_rows_launch(ctx, t, t.hbuf, B, H, dtype, y_row_ptr, y_col, y_val, Wd, b_dec, V, rows))) return rc;
    if (!cost_out) return DAE_OK;
    int n_l2 = 0;
    if (reg_lambda != 0.0f) {
        // the tensors the step counts: W_enc, b_dec, b_enc, and W_dec unless tied
        const float* ts[4] = {W_enc, b_dec, b_enc, tied ? nullptr : W_dec};
        const size_t ns[4] = {(size_t)V * H, (size_t)V, (size_t)H, (size_t)V * H};
        if ((rc = dae_launch_l2_partials(ctx, ts, ns, 4, t.l2_part, &n_l2))) return rc;
    }
    return dae_launch_loss_cost(ctx, rows, B, n_batch, t.l2_part, n_l2, reg_lambda, cost_out);
}

}  // extern "C"
