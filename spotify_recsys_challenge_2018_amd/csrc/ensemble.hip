// ensemble.hip -- the ensemble's canonical value at CALLER-GIVEN (row, column) pairs (include/dae_hip.h "ensembles"; DESIGN.md
// section 4e "Ranks under the ensemble"), and the checks every ensemble call makes of its scorers.
//
//     t_m[r, c] = sigmoid(z_m[r, c]) * a_m[r]
//     acc = t_0;  acc = acc + t_m  for m = 1 .. M-2                 (untitled: the last member is not in acc)
//     untitled:  y = t_{M-1} + acc                                  (M = 1: y = t_0)
//     titled:    acc also takes t_{M-1};  y = sigmoid(z_title) * w_title[r] + acc
//
// PER SCORER the candidate chain of candidates.hip (dae_decode_candidates, DAE_OUT_SCORE) writes the canonical sigmoid of every
// listed pair into an array of its own; ensemble_combine_kernel, a workgroup per row of the candidate CSR, then performs the
// products and sums above on those arrays, each one __fmul_rn / __fadd_rn: the operations and operands of the mix epilogues
// (decode_generic.hip, rank_of.hip), so a pair's value here IS the value the ranking calls list it by.
#include "dae_internal.h"
#include "ensemble_rank_of_plan.h"

namespace {

constexpr int EC_MAX_INLINE = 8;       // scorers whose weight pointers travel in the kernel's arguments

struct CombP {
    const float* s; size_t s_stride;               // [K][s_stride] canonical sigmoids, members first, the title scorer last
    const float* a[EC_MAX_INLINE];                 // a_m [B] of members m0 .. m0 + n_m - 1
    int m0, n_m, M;                                // this launch's members; all members
    const float* w_title;                          // null: untitled
    const int32_t* row_ptr; const int32_t* col; int n_cand, V;
    float* out;                                    // y; between the launches of a call with M > EC_MAX_INLINE: acc so far
};

// One launch takes up to EC_MAX_INLINE members in order; a call with more members takes several, the running acc kept in out[]
// (the same roundings in the same order: acc is an fp32 value either way).  The LAST launch finishes y and the ids' values.
__global__ __launch_bounds__(256) void ensemble_combine_kernel(const CombP p)
{
    const int row = blockIdx.x;
    const int a0 = p.row_ptr[row], b0 = p.row_ptr[row + 1];
    const int beg = a0 > 0 ? a0 : 0;
    const int end = b0 < p.n_cand ? b0 : p.n_cand;            // nothing is read or written at or past the caller's n_cand
    if (end <= beg) return;
    const bool titled = p.w_title != nullptr;
    const bool last_launch = p.m0 + p.n_m == p.M;
    const int n_acc = titled ? p.M : p.M - 1;                 // members summed in acc
    float w[EC_MAX_INLINE];
#pragma unroll
    for (int i = 0; i < EC_MAX_INLINE; ++i) w[i] = i < p.n_m ? p.a[i][row] : 0.0f;
    const float wt = titled ? p.w_title[row] : 0.0f;
    for (int e = beg + threadIdx.x; e < end; e += 256) {
        const int c = p.col[e];
        if (c < 0 || c >= p.V) {                              // -1: padding; any other id: the chains flagged it already
            if (last_launch) p.out[e] = c == -1 ? -__builtin_inff() : __builtin_nanf("");
            continue;
        }
        float acc = p.m0 > 0 ? p.out[e] : 0.0f;
        float y = acc;
#pragma unroll
        for (int i = 0; i < EC_MAX_INLINE; ++i) {
            if (i >= p.n_m) break;
            const int m = p.m0 + i;
            const float t = __fmul_rn(p.s[(size_t)m * p.s_stride + e], w[i]);
            if (m >= n_acc) y = m == 0 ? t : __fadd_rn(t, acc);                  // untitled, the last member: y = t_{M-1} + acc
            else acc = m == 0 ? t : __fadd_rn(acc, t);
        }
        if (titled && last_launch) y = __fadd_rn(__fmul_rn(p.s[(size_t)p.M * p.s_stride + e], wt), acc);
        p.out[e] = (last_launch) ? y : acc;
    }
}

}  // namespace

int dae_ensemble_check(const char* fn, dae_ctx* rc_ctx, dae_ctx* const* members, int M, const float* const* h, const int* H,
                       const float* const* row_scale, dae_ctx* title_ctx, int ld_feat, int dtype, int* V_out)
{
    const bool titled = title_ctx != nullptr;
    const int n_ctx = M + (titled ? 1 : 0);
    auto ctx_at = [&](int i) { return i < M ? members[i] : title_ctx; };
    char who[32];
    int V = 0;
    for (int i = 0; i < n_ctx; ++i) {
        dae_ctx* c = ctx_at(i);
        if (i < M) snprintf(who, sizeof(who), "member %d", i); else snprintf(who, sizeof(who), "the title context");
        if (!c) return dae_fail(rc_ctx, DAE_ERR_ARG, "%s: %s is a null context", fn, who);
        if (i < M && (!h[i] || !row_scale[i])) return dae_fail(rc_ctx, DAE_ERR_ARG, "null pointer (hidden rows / row_scale of %s)", who);
        for (int o = 0; o < i; ++o)
            if (ctx_at(o) == c) return dae_fail(rc_ctx, DAE_ERR_ARG, "%s: %s is listed twice (every scorer needs a context of its own)", fn, who);
        if (c->device != rc_ctx->device) return dae_fail(rc_ctx, DAE_ERR_ARG, "%s: %s is on another device", fn, who);
        if (c->stream != rc_ctx->stream) return dae_fail(rc_ctx, DAE_ERR_STATE, "%s: %s is bound to another stream", fn, who);
        if (c->mixT) return dae_fail(rc_ctx, DAE_ERR_STATE, "%s sets the mix itself: clear dae_set_score_mix on %s", fn, who);
        if (dtype < 0) continue;                              // (the candidate call reads the row-major tensors: no image)
        const dae_packed& pk = dtype == DAE_DTYPE_F32 ? c->pk_f32 : c->pk_bf16;
        const int Hi = i < M ? H[i] : ld_feat;
        if (!pk.valid) return dae_fail(rc_ctx, DAE_ERR_STATE, "%s: %s holds no image prepacked for dtype %d", fn, who, dtype);
        if (pk.cat_id != 0) return dae_fail(rc_ctx, DAE_ERR_STATE, "%s: %s holds a catalogue image", fn, who);
        if (pk.col_lo != 0 || pk.col_hi != pk.V)
            return dae_fail(rc_ctx, DAE_ERR_STATE, "%s: %s holds a shard image (columns [%d, %d) of %d)", fn, who, pk.col_lo, pk.col_hi, pk.V);
        if (pk.H != Hi) return dae_fail(rc_ctx, DAE_ERR_ARG, "H=%d of %s does not match its prepacked H=%d", Hi, who, pk.H);
        if (i == 0) V = pk.V;
        if (pk.V != V) return dae_fail(rc_ctx, DAE_ERR_ARG, "%s: %s holds %d columns, member 0 holds %d", fn, who, pk.V, V);
    }
    *V_out = V;
    return DAE_OK;
}

int dae_launch_ensemble_candidates(dae_ctx* rc_ctx, const dae_ens_tensors& t, int B, int V, const int32_t* row_ptr, const int32_t* col,
                                   int n_cand, float* s, size_t s_stride, float* out, int32_t* status)
{
    const bool titled = t.feat != nullptr;
    // the chains: one array of canonical sigmoids per scorer.  An id outside [0, V) is flagged once, by the first of them
    for (int m = 0; m < t.M; ++m) {
        const int rc = dae_decode_candidates(rc_ctx, t.h[m], t.H[m], B, t.H[m], t.W_dec[m], t.b_dec[m], V, row_ptr, col, n_cand,
                                             DAE_OUT_SCORE, s + (size_t)m * s_stride, m == 0 ? status : nullptr);
        if (rc) return rc;
    }
    if (titled) {
        const int rc = dae_decode_candidates(rc_ctx, t.feat, t.ld_feat, B, t.ld_feat, t.OutW_T, t.Out_b, V, row_ptr, col, n_cand,
                                             DAE_OUT_SCORE, s + (size_t)t.M * s_stride, nullptr);
        if (rc) return rc;
    }
    for (int m0 = 0; m0 < t.M; m0 += EC_MAX_INLINE) {
        CombP p{};
        p.s = s; p.s_stride = s_stride;
        p.m0 = m0; p.n_m = t.M - m0 < EC_MAX_INLINE ? t.M - m0 : EC_MAX_INLINE; p.M = t.M;
        for (int i = 0; i < p.n_m; ++i) p.a[i] = t.row_scale[m0 + i];
        p.w_title = titled ? t.w_title : nullptr;
        p.row_ptr = row_ptr; p.col = col; p.n_cand = n_cand; p.V = V;
        p.out = out;
        hipLaunchKernelGGL(ensemble_combine_kernel, dim3(B), dim3(256), 0, rc_ctx->stream, p);
        DAE_CHECK_LAUNCH(rc_ctx, "ensemble_combine_kernel");
    }
    return DAE_OK;
}

extern "C" {

int dae_ensemble_candidates(dae_ctx* const* members, int M, const float* const* h, const int* H, const float* const* row_scale,
                            const float* const* W_dec, const float* const* b_dec, dae_ctx* title_ctx, const float* feat,
                            int ld_feat, const float* OutW_T, const float* Out_b, const float* w_title, int B, int V,
                            const int32_t* cand_row_ptr, const int32_t* cand_col, int n_cand, float* out, int32_t* status)
{
    if (!members || M < 1 || !members[M - 1]) return dae_fail(title_ctx, DAE_ERR_ARG, "dae_ensemble_candidates: needs M >= 1 member contexts");
    const bool titled = title_ctx != nullptr;
    dae_ctx* rc_ctx = titled ? title_ctx : members[M - 1];
    if (!h || !H || !row_scale || !W_dec || !b_dec || !cand_row_ptr || !cand_col || !out) return dae_fail(rc_ctx, DAE_ERR_ARG, "null pointer");
    if (titled ? (!feat || !w_title || !OutW_T || !Out_b) : (feat || w_title || OutW_T || Out_b))
        return dae_fail(rc_ctx, DAE_ERR_ARG, titled ? "null pointer (feat / Output_W^T / Output_b / w_title of the title context)"
                                                    : "dae_ensemble_candidates: title tensors without a title context");
    if (B < 1 || B > 4096) return dae_fail(rc_ctx, DAE_ERR_ARG, "B=%d out of [1, 4096]", B);
    if (n_cand < 0) return dae_fail(rc_ctx, DAE_ERR_ARG, "n_cand=%d is negative", n_cand);
    if (V < 1) return dae_fail(rc_ctx, DAE_ERR_ARG, "bad shape V=%d", V);
    int Vimg = 0;
    int rc = dae_ensemble_check("dae_ensemble_candidates", rc_ctx, members, M, h, H, row_scale, title_ctx, ld_feat, -1, &Vimg);
    if (rc) return rc;
    for (int m = 0; m < M; ++m) {
        if (!W_dec[m] || !b_dec[m]) return dae_fail(rc_ctx, DAE_ERR_ARG, "null pointer (W_dec / b_dec of member %d)", m);
        if (reinterpret_cast<uintptr_t>(W_dec[m]) % 16) return dae_fail(rc_ctx, DAE_ERR_ARG, "the decoder tensor of member %d must be 16-byte aligned", m);
        if (H[m] % 4) return dae_fail(rc_ctx, DAE_ERR_ARG, "H=%d of member %d must be a multiple of 4", H[m], m);
    }
    if (titled && (reinterpret_cast<uintptr_t>(OutW_T) % 16 || ld_feat % 4))
        return dae_fail(rc_ctx, DAE_ERR_ARG, "Output_W^T must be 16-byte aligned and ld_feat=%d a multiple of 4", ld_feat);
    if (n_cand == 0) return DAE_OK;
    const int K = M + (titled ? 1 : 0);
    const dae_ens_scratch sp = dae_plan_ensemble_scratch(K, n_cand, 0, 0);
    rc = dae_reserve(rc_ctx, rc_ctx->rank_of, sp.total);
    if (rc) return rc;
    float* s = reinterpret_cast<float*>(static_cast<char*>(rc_ctx->rank_of.p) + sp.o_s);
    const dae_ens_tensors t{M, h, H, row_scale, W_dec, b_dec, feat, ld_feat, OutW_T, Out_b, w_title};
    return dae_launch_ensemble_candidates(rc_ctx, t, B, V, cand_row_ptr, cand_col, n_cand, s, sp.s_stride, out, status);
}

}  // extern "C"
