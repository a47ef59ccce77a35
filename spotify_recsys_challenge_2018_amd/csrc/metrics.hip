// metrics.hip -- the challenge's three ranking metrics (the reference's utils/metrics.py: get_r_precision, get_ndcg, get_rsc)
// from the top-k lists where the rankers leave them: one small record per row instead of the row's k indices.
//
// The kernel counts and adds, the divisions stay with the host (utils/metrics.py finish_*), so the floats are Python's own.
// The only floating-point work here is the DCG: float64 ADDITIONS of the caller's discount table, one per hit, in ascending
// position -- the order get_ndcg adds them in.  Every lane of the wave walks the same ballot masks, so the sum is sequential
// and never reassociated; that is what makes the record bit-equal to the reference's loop (tests/test_gpu_metrics.py).
#include "dae_internal.h"

namespace {

constexpr int MET_CAP = 1024;     // answers of a row in LDS at a time; longer rows take several passes over the same code

// One wave per row (a workgroup is one wave, so its barriers cost nothing and never meet another row's trip count).  Lane l
// holds the list entries l, 64 + l, ...: the ballot of slot j is the hit mask of positions 64 j .. 64 j + 63 in order.
// A row's candidates are its entries >= 0 IN ORDER (the rankers pad the tail with -1; an entry < 0 anywhere is skipped and
// does not count as a position, which is what eval_topk's filter does).
template <int NS>
__global__ __launch_bounds__(64) void rank_metrics_kernel(const int32_t* __restrict__ idx, int64_t ld, int B, int k,
                                                          const int32_t* __restrict__ ans_rp, const int32_t* __restrict__ ans_col,
                                                          const double* __restrict__ disc, dae_metric_rec* __restrict__ out)
{
    __shared__ int32_t s_ans[MET_CAP];
    const int row = blockIdx.x, lane = threadIdx.x;
    if (row >= B) return;
    const int a0 = ans_rp[row];
    const int n = ans_rp[row + 1] - a0;
    int32_t cand[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int p = j * 64 + lane;
        cand[j] = p < k ? idx[(int64_t)row * ld + p] : -1;
    }
    uint32_t hit = 0;             // bit j: cand[j] is one of the row's answers
    for (int c0 = 0; c0 < n; c0 += MET_CAP) {
        const int nc = n - c0 < MET_CAP ? n - c0 : MET_CAP;
        __syncthreads();          // (the pass before has been read)
        for (int i = lane; i < nc; i += 64) s_ans[i] = ans_col[(int64_t)a0 + c0 + i];
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < nc; ++i) {
            const int32_t v = s_ans[i];
#pragma unroll
            for (int j = 0; j < NS; ++j) hit |= (cand[j] == v ? 1u : 0u) << j;
        }
    }
    int hits_r = 0, first = -1, m = 0, base = 0;
    double dcg = 0.0;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const bool ok = cand[j] >= 0;                        // (an answer of -1 -- a track outside the vocabulary -- hits nothing)
        const uint64_t valid = __ballot(ok);
        uint64_t hm = __ballot(ok && ((hit >> j) & 1u));
        while (hm) {                                         // wave-uniform: ascending positions
            const int b = __ffsll((unsigned long long)hm) - 1;
            hm &= hm - 1;
            const int p = base + __popcll(valid & ((1ull << b) - 1ull));
            if (first < 0) first = p;
            if (p < n) ++hits_r;
            if (p == 0) dcg = 1.0;
            else { dcg += disc[p]; ++m; }
        }
        base += __popcll(valid);
    }
    if (lane == 0) {
        dae_metric_rec r;
        r.hits_r = hits_r; r.first = first; r.m = m; r.n_answer = n > 0 ? n : 0; r.dcg = dcg;
        out[row] = r;
    }
}

}  // namespace

extern "C" int dae_rank_metrics(dae_ctx* ctx, const int32_t* idx, int64_t ld, int B, int k, const int32_t* ans_row_ptr,
                                const int32_t* ans_col, const double* disc, dae_metric_rec* out)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!idx || !ans_row_ptr || !disc || !out) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (k > DAE_MAX_K) return dae_fail(ctx, DAE_ERR_ARG, "dae_rank_metrics: k=%d out of [1,%d]", k, DAE_MAX_K);
    if (k < 1 || ld < k || B < 0) return dae_fail(ctx, DAE_ERR_ARG, "dae_rank_metrics: bad shape B=%d k=%d ld=%lld", B, k, (long long)ld);
    if (B == 0) return DAE_OK;
    if (k <= 512)
        hipLaunchKernelGGL(rank_metrics_kernel<8>, dim3(B), dim3(64), 0, ctx->stream, idx, ld, B, k, ans_row_ptr, ans_col, disc, out);
    else
        hipLaunchKernelGGL(rank_metrics_kernel<DAE_MAX_K / 64>, dim3(B), dim3(64), 0, ctx->stream, idx, ld, B, k, ans_row_ptr, ans_col, disc, out);
    DAE_CHECK_LAUNCH(ctx, "rank_metrics_kernel");
    return DAE_OK;
}
