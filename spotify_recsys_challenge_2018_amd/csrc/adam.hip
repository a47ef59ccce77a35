// adam.hip -- K9 of the training step: the TF1 AdamOptimizer (DAEs.py:102), dense and on a row-sparse
// gradient.  The element update itself is dae_adam_el (train_common.h), shared with the armed decoder-gradient kernels.
#include "train_common.h"

namespace {

// ---- K9: TF1 AdamOptimizer, dense ------------------------------------------------
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, float* __restrict__ m,
                                                   float* __restrict__ v,
                                                   const float* __restrict__ g, size_t n,
                                                   float lr_t, float b1, float b2, float eps)
{
    const size_t n4 = n / 4;
    float4* p4 = reinterpret_cast<float4*>(p); float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v); const float4* g4 = reinterpret_cast<const float4*>(g);
    // two float4 groups per iteration: 8 independent 16-byte loads in flight per thread (HBM-bound: 7 passes
    // over the tensor).  Every byte is touched once: nontemporal loads and stores keep the 7 streams out of each
    // other's way in L2.
    const size_t stride = (size_t)gridDim.x * 256;
    size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (; o + stride < n4; o += 2 * stride) {
        const size_t o2 = o + stride;
        float4 pa = nt_ld4(p + 4 * o), ma = nt_ld4(m + 4 * o), va = nt_ld4(v + 4 * o);
        const float4 ga = nt_ld4(g + 4 * o);
        float4 pb = nt_ld4(p + 4 * o2), mb = nt_ld4(m + 4 * o2), vb = nt_ld4(v + 4 * o2);
        const float4 gb = nt_ld4(g + 4 * o2);
        dae_adam_el4(pa, ma, va, ga, lr_t, b1, b2, eps);
        dae_adam_el4(pb, mb, vb, gb, lr_t, b1, b2, eps);
        nt_st4(p + 4 * o, pa); nt_st4(m + 4 * o, ma); nt_st4(v + 4 * o, va);
        nt_st4(p + 4 * o2, pb); nt_st4(m + 4 * o2, mb); nt_st4(v + 4 * o2, vb);
    }
    for (; o < n4; o += stride) {
        float4 pp = p4[o], mm = m4[o], vv = v4[o];
        dae_adam_el4(pp, mm, vv, g4[o], lr_t, b1, b2, eps);
        p4[o] = pp; m4[o] = mm; v4[o] = vv;
    }
    for (size_t o = n4 * 4 + (size_t)blockIdx.x * 256 + threadIdx.x; o < n;
         o += (size_t)gridDim.x * 256) {
        float pp = p[o], mm = m[o], vv = v[o];
        dae_adam_el(pp, mm, vv, g[o], lr_t, b1, b2, eps);
        p[o] = pp; m[o] = mm; v[o] = vv;
    }
}

// ---- K9 on a ROW-SPARSE gradient: the same dense TF1 Adam, without the HBM passes over rows that have none ------
// The untied encoder's gradient is non-zero on the few thousand rows the batch's input names (4 % of 170 000).
// Dense Adam still moves every row (m and v decay, p follows m), which costs 7 passes over 174 MB per step.  A row
// without gradient, however, evolves by a recurrence nobody else reads: its state can stay at the step it was last
// current for (`last[row]`) and be brought up to date -- by running the SAME per-element update with g = 0 once per
// missed step, with the alpha each of those steps used (lr_tab[s]) -- when the row is next needed: before a step
// whose input names it (dae_adam_rows_begin), or for everyone at a sync point (dae_adam_rows_flush).  Every element
// sees exactly the operation sequence dense Adam would have applied, so the parameters are bit-identical
// (tests/test_gpu_train.py); only the memory traffic of untouched rows is gone.
// One wave per listed row; a row listed several times (a track in many playlists) is claimed once per launch through
// mark[row] (atomicExch with a per-launch stamp).
// MODE 0: begin  (listed rows -> current at step - 1)
// MODE 1: apply  (listed rows -> current at step - 1, then the update of `step` with their gradient row, which is
//                 zeroed again so that the dense gradient buffer stays all-zero between steps)
template <int MODE>
__global__ __launch_bounds__(256) void adam_rows_kernel(float* __restrict__ p, float* __restrict__ m,
                                                        float* __restrict__ v, float* __restrict__ g,
                                                        int* __restrict__ last, int* __restrict__ mark,
                                                        float* __restrict__ lr_tab, int n_rows, int row_len,
                                                        const int32_t* __restrict__ rows,
                                                        const int32_t* __restrict__ n_listed_dev, int n_listed_max,
                                                        float lr_t, float b1, float b2, float eps, int step)
{
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (MODE == 1 && blockIdx.x == 0 && threadIdx.x == 0) lr_tab[step] = lr_t;
    const int n_listed = n_listed_dev ? min(*n_listed_dev, n_listed_max) : n_listed_max;
    if (w >= n_listed) return;
    const int row = rows[w];
    if (row < 0 || row >= n_rows) return;
    const int stamp = 2 * step + MODE;
    // (round 6) Everything that depends on `row` alone is requested TOGETHER: the claim, the row's step and the first 64 float4 of
    // its state (the whole row at hidden 256) -- the wave was four dependent trips to memory (row, claim, step, state) for one
    // update, and a launch is ~100 such waves per CU: 27 + 30 us for 95 MB.  A wave that loses the claim has read lines the
    // winner reads anyway.
    const bool vec = (row_len & 3) == 0;
    const bool first_in = vec && lane < (row_len >> 2);
    const size_t o_first = ((size_t)row * row_len >> 2) + lane;
    float4 pp0 = make_float4(0.f, 0.f, 0.f, 0.f), mm0 = pp0, vv0 = pp0, gg0 = pp0;
    if (first_in) {
        pp0 = reinterpret_cast<float4*>(p)[o_first]; mm0 = reinterpret_cast<float4*>(m)[o_first];
        vv0 = reinterpret_cast<float4*>(v)[o_first];
        if (MODE == 1) gg0 = reinterpret_cast<float4*>(g)[o_first];
    }
    const int from = last[row];
    int claimed = 0;
    if (lane == 0) claimed = atomicExch(&mark[row], stamp) != stamp;
    claimed = __shfl(claimed, 0);
    if (!claimed) return;
    const int upto = step - 1;
    // four elements per lane at a time: the replay is a sequential recurrence per element (sqrt -> divide -> subtract),
    // so independent chains are the only instruction-level parallelism there is
    if (vec) {
        for (int c4 = lane; c4 < (row_len >> 2); c4 += 64) {
            const size_t o = ((size_t)row * row_len >> 2) + c4;
            const bool pre = c4 == lane;                           // the first round was requested above
            float4 pp = pre ? pp0 : reinterpret_cast<float4*>(p)[o], mm = pre ? mm0 : reinterpret_cast<float4*>(m)[o],
                   vv = pre ? vv0 : reinterpret_cast<float4*>(v)[o];
            for (int s_ = from + 1; s_ <= upto; ++s_) {
                dae_adam_el4(pp, mm, vv, make_float4(0.f, 0.f, 0.f, 0.f), lr_tab[s_], b1, b2, eps);
            }
            if (MODE == 1) {
                const float4 gg = pre ? gg0 : reinterpret_cast<float4*>(g)[o];
                dae_adam_el4(pp, mm, vv, gg, lr_t, b1, b2, eps);
                reinterpret_cast<float4*>(g)[o] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            reinterpret_cast<float4*>(p)[o] = pp; reinterpret_cast<float4*>(m)[o] = mm;
            reinterpret_cast<float4*>(v)[o] = vv;
        }
    } else
    for (int c = lane; c < row_len; c += 64) {
        const size_t o = (size_t)row * row_len + c;
        float pp = p[o], mm = m[o], vv = v[o];
        for (int s_ = from + 1; s_ <= upto; ++s_) {
            dae_adam_el(pp, mm, vv, 0.0f, lr_tab[s_], b1, b2, eps);
        }
        if (MODE == 1) {
            const float gg = g[o];
            dae_adam_el(pp, mm, vv, gg, lr_t, b1, b2, eps);
            g[o] = 0.0f;
        }
        p[o] = pp; m[o] = mm; v[o] = vv;
    }
    if (lane == 0) last[row] = MODE == 1 ? step : upto;
}

// every row -> current at `step` (sync points: evaluation, saving, sharding, ...); one wave per row
__global__ __launch_bounds__(256) void adam_rows_flush_kernel(float* __restrict__ p, float* __restrict__ m,
                                                              float* __restrict__ v, int* __restrict__ last,
                                                              const float* __restrict__ lr_tab, int n_rows,
                                                              int row_len, float b1, float b2, float eps, int step)
{
    const int lane = threadIdx.x & 63;
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < n_rows; row += gridDim.x * 4) {
        const int from = last[row];
        if (from >= step) continue;
        if ((row_len & 3) == 0) {
            for (int c4 = lane; c4 < (row_len >> 2); c4 += 64) {
                const size_t o = ((size_t)row * row_len >> 2) + c4;
                float4 pp = reinterpret_cast<float4*>(p)[o], mm = reinterpret_cast<float4*>(m)[o],
                       vv = reinterpret_cast<float4*>(v)[o];
                for (int s_ = from + 1; s_ <= step; ++s_) {
                    dae_adam_el4(pp, mm, vv, make_float4(0.f, 0.f, 0.f, 0.f), lr_tab[s_], b1, b2, eps);
                }
                reinterpret_cast<float4*>(p)[o] = pp; reinterpret_cast<float4*>(m)[o] = mm;
                reinterpret_cast<float4*>(v)[o] = vv;
            }
        } else
        for (int c = lane; c < row_len; c += 64) {
            const size_t o = (size_t)row * row_len + c;
            float pp = p[o], mm = m[o], vv = v[o];
            for (int s_ = from + 1; s_ <= step; ++s_) {
                dae_adam_el(pp, mm, vv, 0.0f, lr_tab[s_], b1, b2, eps);
            }
            p[o] = pp; m[o] = mm; v[o] = vv;
        }
        if (lane == 0) last[row] = step;
    }
}

}  // namespace

int dae_launch_adam(dae_ctx* ctx, float* param, float* m, float* v, const float* grad, int64_t n,
                    float lr_t, float beta1, float beta2, float eps)
{
    if (n <= 0) return DAE_OK;
    size_t work = (size_t)n / 4;
    hipLaunchKernelGGL(adam_kernel, dim3(grid_for(work ? work : 1)), dim3(256), 0, ctx->stream, param, m, v,
                       grad, (size_t)n, lr_t, beta1, beta2, eps);
    DAE_CHECK_LAUNCH(ctx, "adam_kernel");
    return DAE_OK;
}

int dae_launch_adam_rows(dae_ctx* ctx, int mode, float* param, float* m, float* v, float* grad, int32_t* last,
                         int32_t* mark, float* lr_tab, int n_rows, int row_len, const int32_t* rows,
                         const int32_t* n_listed_dev, int n_listed_max, float lr_t, float beta1, float beta2,
                         float eps, int step)
{
    if (mode == 2) {
        int blocks = (n_rows + 3) / 4;
        if (blocks > 16 * DAE_NUM_CU) blocks = 16 * DAE_NUM_CU;
        hipLaunchKernelGGL(adam_rows_flush_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, ctx->stream, param, m, v,
                           last, lr_tab, n_rows, row_len, beta1, beta2, eps, step);
        DAE_CHECK_LAUNCH(ctx, "adam_rows_flush_kernel");
        return DAE_OK;
    }
    // mode 1 always launches: its first thread records this step's alpha even when no row is listed
    const int blocks = (n_listed_max + 3) / 4 > 0 ? (n_listed_max + 3) / 4 : 1;
    if (mode == 0)
        hipLaunchKernelGGL(adam_rows_kernel<0>, dim3(blocks), dim3(256), 0, ctx->stream, param, m, v, grad, last, mark,
                           lr_tab, n_rows, row_len, rows, n_listed_dev, n_listed_max, lr_t, beta1, beta2, eps, step);
    else
        hipLaunchKernelGGL(adam_rows_kernel<1>, dim3(blocks), dim3(256), 0, ctx->stream, param, m, v, grad, last, mark,
                           lr_tab, n_rows, row_len, rows, n_listed_dev, n_listed_max, lr_t, beta1, beta2, eps, step);
    DAE_CHECK_LAUNCH(ctx, "adam_rows_kernel");
    return DAE_OK;
}
// alpha_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) with the beta powers kept as fp32 running products, as TF's
// beta1_power / beta2_power variables are.  The products are cached on the context (training calls this with
// t, t, t, t, t+1, ...): restarting the O(t) loop on every call costs milliseconds per step after 10^5 steps.
static float adam_alpha(dae_ctx* ctx, float lr, float beta1, float beta2, int t)
{
    if (ctx->adam_b1 != beta1 || ctx->adam_b2 != beta2 || t < ctx->adam_t) {
        ctx->adam_b1 = beta1; ctx->adam_b2 = beta2; ctx->adam_t = 0; ctx->adam_b1p = 1.0f; ctx->adam_b2p = 1.0f;
    }
    while (ctx->adam_t < t) { ctx->adam_b1p *= beta1; ctx->adam_b2p *= beta2; ++ctx->adam_t; }
    return lr * sqrtf(1.0f - ctx->adam_b2p) / (1.0f - ctx->adam_b1p);
}

extern "C" {

int dae_adam_step(dae_ctx* ctx, float* param, float* m, float* v, const float* grad, int64_t n,
                  float lr, float beta1, float beta2, float eps, int t)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!param || !m || !v || !grad) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (t < 1) return dae_fail(ctx, DAE_ERR_ARG, "t is the 1-based step count");
    if ((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(m) |
         reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(grad)) % 16)
        return dae_fail(ctx, DAE_ERR_ARG, "param, m, v, grad must be 16-byte aligned");
    const float alpha = adam_alpha(ctx, lr, beta1, beta2, t);
    return dae_launch_adam(ctx, param, m, v, grad, n, alpha, beta1, beta2, eps);
}

int dae_arm_decoder_adam(dae_ctx* ctx, float* m, float* v, float lr, float beta1, float beta2, float eps, int t)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!m || !v) { ctx->arm_m = nullptr; ctx->arm_v = nullptr; return DAE_OK; }          // disarm
    if (t < 1) return dae_fail(ctx, DAE_ERR_ARG, "t is the 1-based step count");
    if ((reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) % 16)
        return dae_fail(ctx, DAE_ERR_ARG, "m, v must be 16-byte aligned");
    ctx->arm_m = m; ctx->arm_v = v; ctx->arm_alpha = adam_alpha(ctx, lr, beta1, beta2, t);
    ctx->arm_b1 = beta1; ctx->arm_b2 = beta2; ctx->arm_eps = eps;
    return DAE_OK;
}

static int adam_rows_check(dae_ctx* ctx, const void* param, const void* m, const void* v, const void* state,
                           const void* lr_tab, int n_rows, int row_len, int tab_cap, int t)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!param || !m || !v || !state || !lr_tab) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (n_rows < 1 || row_len < 1) return dae_fail(ctx, DAE_ERR_ARG, "empty tensor");
    if (t < 1) return dae_fail(ctx, DAE_ERR_ARG, "t is the 1-based step count");
    if (t >= tab_cap) return dae_fail(ctx, DAE_ERR_ARG, "step %d does not fit the alpha table (%d entries)", t, tab_cap);
    return DAE_OK;
}

int dae_adam_rows_begin(dae_ctx* ctx, float* param, float* m, float* v, int32_t* state, float* lr_tab, int tab_cap,
                        int n_rows, int row_len, const int32_t* rows, const int32_t* n_listed_dev, int n_listed_max,
                        float beta1, float beta2, float eps, int t)
{
    int rc = adam_rows_check(ctx, param, m, v, state, lr_tab, n_rows, row_len, tab_cap, t);
    if (rc) return rc;
    if (n_listed_max <= 0) return DAE_OK;
    if (!rows) return dae_fail(ctx, DAE_ERR_ARG, "null row list");
    return dae_launch_adam_rows(ctx, 0, param, m, v, nullptr, state, state + n_rows, lr_tab, n_rows, row_len, rows,
                                n_listed_dev, n_listed_max, 0.0f, beta1, beta2, eps, t);
}

int dae_adam_rows_apply(dae_ctx* ctx, float* param, float* m, float* v, float* grad, int32_t* state, float* lr_tab,
                        int tab_cap, int n_rows, int row_len, const int32_t* rows, const int32_t* n_listed_dev,
                        int n_listed_max, float lr, float beta1, float beta2, float eps, int t)
{
    int rc = adam_rows_check(ctx, param, m, v, state, lr_tab, n_rows, row_len, tab_cap, t);
    if (rc) return rc;
    if (!grad || (n_listed_max > 0 && !rows)) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    const float alpha = adam_alpha(ctx, lr, beta1, beta2, t);
    return dae_launch_adam_rows(ctx, 1, param, m, v, grad, state, state + n_rows, lr_tab, n_rows, row_len, rows,
                                n_listed_dev, n_listed_max < 0 ? 0 : n_listed_max, alpha, beta1, beta2, eps, t);
}

int dae_adam_rows_flush(dae_ctx* ctx, float* param, float* m, float* v, int32_t* state, const float* lr_tab,
                        int tab_cap, int n_rows, int row_len, float beta1, float beta2, float eps, int t)
{
    if (t == 0) return DAE_OK;
    int rc = adam_rows_check(ctx, param, m, v, state, lr_tab, n_rows, row_len, tab_cap, t);
    if (rc) return rc;
    return dae_launch_adam_rows(ctx, 2, param, m, v, nullptr, state, nullptr, const_cast<float*>(lr_tab), n_rows, row_len,
                                nullptr, nullptr, 0, 0.0f, beta1, beta2, eps, t);
}

}  // extern "C"
