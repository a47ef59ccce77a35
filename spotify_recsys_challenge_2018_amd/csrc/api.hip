// api.hip -- the C ABI of libdae_hip.so (include/dae_hip.h) apart from what lives next to its kernels: the context and its
// scratch, the setters and read-outs, the decoder images' prepack / share entry points, and the thin argument-checking
// wrappers of the csr, encode, train, title and selection launchers.  The scoring launch sequences are score.hip's, the Adam
// entry points adam.hip's.  One kernel lives here: dae_clock_probe's.
#include <stdarg.h>

#include <climits>

#include "dae_internal.h"

thread_local std::string g_dae_create_err;

int dae_fail(dae_ctx* ctx, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_dae_create_err = buf;
    return code;
}

int dae_reserve(dae_ctx* ctx, dae_buf& b, size_t bytes)
{
    if (bytes <= b.bytes && b.p) return DAE_OK;
    if (bytes == 0) bytes = 16;
    if (b.p) {
        // growing: drain the stream first, the old buffer may still be in use
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return dae_fail(ctx, DAE_ERR_HIP, "sync before regrow: %s", hipGetErrorString(e));
        (void)hipFree(b.p);
        ctx->scratch_total -= b.bytes;
        b.p = nullptr; b.bytes = 0;
    }
    bytes = (bytes + 255) & ~(size_t)255;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess)
        return dae_fail(ctx, DAE_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    b.p = p; b.bytes = bytes;
    ctx->scratch_total += bytes;
    return DAE_OK;
}

int dae_ensure_guard(dae_ctx* ctx)
{
    if (ctx->guard.p) return DAE_OK;
    int rc = dae_reserve(ctx, ctx->guard, DAE_GUARD_BYTES);
    if (rc) return rc;
    DAE_HIP_CHECK(ctx, hipMemsetAsync(ctx->guard.p, 0, DAE_GUARD_BYTES, ctx->stream));
    return DAE_OK;
}

extern "C" {

int dae_version(void) { return 1002; }

int dae_create(int device, dae_ctx** out)
{
    if (!out) return dae_fail(nullptr, DAE_ERR_ARG, "out is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return dae_fail(nullptr, DAE_ERR_HIP, "no HIP device available (%s)", hipGetErrorString(e));
    if (device < 0 || device >= n)
        return dae_fail(nullptr, DAE_ERR_ARG, "device %d out of range [0,%d)", device, n);
    e = hipSetDevice(device);
    if (e != hipSuccess) return dae_fail(nullptr, DAE_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return dae_fail(nullptr, DAE_ERR_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return dae_fail(nullptr, DAE_ERR_HIP, "device %d is %s; this library is built for gfx950 only",
                        device, prop.gcnArchName);
    dae_ctx* c = new dae_ctx();
    c->device = device;
    *out = c;
    return DAE_OK;
}

int dae_destroy(dae_ctx* ctx)
{
    if (!ctx) return DAE_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    auto release = [](dae_buf& b) { if (b.p) (void)hipFree(b.p); };
    for (dae_packed* pk : {&ctx->pk_f32, &ctx->pk_bf16}) {
        if (!pk->borrowed) dae_packed_shared_bufs(*pk, release);       // (a borrowed image is its owner's to free)
        release(pk->order); release(pk->ident);
    }
    for (dae_buf* b : {&ctx->h_packed, &ctx->sample, &ctx->tau, &ctx->sample_top, &ctx->cand, &ctx->cand_cnt, &ctx->gmax,
                       &ctx->h_packed16, &ctx->h_scratch, &ctx->train_a, &ctx->train_b, &ctx->train_c, &ctx->train_d, &ctx->csr_tmp,
                       &ctx->feed_tmp, &ctx->row_bad, &ctx->guard, &ctx->refined, &ctx->refstat, &ctx->mix_fhat, &ctx->title_scratch,
                       &ctx->tile_band, &ctx->title_tab, &ctx->audit, &ctx->audit_stat, &ctx->title_y1, &ctx->live, &ctx->skip_stat, &ctx->live_sync,
                       &ctx->row_d, &ctx->samp_tab, &ctx->sskip_stat,
                       &ctx->cand_list, &ctx->cat_seeds, &ctx->rank_of, &ctx->loss_rows, &ctx->mix_loss})
        release(*b);
    for (hipEvent_t ev : ctx->prof_ev) (void)hipEventDestroy(ev);
    delete ctx;
    return DAE_OK;
}

int dae_set_stream(dae_ctx* ctx, void* hip_stream)
{
    if (!ctx) return DAE_ERR_ARG;
    ctx->stream = static_cast<hipStream_t>(hip_stream);
    return DAE_OK;
}

const char* dae_last_error(const dae_ctx* ctx)
{
    return ctx ? ctx->err.c_str() : g_dae_create_err.c_str();
}

size_t dae_scratch_bytes(const dae_ctx* ctx) { return ctx ? ctx->scratch_total : 0; }

int dae_profile_enable(dae_ctx* ctx, int on)
{
    if (!ctx) return DAE_ERR_ARG;
    ctx->prof_on = on != 0;
    ctx->prof_used = 0;
    return DAE_OK;
}

int dae_profile_read(dae_ctx* ctx, double* ms_total, int* launches)
{
    if (!ctx) return DAE_ERR_ARG;
    double tot = 0.0;
    int n = 0;
    for (size_t i = 0; i + 1 < ctx->prof_used; i += 2) {
        DAE_HIP_CHECK(ctx, hipEventSynchronize(ctx->prof_ev[i + 1]));
        float ms = 0.f;
        DAE_HIP_CHECK(ctx, hipEventElapsedTime(&ms, ctx->prof_ev[i], ctx->prof_ev[i + 1]));
        tot += ms; ++n;
    }
    ctx->prof_used = 0;
    if (ms_total) *ms_total = tot;
    if (launches) *launches = n;
    return DAE_OK;
}

const char* dae_profile_kernel(const dae_ctx* ctx) { return ctx ? ctx->prof_kernel.c_str() : ""; }

namespace {
__global__ __launch_bounds__(64) void clock_probe_kernel(unsigned long long* out, unsigned long long ticks)
{
    if (threadIdx.x != 0) return;
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long c0 = __builtin_amdgcn_s_memtime();
    unsigned long long r1 = r0;
    while (r1 - r0 < ticks) {
        __builtin_amdgcn_s_sleep(16);
        r1 = __builtin_amdgcn_s_memrealtime();
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    r1 = __builtin_amdgcn_s_memrealtime();
    out[0] = c1 - c0;
    out[1] = r1 - r0;
}
}  // namespace

int dae_clock_probe(dae_ctx* ctx, void* hip_stream, int window_us, uint64_t* out2_dev, int* wall_khz_out)
{
    if (!ctx || !out2_dev || window_us < 1 || window_us > 1000000) return dae_fail(ctx, DAE_ERR_ARG, "dae_clock_probe: bad arguments");
    int khz = 0;
    DAE_HIP_CHECK(ctx, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
    if (khz <= 0) return dae_fail(ctx, DAE_ERR_STATE, "dae_clock_probe: no wall clock rate");
    if (wall_khz_out) *wall_khz_out = khz;
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
    const unsigned long long ticks = (unsigned long long)window_us * (unsigned long long)khz / 1000ull;
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<unsigned long long*>(out2_dev), ticks);
    DAE_CHECK_LAUNCH(ctx, "clock_probe_kernel");
    return DAE_OK;
}

int dae_coo_to_csr(dae_ctx* ctx, const int64_t* positions, const float* values, int values_broadcast,
                   int64_t nnz, int n_rows, int n_cols, int32_t* row_ptr, int32_t* col, float* val,
                   int32_t* status)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!row_ptr || !status || (nnz > 0 && (!positions || !values || !col || !val)))
        return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (nnz < 0 || nnz >= (int64_t)1 << 31) return dae_fail(ctx, DAE_ERR_ARG, "nnz=%lld out of range", (long long)nnz);
    if (n_rows < 1 || n_cols < 1) return dae_fail(ctx, DAE_ERR_ARG, "bad shape %d x %d", n_rows, n_cols);
    return dae_launch_coo_to_csr(ctx, positions, values, values_broadcast, nnz, n_rows, n_cols, row_ptr, col, val,
                                 status);
}

int dae_seeds_from_csr(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, int B, int n_tracks,
                       int32_t* seed_row_ptr, int32_t* seed_col)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!row_ptr || !col || !seed_row_ptr || !seed_col) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (B <= 0) return DAE_OK;
    return dae_launch_seeds_from_csr(ctx, row_ptr, col, B, n_tracks, seed_row_ptr, seed_col);
}

int dae_encode(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val,
               const float* W_enc, const float* b_enc, int V, int H, int B,
               float ikp, float kp, uint32_t seed, float* h_out)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!row_ptr || !W_enc || !b_enc || !h_out) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (H <= 0 || (H % 4) != 0) return dae_fail(ctx, DAE_ERR_ARG, "H=%d must be a positive multiple of 4", H);
    if (B < 0 || V <= 0) return dae_fail(ctx, DAE_ERR_ARG, "bad shape B=%d V=%d", B, V);
    if (!(ikp > 0.f && ikp <= 1.f) || !(kp > 0.f && kp <= 1.f))
        return dae_fail(ctx, DAE_ERR_ARG, "keep probabilities must be in (0,1]");
    if ((reinterpret_cast<uintptr_t>(W_enc) | reinterpret_cast<uintptr_t>(b_enc) |
         reinterpret_cast<uintptr_t>(h_out)) % 16)
        return dae_fail(ctx, DAE_ERR_ARG, "W_enc, b_enc, h_out must be 16-byte aligned");
    return dae_launch_encode(ctx, row_ptr, col, val, W_enc, b_enc, V, H, B, ikp, kp, seed, h_out,
                             nullptr, 0, 0);
}

// a slot that borrows another context's image gets buffers of its own again before it is written
static void unborrow(dae_packed& pk)
{
    if (!pk.borrowed) return;
    dae_packed_shared_bufs(pk, [](dae_buf& b) { b = dae_buf{}; });
    pk.borrowed = false; pk.valid = false; pk.exact = false; pk.order_nrank = -1;
}

int dae_share_decoder(dae_ctx* dst, const dae_ctx* src, int dtype)
{
    if (!dst) return DAE_ERR_ARG;
    if (!src || src == dst) return dae_fail(dst, DAE_ERR_ARG, "dae_share_decoder: needs another context");
    if (dst->device != src->device) return dae_fail(dst, DAE_ERR_ARG, "dae_share_decoder: contexts on different devices");
    if (!dae_known_dtype(dtype)) return dae_fail(dst, DAE_ERR_ARG, "unknown dtype %d", dtype);
    const dae_packed& sp = dtype == DAE_DTYPE_F32 ? src->pk_f32 : src->pk_bf16;
    dae_packed& dp = dtype == DAE_DTYPE_F32 ? dst->pk_f32 : dst->pk_bf16;
    if (!sp.valid || (dtype == DAE_DTYPE_BF16_EXACT && !sp.exact))
        return dae_fail(dst, DAE_ERR_STATE, "dae_share_decoder: the source context holds no such image");
    if (sp.borrowed) return dae_fail(dst, DAE_ERR_ARG, "dae_share_decoder: share from the context that owns the image");
    if (!dp.borrowed) {                                    // drop the own image of this slot (after its last use)
        hipError_t e = hipStreamSynchronize(dst->stream);
        if (e != hipSuccess) return dae_fail(dst, DAE_ERR_HIP, "sync: %s", hipGetErrorString(e));
        dae_packed_shared_bufs(dp, [&](dae_buf& b) {
            if (b.p) { (void)hipFree(b.p); dst->scratch_total -= b.bytes; b = dae_buf{}; }
        });
    }
    const dae_buf order = dp.order, ident = dp.ident;      // the tile lists stay this context's own (small, built lazily)
    dp = sp;
    dp.order = order; dp.ident = ident; dp.order_nrank = -1; dp.order_nsamp = -1;
    dp.borrowed = true;
    int rc = dae_reserve(dst, dp.ident, (size_t)(dp.ntiles > 0 ? dp.ntiles : 1) * sizeof(int));
    if (rc) return rc;
    return dae_launch_tile_iota(dst, static_cast<int*>(dp.ident.p), dp.ntiles);
}

int dae_prepack_decoder(dae_ctx* ctx, const float* W_dec, const float* b_dec, int V, int H,
                        int col_lo, int col_hi, int dtype)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!W_dec || !b_dec) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (H <= 0 || V <= 0 || col_lo < 0 || col_hi > V || col_lo >= col_hi)
        return dae_fail(ctx, DAE_ERR_ARG, "bad shape V=%d H=%d cols=[%d,%d)", V, H, col_lo, col_hi);
    unborrow(dtype == DAE_DTYPE_F32 ? ctx->pk_f32 : ctx->pk_bf16);
    if (dtype == DAE_DTYPE_F32) return dae_launch_prepack_f32(ctx, W_dec, b_dec, V, H, col_lo, col_hi);
    if (dtype == DAE_DTYPE_BF16) return dae_launch_prepack_bf16(ctx, W_dec, b_dec, V, H, col_lo, col_hi);
    if (dtype == DAE_DTYPE_BF16_EXACT) return dae_launch_prepack_bf16(ctx, W_dec, b_dec, V, H, col_lo, col_hi, 1);
    return dae_fail(ctx, DAE_ERR_ARG, "unknown dtype %d", dtype);
}

int dae_prepack_decoder_rows(dae_ctx* ctx, const float* W_rows, const float* b_rows, int n_rows, int H, int col_lo,
                             int dtype)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!W_rows || !b_rows) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (n_rows <= 0 || H <= 0 || col_lo < 0 || (int64_t)col_lo + n_rows > INT_MAX)
        return dae_fail(ctx, DAE_ERR_ARG, "bad shape n_rows=%d H=%d col_lo=%d", n_rows, H, col_lo);
    // the prepack kernels index their arguments by GLOBAL column and read rows [col_lo, col_hi) only (prepack_tile_kernel,
    // exact_bounds_kernel, the W32 copy: each forms W + v * H with col_lo <= v < col_hi): the shifted base is never
    // dereferenced below row col_lo
    const float* W = W_rows - (size_t)col_lo * H;
    const float* b = b_rows - (size_t)col_lo;
    return dae_prepack_decoder(ctx, W, b, col_lo + n_rows, H, col_lo, col_lo + n_rows, dtype);
}

int dae_exact_bounds(dae_ctx* ctx, float* eps_out)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!eps_out) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    const dae_packed& pk = ctx->pk_bf16;
    if (!pk.valid || !pk.exact) return dae_fail(ctx, DAE_ERR_STATE, "decoder weights not prepacked with DAE_DTYPE_BF16_EXACT");
    DAE_HIP_CHECK(ctx, hipMemcpyAsync(eps_out, pk.eps.p, (size_t)(pk.col_hi - pk.col_lo) * sizeof(float),
                                      hipMemcpyDeviceToDevice, ctx->stream));
    return DAE_OK;
}

int dae_exact_stats_read(dae_ctx* ctx, uint64_t out3[3])
{
    if (!ctx) return DAE_ERR_ARG;
    if (!out3) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    out3[0] = out3[1] = out3[2] = 0;
    const int n = ctx->refstat_rows;
    if (!ctx->refstat.p || n <= 0) return DAE_OK;
    std::vector<int> h((size_t)2 * n);
    DAE_HIP_CHECK(ctx, hipMemcpyAsync(h.data(), ctx->refstat.p, h.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    DAE_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    out3[0] = (uint64_t)n;
    for (int r = 0; r < n; ++r) { out3[1] += (uint64_t)h[2 * r]; out3[2] += (uint64_t)h[2 * r + 1]; }
    return DAE_OK;
}

int dae_set_filter_skip(dae_ctx* ctx, int on)
{
    if (!ctx) return DAE_ERR_ARG;
    ctx->filter_skip = on ? 1 : 0;
    return DAE_OK;
}

int dae_filter_skip_read(dae_ctx* ctx, uint64_t out3[3])
{
    if (!ctx) return DAE_ERR_ARG;
    if (!out3) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    out3[0] = out3[1] = out3[2] = 0;
    if (!ctx->skip_stat.p) return DAE_OK;
    unsigned long long h[3] = {0, 0, 0};
    DAE_HIP_CHECK(ctx, hipMemcpyAsync(h, ctx->skip_stat.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    DAE_HIP_CHECK(ctx, hipMemsetAsync(ctx->skip_stat.p, 0, sizeof(h), ctx->stream));
    DAE_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 3; ++i) out3[i] = (uint64_t)h[i];
    return DAE_OK;
}

int dae_live_proof_read(dae_ctx* ctx, uint64_t* groups_proved)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!groups_proved) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    *groups_proved = 0;
    if (!ctx->skip_stat.p) return DAE_OK;
    unsigned long long h = 0;                               // the fourth word: dae_filter_skip_read keeps its three
    unsigned long long* const word = static_cast<unsigned long long*>(ctx->skip_stat.p) + 3;
    DAE_HIP_CHECK(ctx, hipMemcpyAsync(&h, word, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    DAE_HIP_CHECK(ctx, hipMemsetAsync(word, 0, sizeof(h), ctx->stream));
    DAE_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *groups_proved = (uint64_t)h;
    return DAE_OK;
}

int dae_sample_skip_read(dae_ctx* ctx, uint64_t out3[3])
{
    if (!ctx) return DAE_ERR_ARG;
    if (!out3) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    out3[0] = out3[1] = out3[2] = 0;
    if (!ctx->sskip_stat.p) return DAE_OK;
    unsigned long long slots[DAE_SSKIP_SLOTS];              // one word per workgroup of the sample launch: summed here
    DAE_HIP_CHECK(ctx, hipMemcpyAsync(slots, ctx->sskip_stat.p, sizeof(slots), hipMemcpyDeviceToHost, ctx->stream));
    DAE_HIP_CHECK(ctx, hipMemsetAsync(ctx->sskip_stat.p, 0, sizeof(slots), ctx->stream));
    DAE_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    unsigned long long h = 0;
    for (unsigned long long v : slots) h += v;
    out3[0] = (uint64_t)ctx->sskip_launches; out3[1] = (uint64_t)ctx->sskip_planned; out3[2] = (uint64_t)h;
    ctx->sskip_launches = ctx->sskip_planned = 0;
    return DAE_OK;
}

int dae_last_tau_read(dae_ctx* ctx, float* tau_out, int B)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!tau_out || B < 1) return dae_fail(ctx, DAE_ERR_ARG, "dae_last_tau_read: bad arguments");
    if (!ctx->tau.p || (size_t)B * sizeof(float) > ctx->tau.bytes) return dae_fail(ctx, DAE_ERR_STATE, "no thresholds of %d rows on this context", B);
    DAE_HIP_CHECK(ctx, hipMemcpyAsync(tau_out, ctx->tau.p, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    DAE_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return DAE_OK;
}

int dae_filter_skip_last(dae_ctx* ctx, int32_t* live_out, int cap, int* n_rg_out)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!n_rg_out || (cap > 0 && !live_out)) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    *n_rg_out = ctx->live_n_rg;
    const int n = ctx->live_n_rg < cap ? ctx->live_n_rg : cap;
    if (n <= 0) return DAE_OK;
    DAE_HIP_CHECK(ctx, hipMemcpyAsync(live_out, ctx->live.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    DAE_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return DAE_OK;
}

int dae_tile_bounds_read(dae_ctx* ctx, float* ub_out, int cap_tiles, int* ntiles_out)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!ntiles_out || (cap_tiles > 0 && !ub_out)) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    const dae_packed& pk = ctx->pk_f32;
    if (!pk.valid || !pk.ub_valid || !pk.tile_ub.p) return dae_fail(ctx, DAE_ERR_STATE, "no fp32 decoder image with tile bounds");
    *ntiles_out = pk.ntiles;
    const int n = pk.ntiles < cap_tiles ? pk.ntiles : cap_tiles;
    if (n <= 0) return DAE_OK;
    DAE_HIP_CHECK(ctx, hipMemcpyAsync(ub_out, pk.tile_ub.p, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    DAE_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return DAE_OK;
}

int dae_set_exact_margin(dae_ctx* ctx, float scale)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!(scale > 0.0f) || !(scale <= 1024.0f)) return dae_fail(ctx, DAE_ERR_ARG, "dae_set_exact_margin: scale must be in (0, 1024]");
    ctx->exact_margin = scale;
    return DAE_OK;
}

int dae_exact_guard_read(dae_ctx* ctx, int32_t* violations, int32_t* column)
{
    if (!ctx) return DAE_ERR_ARG;
    int32_t w[2] = {0, -1};
    if (ctx->guard.p) {
        DAE_HIP_CHECK(ctx, hipMemcpyAsync(w, ctx->guard.p, sizeof(w), hipMemcpyDeviceToHost, ctx->stream));
        DAE_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (w[0] != 0) DAE_HIP_CHECK(ctx, hipMemsetAsync(ctx->guard.p, 0, sizeof(w), ctx->stream));
    }
    if (violations) *violations = w[0];
    if (column) *column = w[0] ? w[1] : -1;
    return DAE_OK;
}

int dae_exact_guard_words(dae_ctx* ctx, const int32_t** words_dev)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!words_dev) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    const int rc = dae_ensure_guard(ctx);
    if (rc) return rc;
    *words_dev = static_cast<const int32_t*>(ctx->guard.p);
    return DAE_OK;
}

int dae_exact_guard_snapshot(dae_ctx* ctx, int32_t* words_out_dev)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!words_out_dev) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    const int32_t* gw = nullptr;
    const int rc = dae_exact_guard_words(ctx, &gw);
    if (rc) return rc;
    DAE_HIP_CHECK(ctx, hipMemcpyAsync(words_out_dev, gw, DAE_GUARD_BYTES, hipMemcpyDeviceToDevice, ctx->stream));
    return DAE_OK;
}

int dae_topk_dense(dae_ctx* ctx, const float* logits, int64_t ld, int B, int ncols, int col_base,
                   const int32_t* seed_row_ptr, const int32_t* seed_col, int k, int out_kind,
                   float* out_score, int32_t* out_idx)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!logits || !out_score || !out_idx) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (ncols < 0 || ld < ncols) return dae_fail(ctx, DAE_ERR_ARG, "bad ncols/ld");
    if ((seed_row_ptr == nullptr) != (seed_col == nullptr))
        return dae_fail(ctx, DAE_ERR_ARG, "seed_row_ptr and seed_col must both be given or both null");
    dae_topk_args ta;
    memset(&ta, 0, sizeof(ta));
    ta.B = B; ta.k = k; ta.out_kind = out_kind;
    ta.bitmap_base = col_base; ta.bitmap_n = ncols;
    ta.seed_row_ptr = seed_row_ptr; ta.seed_col = seed_col;
    ta.out_score = out_score; ta.out_idx = out_idx;
    dae_dense_src ds{logits, ld, ncols, col_base, 1};
    return dae_launch_topk_dense(ctx, ds, ta);
}

int dae_topk_merge(dae_ctx* ctx, int G, int B, int k, const float* cand_logit,
                   const int32_t* cand_idx, int out_kind, float* out_score, int32_t* out_idx)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!cand_logit || !cand_idx || !out_score || !out_idx) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (G < 1) return dae_fail(ctx, DAE_ERR_ARG, "G=%d", G);
    dae_topk_args ta;
    memset(&ta, 0, sizeof(ta));
    ta.B = B; ta.k = k; ta.out_kind = out_kind;
    ta.out_score = out_score; ta.out_idx = out_idx;
    return dae_launch_topk_soa(ctx, G, cand_logit, cand_idx, ta);
}

int dae_set_train_dtype(dae_ctx* ctx, int dtype)
{
    if (!ctx) return DAE_ERR_ARG;
    if (dtype != DAE_DTYPE_F32 && dtype != DAE_DTYPE_BF16) return dae_fail(ctx, DAE_ERR_ARG, "unknown dtype %d", dtype);
    ctx->train_dtype = dtype;
    return DAE_OK;
}

int dae_train_forward_backward(dae_ctx* ctx,
        const int32_t* x_row_ptr, const int32_t* x_col, const float* x_val,
        const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
        const float* W_enc, const float* b_enc, const float* W_dec, const float* b_dec,
        int V, int H, int B, int n_batch, int tied,
        float ikp, float kp, uint32_t seed, float reg_lambda,
        float* gW_enc, float* gb_enc, float* gW_dec, float* gb_dec, float* cost_out)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!x_row_ptr || !y_row_ptr || !W_enc || !b_enc || !b_dec || !gW_enc || !gb_enc || !gb_dec || !cost_out)
        return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (!tied && (!W_dec || (!gW_dec && !ctx->arm_m)))
        return dae_fail(ctx, DAE_ERR_ARG, "untied model needs W_dec and gW_dec (or the armed decoder Adam)");
    if (V <= 0 || H <= 0 || B <= 0 || n_batch <= 0) return dae_fail(ctx, DAE_ERR_ARG, "bad shape");
    if (!(ikp > 0.f && ikp <= 1.f) || !(kp > 0.f && kp <= 1.f))
        return dae_fail(ctx, DAE_ERR_ARG, "keep probabilities must be in (0,1]");
    return dae_train_step_f32(ctx, x_row_ptr, x_col, x_val, y_row_ptr, y_col, y_val, W_enc, b_enc,
                              W_dec, b_dec, V, H, B, n_batch, tied, ikp, kp, seed, reg_lambda,
                              gW_enc, gb_enc, gW_dec, gb_dec, cost_out);
}

static int check_shard(dae_ctx* ctx, int col_lo, int col_hi, int H, int B, float ikp, float kp)
{
    if (col_lo < 0 || col_hi <= col_lo) return dae_fail(ctx, DAE_ERR_ARG, "bad shard [%d,%d)", col_lo, col_hi);
    if (H <= 0 || B <= 0) return dae_fail(ctx, DAE_ERR_ARG, "bad shape");
    if (!(ikp > 0.f && ikp <= 1.f) || !(kp > 0.f && kp <= 1.f))
        return dae_fail(ctx, DAE_ERR_ARG, "keep probabilities must be in (0,1]");
    return DAE_OK;
}

int dae_train_shard_encode(dae_ctx* ctx,
        const int32_t* x_row_ptr, const int32_t* x_col, const float* x_val,
        const float* W_enc_loc, int col_lo, int col_hi, int H, int B,
        float ikp, uint32_t seed, float* pre_partial)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!x_row_ptr || !W_enc_loc || !pre_partial) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    int rc = check_shard(ctx, col_lo, col_hi, H, B, ikp, 1.0f);
    if (rc) return rc;
    return dae_train_shard_encode_f32(ctx, x_row_ptr, x_col, x_val, W_enc_loc, col_lo, col_hi, H, B,
                                      ikp, seed, pre_partial);
}

int dae_train_shard_decode(dae_ctx* ctx, const float* pre, const float* b_enc,
        const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
        const float* W_enc_loc, const float* W_dec_loc, const float* b_dec_loc,
        int col_lo, int col_hi, int H, int B, int n_batch, int tied,
        float kp, uint32_t seed, float reg_lambda,
        float* gW_out, float* gb_dec_loc, float* dh_partial, float* cost_partial)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!pre || !b_enc || !y_row_ptr || !W_enc_loc || !b_dec_loc || !gW_out || !gb_dec_loc || !dh_partial ||
        !cost_partial)
        return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (!tied && !W_dec_loc) return dae_fail(ctx, DAE_ERR_ARG, "untied model needs W_dec_loc");
    if (n_batch <= 0) return dae_fail(ctx, DAE_ERR_ARG, "bad shape");
    int rc = check_shard(ctx, col_lo, col_hi, H, B, 1.0f, kp);
    if (rc) return rc;
    return dae_train_shard_decode_f32(ctx, pre, b_enc, y_row_ptr, y_col, y_val, W_enc_loc, W_dec_loc,
                                      b_dec_loc, col_lo, col_hi, H, B, n_batch, tied, kp, seed,
                                      reg_lambda, gW_out, gb_dec_loc, dh_partial, cost_partial);
}

int dae_train_shard_finish(dae_ctx* ctx, const float* dh,
        const int32_t* x_row_ptr, const int32_t* x_col, const float* x_val,
        const float* W_enc_loc, const float* b_enc, const float* W_dec_loc, const float* b_dec_loc,
        int col_lo, int col_hi, int H, int B, int tied,
        float ikp, float kp, uint32_t seed, float reg_lambda,
        float* gW_enc_loc, float* gb_enc, float* gW_dec_loc, float* gb_dec_loc)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!dh || !x_row_ptr || !W_enc_loc || !b_enc || !b_dec_loc || !gW_enc_loc || !gb_enc || !gb_dec_loc)
        return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (!tied && (!W_dec_loc || !gW_dec_loc)) return dae_fail(ctx, DAE_ERR_ARG, "untied model needs W_dec_loc and gW_dec_loc");
    int rc = check_shard(ctx, col_lo, col_hi, H, B, ikp, kp);
    if (rc) return rc;
    return dae_train_shard_finish_f32(ctx, dh, x_row_ptr, x_col, x_val, W_enc_loc, b_enc, W_dec_loc,
                                      b_dec_loc, col_lo, col_hi, H, B, tied, ikp, kp, seed, reg_lambda,
                                      gW_enc_loc, gb_enc, gW_dec_loc, gb_dec_loc);
}

int dae_title_features(dae_ctx* ctx, const int32_t* titles, int B, int L, const float* emb, int n_char, int E,
                       const float* conv_w, const float* conv_b, const int32_t* filter_sizes, int n_sizes, int F,
                       float keep_prob, uint32_t seed, float* feat, int64_t ld, int32_t* argmax, float* feat_raw)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!titles || !emb || !conv_w || !conv_b || !filter_sizes || !feat) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (B <= 0) return DAE_OK;
    if (n_char < 1 || F < 1) return dae_fail(ctx, DAE_ERR_ARG, "bad shape");
    if (!(keep_prob > 0.f && keep_prob <= 1.f)) return dae_fail(ctx, DAE_ERR_ARG, "keep probability must be in (0,1]");
    return dae_launch_title_features(ctx, titles, B, L, emb, n_char, E, conv_w, conv_b, filter_sizes, n_sizes, F,
                                     keep_prob, seed, feat, ld, argmax, feat_raw);
}

int dae_title_prepack_features(dae_ctx* ctx, const float* emb, int n_char, int E, const float* conv_w,
                               const int32_t* filter_sizes, int n_sizes, int F)
{
    if (!ctx) return DAE_ERR_ARG;
    if (emb && (!conv_w || !filter_sizes)) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    return dae_launch_title_table(ctx, emb, n_char, E, conv_w, filter_sizes, n_sizes, F);
}

int dae_mix_scores(dae_ctx* ctx, const float* title_score, int64_t ld_title, float* dae_score, int64_t ld_dae,
                   const float* w_title, const float* w_playlist, int B, int ncols)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!title_score || !dae_score || !w_title || !w_playlist) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (B <= 0 || ncols <= 0) return DAE_OK;
    if (ld_title < ncols || ld_dae < ncols) return dae_fail(ctx, DAE_ERR_ARG, "leading dimension < %d columns", ncols);
    return dae_launch_mix_scores(ctx, title_score, ld_title, dae_score, ld_dae, w_title, w_playlist, B, ncols);
}

int dae_row_sums(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val, int B,
                 float input_keep_prob, uint32_t seed, float* out)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!row_ptr || !out) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (B <= 0) return DAE_OK;
    if (!(input_keep_prob > 0.f && input_keep_prob <= 1.f)) return dae_fail(ctx, DAE_ERR_ARG, "keep probability must be in (0,1]");
    return dae_launch_row_sums(ctx, row_ptr, col, val, B, input_keep_prob, seed, out);
}

int dae_mix_weights(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val, int B, float input_keep_prob,
                    uint32_t seed, const float* titles_use, float* w_title, float* w_playlist)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!row_ptr || !titles_use || !w_title || !w_playlist) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (B <= 0) return DAE_OK;
    if (!(input_keep_prob > 0.f && input_keep_prob <= 1.f)) return dae_fail(ctx, DAE_ERR_ARG, "keep probability must be in (0,1]");
    return dae_launch_mix_weights(ctx, row_ptr, col, val, B, input_keep_prob, seed, titles_use, w_title, w_playlist);
}

int dae_title_loss_backward(dae_ctx* ctx, const float* title_logits, int64_t ld_z, const float* dae_score, int64_t ld_d,
                            const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
                            const float* w_title, const float* w_playlist, int B, int V, int n_batch,
                            const float* feat, int ld, const float* Output_WT, float* gOutput_WT, float* gOutput_b,
                            float* dfeat, float* cost_out)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!title_logits || !dae_score || !y_row_ptr || !w_title || !w_playlist || !feat || !Output_WT || !gOutput_WT ||
        !gOutput_b || !dfeat || !cost_out)
        return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (B <= 0 || V <= 0 || n_batch <= 0 || ld_z < V || ld_d < V) return dae_fail(ctx, DAE_ERR_ARG, "bad shape");
    return dae_launch_title_loss_backward(ctx, title_logits, ld_z, dae_score, ld_d, y_row_ptr, y_col, y_val, w_title,
                                          w_playlist, B, V, n_batch, feat, ld, Output_WT, gOutput_WT, gOutput_b,
                                          dfeat, cost_out);
}

int dae_title_loss_backward_cols(dae_ctx* ctx, const float* title_logits, int64_t ld_z, const float* dae_score, int64_t ld_d,
                                 const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
                                 const float* w_title, const float* w_playlist, int B, int col_lo, int col_hi, int n_batch,
                                 const float* feat, int ld, const float* Output_WT_rows, float* gOutput_WT_rows,
                                 float* gOutput_b_rows, float* dfeat_partial, float* cost_partial)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!title_logits || !dae_score || !y_row_ptr || !w_title || !w_playlist || !feat || !Output_WT_rows || !gOutput_WT_rows ||
        !gOutput_b_rows || !dfeat_partial || !cost_partial)
        return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (col_lo < 0 || col_hi <= col_lo) return dae_fail(ctx, DAE_ERR_ARG, "column window [%d, %d) is empty or negative", col_lo, col_hi);
    if (B < 1 || B > 256) return dae_fail(ctx, DAE_ERR_ARG, "B=%d outside [1, 256]", B);
    if (ld < 32 || (ld % 32) != 0) return dae_fail(ctx, DAE_ERR_ARG, "ld=%d is no multiple of 32", ld);
    const int V = col_hi - col_lo;
    if (n_batch <= 0 || ld_z < V || ld_d < V) return dae_fail(ctx, DAE_ERR_ARG, "bad shape");
    return dae_launch_title_loss_backward_cols(ctx, title_logits, ld_z, dae_score, ld_d, y_row_ptr, y_col, y_val, w_title,
                                               w_playlist, B, col_lo, col_hi, n_batch, feat, ld, Output_WT_rows,
                                               gOutput_WT_rows, gOutput_b_rows, dfeat_partial, cost_partial);
}

int dae_title_conv_backward(dae_ctx* ctx, const int32_t* titles, int B, int L, const float* emb, int n_char, int E,
                            const float* conv_w, const int32_t* filter_sizes, int n_sizes, int F,
                            const int32_t* argmax, const float* feat_raw, const float* dfeat, int64_t ld,
                            float keep_prob, uint32_t seed, float* g_emb, float* g_conv_w, float* g_conv_b)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!titles || !emb || !conv_w || !filter_sizes || !argmax || !feat_raw || !dfeat || !g_emb || !g_conv_w || !g_conv_b)
        return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (B <= 0) return DAE_OK;
    if (!(keep_prob > 0.f && keep_prob <= 1.f)) return dae_fail(ctx, DAE_ERR_ARG, "keep probability must be in (0,1]");
    return dae_launch_title_conv_backward(ctx, titles, B, L, emb, n_char, E, conv_w, filter_sizes, n_sizes, F, argmax,
                                          feat_raw, dfeat, ld, keep_prob, seed, g_emb, g_conv_w, g_conv_b);
}

int dae_set_overlap_hint(dae_ctx* ctx, int batches_in_flight)
{
    if (!ctx) return DAE_ERR_ARG;
    ctx->overlap_hint = batches_in_flight > 1 ? 1 : 0;
    return DAE_OK;
}

int dae_set_decode_gate(dae_ctx* ctx, void* wait_event, void* record_event)
{
    if (!ctx) return DAE_ERR_ARG;
    ctx->gate_wait = static_cast<hipEvent_t>(wait_event);
    ctx->gate_record = static_cast<hipEvent_t>(record_event);
    return DAE_OK;
}

int dae_set_enc_grad_prezeroed(dae_ctx* ctx, int on)
{
    if (!ctx) return DAE_ERR_ARG;
    ctx->enc_grad_prezeroed = on ? 1 : 0;
    return DAE_OK;
}

}  // extern "C"
