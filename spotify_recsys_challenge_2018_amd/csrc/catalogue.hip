// catalogue.hip -- rank a SHARED subset of the track columns: "the k best tracks among THESE columns, the same for every row" (a
// market's catalogue, the tracks still licensed, a second generator's pool) at the cost of a ranking over those n columns, not V.
//
// A dae_catalogue is an ascending list of n global track columns, cols[0 .. n), and its inverse local_of[n_tracks] (-1 = not in
// the catalogue).  dae_prepack_decoder_catalogue gathers rows cols[.] of the caller's decoder into an image whose columns are the
// LOCAL ones, [0, n) -- the image the existing fused path already ranks.  A catalogue call is that path between three launches of
// its own:
//   a. cat_seed_count_kernel + cat_seed_compact_kernel: the seed CSR (global columns) -> the seeds that lie in the catalogue, as
//      local columns, in order, with fresh row pointers (seeds outside it cannot be ranked: dropping them keeps the thresholds'
//      k + n_seeds tight);
//   b. dae_score_topk / dae_decode_topk / dae_title_rank on the image with n_tracks = n -- unchanged kernels, plans and limits;
//   c. cat_map_back_kernel: out_idx through cols, in place (-1 stays -1).
// ASCENDING ORDER is what makes this the whole story: local order equals global order, so the canonical tie-break (key descending,
// column ascending) ranks the same way in both spaces, and a sorted unique seed row stays sorted and unique.  A logit depends on its
// own decoder row and the hidden row only, and every kernel runs the canonical chain per element: the bits are the full image's.
#include <atomic>
#include <climits>

#include "dae_internal.h"

struct dae_catalogue {
    int device = 0;
    int n = 0, n_tracks = 0;
    int32_t* cols = nullptr;           // [n] the catalogue's columns, ascending (a copy: the caller's list may go)
    int32_t* local_of = nullptr;       // [n_tracks] position in cols, -1 = not in the catalogue
    uint64_t id = 0;                   // process-wide, never 0: what an image gathered from it records (dae_packed::cat_id)
};

namespace {

std::atomic<uint64_t> g_next_cat_id{1};

constexpr int CAT_SLAB = 4096;         // rows of one translation (score.hip DAE_ROW_SLAB: a scoring slab)
constexpr size_t CAT_RP_INTS = 4160;   // dae_ctx::cat_seeds in ints: [CAT_SLAB + 1] row pointers, padded | [CAT_SLAB] counts | the columns
constexpr size_t CAT_HEAD_INTS = CAT_RP_INTS + CAT_SLAB;

__device__ __forceinline__ int cat_wave_sum(int v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// validate cols[0 .. n) (strictly ascending, inside [0, n_tracks)) and scatter the inverse table (pre-filled with -1).
// *first_bad (pre-set to INT_MAX) = the smallest offending position.  A column id is tested before an address is formed from it.
__global__ __launch_bounds__(256) void cat_build_kernel(const int32_t* __restrict__ cols, int n, int n_tracks,
                                                        int32_t* __restrict__ local_of, int* __restrict__ first_bad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = cols[i];
    const bool in_range = (unsigned)c < (unsigned)n_tracks;
    if (!in_range || (i > 0 && cols[i - 1] >= c)) atomicMin(first_bad, i);
    if (in_range) local_of[c] = i;     // (a duplicate races here: such a list is refused and the table discarded)
}

// Wg[i][:] = W[cols[i]][:], bg[i] = b[cols[i]] -- a wave per catalogue row; a column outside [0, V) gathers zeros
__global__ __launch_bounds__(256) void cat_gather_kernel(const float* __restrict__ W, const float* __restrict__ b, int V, int H,
                                                         const int32_t* __restrict__ cols, int n, float* __restrict__ Wg,
                                                         float* __restrict__ bg)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const int c = cols[i];
    const bool ok = (unsigned)c < (unsigned)V;
    const float* src = W + (ok ? (size_t)c * H : 0);
    float* dst = Wg + (size_t)i * H;
    for (int k = lane; k < H; k += 64) dst[k] = ok ? src[k] : 0.0f;
    if (lane == 0) bg[i] = ok ? b[c] : 0.0f;
}

// a. part one: cnt[row] = seeds of the row that lie in the catalogue (a wave per row)
__global__ __launch_bounds__(256) void cat_seed_count_kernel(const int32_t* __restrict__ srp, const int32_t* __restrict__ sc, int B,
                                                             const int32_t* __restrict__ local_of, int n_tracks,
                                                             int* __restrict__ cnt)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    const int lo = srp[row], hi = srp[row + 1];
    int m = 0;
    for (int i = lo + lane; i < hi; i += 64) {
        const int c = sc[i];
        if ((unsigned)c < (unsigned)n_tracks && local_of[c] >= 0) ++m;
    }
    m = cat_wave_sum(m);
    if (lane == 0) cnt[row] = m;
}

// a. part two: the row's offset = the sum of the counts before it (B <= CAT_SLAB: 64 lanes x 64 counts at the most), then its
// kept seeds as local columns, in order; nothing is written at or past cap
__global__ __launch_bounds__(256) void cat_seed_compact_kernel(const int32_t* __restrict__ srp, const int32_t* __restrict__ sc, int B,
                                                               const int32_t* __restrict__ local_of, int n_tracks,
                                                               const int* __restrict__ cnt, int32_t* __restrict__ rp_out,
                                                               int32_t* __restrict__ sc_out, int cap)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    int off = 0;
    for (int r = lane; r < row; r += 64) off += cnt[r];
    off = cat_wave_sum(off);
    if (lane == 0) {
        rp_out[row] = off;
        if (row == B - 1) rp_out[B] = off + cnt[row];
    }
    const int lo = srp[row], hi = srp[row + 1];
    for (int i0 = lo; i0 < hi; i0 += 64) {                     // (wave-uniform trip count: the ballot sees every lane)
        const int i = i0 + lane;
        int l = -1;
        if (i < hi) {
            const int c = sc[i];
            if ((unsigned)c < (unsigned)n_tracks) l = local_of[c];
        }
        const unsigned long long kept = __ballot(l >= 0);
        const int pos = off + __popcll(kept & ((1ull << lane) - 1ull));
        if (l >= 0 && pos < cap) sc_out[pos] = l;
        off += __popcll(kept);
    }
}

// c. local column -> global column, in place; -1 (and anything else outside [0, n)) -> -1
__global__ __launch_bounds__(256) void cat_map_back_kernel(int32_t* __restrict__ idx, size_t total, const int32_t* __restrict__ cols, int n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int l = idx[i];
    idx[i] = (unsigned)l < (unsigned)n ? cols[l] : -1;
}

dae_packed& slot_of(dae_ctx* ctx, int dtype) { return dtype == DAE_DTYPE_F32 ? ctx->pk_f32 : ctx->pk_bf16; }

// the context's image of `dtype` was gathered from `cat` (err: the context that takes the message)
int check_image(dae_ctx* err, dae_ctx* ctx, const dae_catalogue* cat, int dtype, const char* which)
{
    const dae_packed& pk = slot_of(ctx, dtype);
    if (!pk.valid || pk.cat_id != cat->id || (dtype == DAE_DTYPE_BF16_EXACT && !pk.exact))
        return dae_fail(err, DAE_ERR_STATE, "%s image of dtype %d was not built from this catalogue (dae_prepack_decoder_catalogue)",
                        which, dtype);
    if (pk.col_lo != 0 || pk.col_hi != cat->n)
        return dae_fail(err, DAE_ERR_STATE, "%s image holds columns [%d, %d), the catalogue has %d", which, pk.col_lo, pk.col_hi, cat->n);
    return DAE_OK;
}

// the underlying call's own refusals, here so that they come before the translation launches, then the catalogue's
int check_rank_args(dae_ctx* ctx, const dae_catalogue* cat, int dtype, int k, const int32_t* seed_row_ptr, const int32_t* seed_col,
                    int n_seeds, const void* out_score, const void* out_idx)
{
    if (!cat) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    const int rc = dae_check_topk_args(ctx, dtype, k, seed_row_ptr, seed_col, out_score, out_idx);
    if (rc) return rc;
    if (n_seeds < 0) return dae_fail(ctx, DAE_ERR_ARG, "n_seeds=%d", n_seeds);
    if (cat->device != ctx->device) return dae_fail(ctx, DAE_ERR_ARG, "the catalogue lives on device %d, the context on %d", cat->device, ctx->device);
    return check_image(ctx, ctx, cat, dtype, "the context's");
}

int reserve_seeds(dae_ctx* ctx, int cap)
{
    return dae_reserve(ctx, ctx->cat_seeds, (CAT_HEAD_INTS + (size_t)(cap > 0 ? cap : 1)) * sizeof(int32_t));
}

// a. into buffers the caller owns: rp [B + 1], cnt [B], out [cap] (the pipeline's launch slots; the offsets' sum in
// cat_seed_compact_kernel walks the counts before the row, whatever B is)
int translate_seeds_into(dae_ctx* ctx, const dae_catalogue* cat, const int32_t* srp, const int32_t* sc, int B, int cap, int32_t* rp,
                         int* cnt, int32_t* out)
{
    const dim3 grid((B + 3) / 4), block(256);
    hipLaunchKernelGGL(cat_seed_count_kernel, grid, block, 0, ctx->stream, srp, sc, B, cat->local_of, cat->n_tracks, cnt);
    DAE_CHECK_LAUNCH(ctx, "cat_seed_count_kernel");
    hipLaunchKernelGGL(cat_seed_compact_kernel, grid, block, 0, ctx->stream, srp, sc, B, cat->local_of, cat->n_tracks, cnt, rp, out, cap);
    DAE_CHECK_LAUNCH(ctx, "cat_seed_compact_kernel");
    return DAE_OK;
}

// a.: rows [0, B) of the seed CSR (srp holds absolute offsets into sc) -> ctx->cat_seeds; B <= CAT_SLAB, reserve_seeds(cap) done
int translate_seeds(dae_ctx* ctx, const dae_catalogue* cat, const int32_t* srp, const int32_t* sc, int B, int cap,
                    const int32_t** srp_out, const int32_t** sc_out)
{
    int32_t* rp = static_cast<int32_t*>(ctx->cat_seeds.p);
    int* cnt = rp + CAT_RP_INTS;
    int32_t* out = rp + CAT_HEAD_INTS;
    const int rc = translate_seeds_into(ctx, cat, srp, sc, B, cap, rp, cnt, out);
    if (rc) return rc;
    *srp_out = rp; *sc_out = out;
    return DAE_OK;
}

int map_back(dae_ctx* ctx, const dae_catalogue* cat, int32_t* idx, size_t total)
{
    if (total == 0) return DAE_OK;
    hipLaunchKernelGGL(cat_map_back_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, idx, total, cat->cols, cat->n);
    DAE_CHECK_LAUNCH(ctx, "cat_map_back_kernel");
    return DAE_OK;
}

// the slabs of a catalogue ranking call: translate, rank(r0, nb, local seeds, outputs of the slab), map back
template <class Rank>
int rank_slabs(dae_ctx* ctx, const dae_catalogue* cat, int B, int k, const int32_t* seed_row_ptr, const int32_t* seed_col, int n_seeds,
               float* out_score, int32_t* out_idx, Rank&& rank)
{
    int rc = seed_row_ptr ? reserve_seeds(ctx, n_seeds) : DAE_OK;
    if (rc) return rc;
    for (int r0 = 0; r0 < B; r0 += CAT_SLAB) {
        const int nb = B - r0 < CAT_SLAB ? B - r0 : CAT_SLAB;
        const int32_t* srp = nullptr; const int32_t* sc = nullptr;
        if (seed_row_ptr) {
            rc = translate_seeds(ctx, cat, seed_row_ptr + r0, seed_col, nb, n_seeds, &srp, &sc);
            if (rc) return rc;
        }
        int32_t* oi = out_idx + (size_t)r0 * k;
        rc = rank(r0, nb, srp, sc, out_score + (size_t)r0 * k, oi);
        if (rc) return rc;
        rc = map_back(ctx, cat, oi, (size_t)nb * k);
        if (rc) return rc;
    }
    return DAE_OK;
}

}  // namespace

// ---- what the pipeline needs of a catalogue (dae_internal.h): the translation on ITS prep stream into ITS slot's buffers, then
// the ranking calls with the local seed lists ready ----------------------------------------------------------------------------
void dae_catalogue_shape(const dae_catalogue* cat, int* device, int* n, int* n_tracks)
{
    *device = cat->device; *n = cat->n; *n_tracks = cat->n_tracks;
}

int dae_catalogue_translate_seeds(dae_ctx* ctx, const dae_catalogue* cat, const int32_t* srp, const int32_t* sc, int B, int cap,
                                  int32_t* rp_out, int32_t* cnt, int32_t* sc_out)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!cat || !srp || !sc || !rp_out || !cnt || !sc_out) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (B < 1 || cap < 0) return dae_fail(ctx, DAE_ERR_ARG, "dae_catalogue_translate_seeds: B=%d cap=%d", B, cap);
    return translate_seeds_into(ctx, cat, srp, sc, B, cap, rp_out, cnt, sc_out);
}

// dae_score_topk_catalogue behind a translation that has run already: local_srp / local_sc are the image's columns (any B: the
// seeds' row pointers are absolute, dae_score_topk walks its own slabs), one map-back over the call's lists
int dae_score_topk_catalogue_local(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val, const float* W_enc,
                                   const float* b_enc, int V, int H, int B, int dtype, const dae_catalogue* cat,
                                   const int32_t* local_srp, const int32_t* local_sc, int k, int out_kind, float* out_score,
                                   int32_t* out_idx)
{
    if (!ctx) return DAE_ERR_ARG;
    int rc = check_rank_args(ctx, cat, dtype, k, local_srp, local_sc, 0, out_score, out_idx);
    if (rc) return rc;
    if (H != slot_of(ctx, dtype).H) return dae_fail(ctx, DAE_ERR_ARG, "H=%d does not match prepacked H=%d", H, slot_of(ctx, dtype).H);
    if (B <= 0) return DAE_OK;
    rc = dae_score_topk(ctx, row_ptr, col, val, W_enc, b_enc, V, H, B, dtype, cat->n, local_srp, local_sc, k, out_kind, out_score, out_idx);
    if (rc) return rc;
    return map_back(ctx, cat, out_idx, (size_t)B * k);
}

// the titled ranking inside a catalogue, between the seed translation and the end of the call: both contexts' images are the
// catalogue's, b.srp / b.sc hold LOCAL columns; the mix term and the ranking over the n local columns (both images end at column
// n), then the map-back.  dae_title_score_catalogue and the pipeline's titled launches both end here.
int dae_title_rank_catalogue(dae_ctx* tc, dae_ctx* dc, int dtype, int B, int H, int ld_feat, const dae_title_bufs& b,
                             const dae_catalogue* cat, int k, float* out_score, int32_t* out_idx, int32_t* guard_out)
{
    int rc = check_image(tc, dc, cat, dtype, "the DAE context's");
    if (rc) return rc;
    rc = check_image(tc, tc, cat, dtype, "the title context's");
    if (rc) return rc;
    rc = dae_title_rank(tc, dc, dtype, B, cat->n, H, ld_feat, b, cat->n, k, out_score, out_idx, guard_out);
    if (rc) return rc;
    return map_back(tc, cat, out_idx, (size_t)B * k);
}

extern "C" {

int dae_catalogue_create(dae_ctx* ctx, const int32_t* cols, int n, int n_tracks, dae_catalogue** out)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!cols || !out) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (n_tracks < 1 || n < 1 || n > n_tracks)
        return dae_fail(ctx, DAE_ERR_ARG, "dae_catalogue_create: n=%d columns of n_tracks=%d (1 <= n <= n_tracks)", n, n_tracks);
    int32_t* block = nullptr;                                  // cols copy | local_of | the status word
    const size_t n_pad = ((size_t)n + 63) & ~(size_t)63;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&block), (n_pad + (size_t)n_tracks + 1) * sizeof(int32_t));
    if (e != hipSuccess) return dae_fail(ctx, DAE_ERR_NOMEM, "dae_catalogue_create: hipMalloc failed: %s", hipGetErrorString(e));
    int32_t* d_cols = block;
    int32_t* d_local = block + n_pad;
    int* d_bad = d_local + n_tracks;
    int first_bad = INT_MAX;
    int32_t at[2] = {0, 0};
    auto enqueue = [&]() -> hipError_t {
        hipError_t x = hipMemcpyAsync(d_cols, cols, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream);
        if (x != hipSuccess) return x;
        x = hipMemsetAsync(d_local, 0xFF, (size_t)n_tracks * sizeof(int32_t), ctx->stream);      // -1 everywhere
        if (x != hipSuccess) return x;
        x = hipMemcpyAsync(d_bad, &first_bad, sizeof(int), hipMemcpyHostToDevice, ctx->stream);
        if (x != hipSuccess) return x;
        hipLaunchKernelGGL(cat_build_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_cols, n, n_tracks, d_local, d_bad);
        x = hipGetLastError();
        if (x != hipSuccess) return x;
        x = hipMemcpyAsync(&first_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);       // the one word read back
        if (x != hipSuccess) return x;
        x = hipStreamSynchronize(ctx->stream);
        if (x != hipSuccess || first_bad == INT_MAX) return x;
        // refused: the offender and its predecessor, for the message
        const int from = first_bad > 0 ? first_bad - 1 : 0;
        x = hipMemcpyAsync(at, d_cols + from, (size_t)(first_bad - from + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
        return x != hipSuccess ? x : hipStreamSynchronize(ctx->stream);
    };
    e = enqueue();
    if (e != hipSuccess || first_bad != INT_MAX) {
        (void)hipFree(block);
        if (e != hipSuccess) return dae_fail(ctx, DAE_ERR_HIP, "dae_catalogue_create: %s", hipGetErrorString(e));
        const int c = first_bad > 0 ? at[1] : at[0];
        if (c < 0 || c >= n_tracks)
            return dae_fail(ctx, DAE_ERR_ARG, "dae_catalogue_create: cols[%d] = %d is outside the track columns [0, %d)", first_bad, c, n_tracks);
        return dae_fail(ctx, DAE_ERR_ARG, "dae_catalogue_create: cols[%d] = %d does not ascend (cols[%d] = %d): the list is strictly "
                        "ascending, each column once", first_bad, c, first_bad - 1, at[0]);
    }
    dae_catalogue* cat = new dae_catalogue();
    cat->device = ctx->device; cat->n = n; cat->n_tracks = n_tracks;
    cat->cols = d_cols; cat->local_of = d_local;
    cat->id = g_next_cat_id.fetch_add(1);
    *out = cat;
    return DAE_OK;
}

int dae_catalogue_destroy(dae_catalogue* cat)
{
    if (!cat) return DAE_OK;
    (void)hipSetDevice(cat->device);
    (void)hipDeviceSynchronize();                              // (calls in flight on any context still read the tables)
    (void)hipFree(cat->cols);                                  // one allocation: cols | local_of | status
    delete cat;
    return DAE_OK;
}

int dae_prepack_decoder_catalogue(dae_ctx* ctx, const dae_catalogue* cat, const float* W_dec, const float* b_dec, int V, int H, int dtype)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!cat || !W_dec || !b_dec) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (!dae_known_dtype(dtype)) return dae_fail(ctx, DAE_ERR_ARG, "unknown dtype %d", dtype);
    if (cat->device != ctx->device) return dae_fail(ctx, DAE_ERR_ARG, "the catalogue lives on device %d, the context on %d", cat->device, ctx->device);
    if (H <= 0 || V < cat->n_tracks)
        return dae_fail(ctx, DAE_ERR_ARG, "bad shape V=%d H=%d for a catalogue over %d track columns", V, H, cat->n_tracks);
    // the gathered rows [n][H] | biases [n]: a temporary of this call, gone when it returns (the image keeps what it needs)
    const size_t w_bytes = ((size_t)cat->n * H * sizeof(float) + 255) & ~(size_t)255;
    float* Wg = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&Wg), w_bytes + (size_t)cat->n * sizeof(float));
    if (e != hipSuccess) return dae_fail(ctx, DAE_ERR_NOMEM, "dae_prepack_decoder_catalogue: hipMalloc failed: %s", hipGetErrorString(e));
    float* bg = reinterpret_cast<float*>(reinterpret_cast<char*>(Wg) + w_bytes);
    hipLaunchKernelGGL(cat_gather_kernel, dim3((cat->n + 3) / 4), dim3(256), 0, ctx->stream, W_dec, b_dec, V, H, cat->cols, cat->n, Wg, bg);
    e = hipGetLastError();
    int rc = e == hipSuccess ? dae_prepack_decoder(ctx, Wg, bg, cat->n, H, 0, cat->n, dtype)
                             : dae_fail(ctx, DAE_ERR_HIP, "launch of cat_gather_kernel failed: %s", hipGetErrorString(e));
    e = hipStreamSynchronize(ctx->stream);                     // the prepack launches read the temporary
    (void)hipFree(Wg);
    if (rc) return rc;
    if (e != hipSuccess) {
        slot_of(ctx, dtype).valid = false;
        return dae_fail(ctx, DAE_ERR_HIP, "dae_prepack_decoder_catalogue: %s", hipGetErrorString(e));
    }
    slot_of(ctx, dtype).cat_id = cat->id;
    return DAE_OK;
}

int dae_score_topk_catalogue(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val, const float* W_enc,
                             const float* b_enc, int V, int H, int B, int dtype, const dae_catalogue* cat,
                             const int32_t* seed_row_ptr, const int32_t* seed_col, int n_seeds, int k, int out_kind,
                             float* out_score, int32_t* out_idx)
{
    if (!ctx) return DAE_ERR_ARG;
    int rc = check_rank_args(ctx, cat, dtype, k, seed_row_ptr, seed_col, n_seeds, out_score, out_idx);
    if (rc) return rc;
    if (!row_ptr || !W_enc || !b_enc) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (H != slot_of(ctx, dtype).H) return dae_fail(ctx, DAE_ERR_ARG, "H=%d does not match prepacked H=%d", H, slot_of(ctx, dtype).H);
    if (H <= 0 || (H % 4) != 0) return dae_fail(ctx, DAE_ERR_ARG, "H=%d must be a positive multiple of 4", H);
    if ((reinterpret_cast<uintptr_t>(W_enc) | reinterpret_cast<uintptr_t>(b_enc)) % 16)
        return dae_fail(ctx, DAE_ERR_ARG, "W_enc, b_enc must be 16-byte aligned");
    return rank_slabs(ctx, cat, B, k, seed_row_ptr, seed_col, n_seeds, out_score, out_idx,
                      [&](int r0, int nb, const int32_t* srp, const int32_t* sc, float* os, int32_t* oi) {
        return dae_score_topk(ctx, row_ptr + r0, col, val, W_enc, b_enc, V, H, nb, dtype, cat->n, srp, sc, k, out_kind, os, oi);
    });
}

int dae_decode_topk_catalogue(dae_ctx* ctx, const float* h, int B, int H, int dtype, const dae_catalogue* cat,
                              const int32_t* seed_row_ptr, const int32_t* seed_col, int n_seeds, int k, int out_kind,
                              float* out_score, int32_t* out_idx)
{
    if (!ctx) return DAE_ERR_ARG;
    int rc = check_rank_args(ctx, cat, dtype, k, seed_row_ptr, seed_col, n_seeds, out_score, out_idx);
    if (rc) return rc;
    if (!h) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (H != slot_of(ctx, dtype).H) return dae_fail(ctx, DAE_ERR_ARG, "H=%d does not match prepacked H=%d", H, slot_of(ctx, dtype).H);
    return rank_slabs(ctx, cat, B, k, seed_row_ptr, seed_col, n_seeds, out_score, out_idx,
                      [&](int r0, int nb, const int32_t* srp, const int32_t* sc, float* os, int32_t* oi) {
        return dae_decode_topk(ctx, h + (size_t)r0 * H, nb, H, dtype, cat->n, srp, sc, k, out_kind, os, oi);
    });
}

int dae_title_score_catalogue(dae_ctx* tc, dae_ctx* dc, int dtype, const int64_t* positions, const float* values, int values_broadcast,
                              int64_t nnz, int n_rows, int V, const float* W_enc, const float* b_enc, int H,
                              const int32_t* titles, int L, const float* emb, int n_char, int E, const float* conv_w,
                              const float* conv_b, const int32_t* filter_sizes, int n_sizes, int F, int ld_feat,
                              const float* titles_use, int n_tracks, int k, float* out_score, int32_t* out_idx,
                              int32_t* guard_out, int32_t* csr_status, const dae_catalogue* cat)
{
    if (!tc) return DAE_ERR_ARG;
    if (!dc || dc == tc) return dae_fail(tc, DAE_ERR_ARG, "dae_title_score_catalogue: needs the DAE's context");
    if (!dae_known_dtype(dtype)) return dae_fail(tc, DAE_ERR_ARG, "unknown dtype %d", dtype);
    if (dtype == DAE_DTYPE_BF16_EXACT)
        return dae_fail(tc, DAE_ERR_ARG, "dae_title_score_catalogue: DAE_DTYPE_BF16_EXACT is not available inside a catalogue; "
                        "DAE_DTYPE_F32 returns the same lists");
    if (k < 1 || k > DAE_MAX_K) return dae_fail(tc, DAE_ERR_ARG, "k=%d out of [1,%d] (titled scoring)", k, DAE_MAX_K);
    if (!cat || !titles || !titles_use || !W_enc || !b_enc || !csr_status || !out_score || !out_idx || (nnz > 0 && (!positions || !values)))
        return dae_fail(tc, DAE_ERR_ARG, "null pointer");
    if (nnz < 0 || nnz >= (int64_t)1 << 31 || V < 1 || H < 1 || ld_feat < n_sizes * F) return dae_fail(tc, DAE_ERR_ARG, "bad shape");
    if (n_rows > CAT_SLAB) return dae_fail(tc, DAE_ERR_ARG, "dae_title_score_catalogue takes at most %d rows (n_rows=%d)", CAT_SLAB, n_rows);
    if (n_tracks != cat->n_tracks)
        return dae_fail(tc, DAE_ERR_ARG, "n_tracks=%d, the catalogue was created over %d track columns", n_tracks, cat->n_tracks);
    if (cat->device != tc->device || dc->device != tc->device) return dae_fail(tc, DAE_ERR_ARG, "contexts and catalogue on different devices");
    if (dc->stream != tc->stream) return dae_fail(tc, DAE_ERR_STATE, "both contexts must be bound to the same stream");
    if (tc->mixT) return dae_fail(tc, DAE_ERR_STATE, "dae_title_score_catalogue sets the score mix itself: clear dae_set_score_mix");
    int rc = check_image(tc, dc, cat, dtype, "the DAE context's");
    if (rc) return rc;
    rc = check_image(tc, tc, cat, dtype, "the title context's");
    if (rc) return rc;
    if (n_rows <= 0) return DAE_OK;
    const int B = n_rows;
    dae_title_bufs b;
    rc = dae_title_bufs_reserve(tc, nnz, B, H, ld_feat, b);
    if (rc) return rc;
    const int cap = (int)(nnz > 0 ? nnz : 1);                  // (room of b.sc: the seeds are the feed's own track columns)
    rc = reserve_seeds(tc, cap);
    if (rc) return rc;
    // the feed's global columns all the way: CSR, the seed lists (columns < n_tracks), hidden rows, mixing weights, features
    rc = dae_title_prepare(tc, dc, positions, values, values_broadcast, nnz, B, V, W_enc, b_enc, H, titles, L, emb, n_char, E, conv_w,
                           conv_b, filter_sizes, n_sizes, F, ld_feat, titles_use, n_tracks, b, csr_status);
    if (rc) return rc;
    const int32_t* srp = nullptr; const int32_t* sc = nullptr;
    rc = translate_seeds(tc, cat, b.srp, b.sc, B, cap, &srp, &sc);
    if (rc) return rc;
    b.srp = const_cast<int32_t*>(srp); b.sc = const_cast<int32_t*>(sc);
    return dae_title_rank_catalogue(tc, dc, dtype, B, H, ld_feat, b, cat, k, out_score, out_idx, guard_out);
}

}  // extern "C"
