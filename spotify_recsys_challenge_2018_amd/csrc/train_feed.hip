// train_feed.hip -- the training feed built on the device (include/dae_hip.h dae_train_set_* / dae_train_batch).
// The training set never changes: its playlists live on the device as the reader's flat arrays (ids + offsets per side),
// and a batch is named by the reader's DRAWS alone -- 12 bytes a row: which playlist, how many leading tracks / artists
// carry the value 1 (utils/data_reader.py next_batch_draw).  Both CSRs of a step come out of two launches, entry for entry
// what dae_coo_to_csr makes of the COO the reader's next_batch returns for the same draws:
//   feed_row_kernel      one wave per row: per side, last-wins dedup and the rank of every kept entry by counting
//                        (csr.hip's per-row step, without the bucket sort in front of it: a row IS a playlist)
//   feed_compact_kernel  one workgroup per row: output offset = the kept counts of the rows before it, summed here
//                        (csr_compact_sum_kernel's scheme: no scan launch), then a copy; the last row's workgroup writes
//                        the status word
//   feed_titles_kernel   dae_train_titles: one wave per row copies the drawn playlists' title rows out of the set
//                        (dae_train_set_attach_titles: the reader's [n_playlists][L] character ids, copied once)
// No memset, no atomics on global memory.  Integer work bound by latency and launch count, not by any rate.
#include "dae_internal.h"
#include "train_feed_check.h"

struct dae_train_set {
    int device = 0;
    void* block = nullptr;             // one allocation: trk_off | art_off | trk | art
    const int64_t* trk_off = nullptr;
    const int64_t* art_off = nullptr;
    const int32_t* trk = nullptr;
    const int32_t* art = nullptr;
    int n_playlists = 0, n_tracks = 0, n_items = 0;
    dae_train_set_shape shape;
    int32_t* titles = nullptr;         // dae_train_set_attach_titles: [n_playlists][title_len], an allocation of its own
    int title_len = 0;
};

namespace {

constexpr int FEED_SIDE_CAP = 512;     // entries of one side ranked inside LDS: 2.5 KB per row (csr_row_kernel<512, 64>'s budget)

// One wave per batch row.  Entry i of a side is y-KEPT iff no later entry of the side has the same id (the LAST position
// wins; y's values are all 1), and x-KEPT iff it is y-kept, the side is fed to x, and i < lim (its value is 1: zeros are
// dropped after the duplicate rule, so an id whose last position carries 0 leaves x altogether).  A kept entry's slot is the
// number of kept entries of the side with a smaller id; artists follow tracks (every track id is below every artist id).
// Kept ids go to yk / xk at row * stride (stride = the longest playlist of the set), their numbers to ycnt / xcnt.
// Sides longer than FEED_SIDE_CAP take the same steps over global memory, their flags in `tmp` (same stride).
__global__ __launch_bounds__(64) void feed_row_kernel(const int32_t* __restrict__ trk, const int64_t* __restrict__ trk_off,
                                                      const int32_t* __restrict__ art, const int64_t* __restrict__ art_off,
                                                      int n_playlists, const int32_t* __restrict__ draw, int B, int x_side,
                                                      int64_t stride, int* __restrict__ yk, int* __restrict__ xk,
                                                      int* tmp, int* __restrict__ ycnt, int* __restrict__ xcnt,
                                                      int* __restrict__ rflag)
{
    __shared__ int s_id[FEED_SIDE_CAP];
    __shared__ unsigned char s_keep[FEED_SIDE_CAP];     // bit 0: y-kept, bit 1: x-kept
    __shared__ int s_cnt[2];
    const int row = blockIdx.x, lane = threadIdx.x;
    const int p = draw[row];
    if (p < 0 || p >= n_playlists) {                     // the caller's status bit 0; the row is empty
        if (lane == 0) { ycnt[row] = 0; xcnt[row] = 0; rflag[row] = 1; }
        return;
    }
    const int64_t b = (int64_t)row * stride;
    int ybase = 0, xbase = 0;
    for (int side = 0; side < 2; ++side) {
        const int64_t* off = side ? art_off : trk_off;
        const int64_t o0 = off[p];
        const int n = (int)(off[p + 1] - o0);
        const int32_t* __restrict__ ids = (side ? art : trk) + o0;
        const int given = draw[(int64_t)(1 + side) * B + row];
        const bool in_x = x_side == 2 || x_side == side;
        const int lim = !in_x ? 0 : (given < 0 || given > n ? n : given);     // entry i carries 1 in x iff i < lim
        if (lane == 0) { s_cnt[0] = 0; s_cnt[1] = 0; }
        __syncthreads();
        if (n <= FEED_SIDE_CAP) {
            for (int i = lane; i < n; i += 64) s_id[i] = ids[i];
            __syncthreads();
            for (int i = lane; i < n; i += 64) {
                const int c = s_id[i];
                int later = 0;
                for (int j = 0; j < n; ++j) later |= (s_id[j] == c) & (j > i);
                s_keep[i] = later ? 0 : (i < lim ? 3 : 1);
            }
            __syncthreads();
            for (int i = lane; i < n; i += 64) {
                const int k = s_keep[i];
                if (!k) continue;
                const int c = s_id[i];
                int ys = 0, xs = 0;
                for (int j = 0; j < n; ++j) {
                    const int kj = s_keep[j], lt = s_id[j] < c;
                    ys += (kj & 1) & lt;
                    xs += (kj >> 1) & lt;
                }
                yk[b + ybase + ys] = c;
                atomicAdd(&s_cnt[0], 1);
                if (k & 2) { xk[b + xbase + xs] = c; atomicAdd(&s_cnt[1], 1); }
            }
        } else {
            // ---- a side longer than the LDS buffers: flags in tmp[b .. b + n) (n <= stride), ids re-read from the table ----
            for (int i = lane; i < n; i += 64) {
                const int c = ids[i];
                int later = 0;
                for (int j = i + 1; j < n; ++j) later |= ids[j] == c;
                tmp[b + i] = later ? 0 : (i < lim ? 3 : 1);
            }
            __threadfence_block();
            __syncthreads();
            for (int i = lane; i < n; i += 64) {
                const int k = tmp[b + i];
                if (!k) continue;
                const int c = ids[i];
                int ys = 0, xs = 0;
                for (int j = 0; j < n; ++j) {
                    const int kj = tmp[b + j], lt = ids[j] < c;
                    ys += (kj & 1) & lt;
                    xs += (kj >> 1) & lt;
                }
                yk[b + ybase + ys] = c;
                atomicAdd(&s_cnt[0], 1);
                if (k & 2) { xk[b + xbase + xs] = c; atomicAdd(&s_cnt[1], 1); }
            }
        }
        __syncthreads();
        ybase += s_cnt[0];
        xbase += s_cnt[1];
        __syncthreads();                                 // every lane has read the counts before the next side clears them
    }
    if (lane == 0) { ycnt[row] = ybase; xcnt[row] = xbase; rflag[row] = 0; }
}

// One workgroup per row: row_ptr of both CSRs from the counts of the rows before, then the copy (values are all 1.0f).
// Nothing is written at or past a cap; row_ptr holds the offsets the full result would have.  The workgroup of the last
// row has walked every row's counters anyway and writes the status word: bit 0 from the rows' flags, bit 1 from the totals.
__global__ __launch_bounds__(256) void feed_compact_kernel(const int* __restrict__ ycnt, const int* __restrict__ xcnt,
                                                           const int* __restrict__ rflag, int B, int64_t stride,
                                                           const int* __restrict__ yk, const int* __restrict__ xk,
                                                           int32_t* __restrict__ x_row_ptr, int32_t* __restrict__ x_col,
                                                           float* __restrict__ x_val, int x_cap,
                                                           int32_t* __restrict__ y_row_ptr, int32_t* __restrict__ y_col,
                                                           float* __restrict__ y_val, int y_cap, int32_t* __restrict__ status)
{
    __shared__ int wy[4], wx[4], wf[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const bool last = row == B - 1;
    int sy = 0, sx = 0, f = 0;
    for (int r = tid; r < row; r += 256) { sy += ycnt[r]; sx += xcnt[r]; }
    if (last)
        for (int r = tid; r < B; r += 256) f |= rflag[r];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { sy += __shfl_xor(sy, d); sx += __shfl_xor(sx, d); f |= __shfl_xor(f, d); }
    if (lane == 0) { wy[tid >> 6] = sy; wx[tid >> 6] = sx; wf[tid >> 6] = f; }
    __syncthreads();
    const int oy = wy[0] + wy[1] + wy[2] + wy[3];
    const int ox = wx[0] + wx[1] + wx[2] + wx[3];
    const int my = ycnt[row], mx = xcnt[row];
    if (tid == 0) {
        y_row_ptr[row] = oy;
        x_row_ptr[row] = ox;
        if (last) {
            y_row_ptr[B] = oy + my;
            x_row_ptr[B] = ox + mx;
            *status = (wf[0] | wf[1] | wf[2] | wf[3]) | ((oy + my > y_cap || ox + mx > x_cap) ? 2 : 0);
        }
    }
    const int64_t b = (int64_t)row * stride;
    for (int s = tid; s < my; s += 256)
        if (oy + s < y_cap) { y_col[oy + s] = yk[b + s]; y_val[oy + s] = 1.0f; }
    for (int s = tid; s < mx; s += 256)
        if (ox + s < x_cap) { x_col[ox + s] = xk[b + s]; x_val[ox + s] = 1.0f; }
}

// One wave per batch row (four rows per workgroup): lane i copies character i of the drawn playlist's title; a playlist
// index out of range gives a row of -1 (no character) -- feed_row_kernel raises the status bit for that same draw.
__global__ __launch_bounds__(256) void feed_titles_kernel(const int32_t* __restrict__ titles, int n_playlists, int L,
                                                          const int32_t* __restrict__ draw, int B, int32_t* __restrict__ out)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    const int p = draw[row];
    const bool ok = p >= 0 && p < n_playlists;
    for (int i = lane; i < L; i += 64) out[(int64_t)row * L + i] = ok ? titles[(int64_t)p * L + i] : -1;
}

}  // namespace

int dae_train_set_create(dae_ctx* ctx, const int32_t* trk, const int64_t* trk_off, const int32_t* art, const int64_t* art_off,
                         int n_playlists, int n_tracks, int n_items, dae_train_set** out)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!out) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    *out = nullptr;
    // everything the device path takes for granted is refused here, before any HIP call
    dae_train_set_shape shape;
    char msg[256];
    const int rc = dae_train_set_check(trk, trk_off, art, art_off, n_playlists, n_tracks, n_items, &shape, msg, sizeof(msg));
    if (rc) return dae_fail(ctx, rc, "dae_train_set_create: %s", msg);
    const size_t off_bytes = ((size_t)n_playlists + 1) * sizeof(int64_t);
    const size_t trk_bytes = ((size_t)shape.n_trk * sizeof(int32_t) + 15) & ~(size_t)15;
    const size_t art_bytes = ((size_t)shape.n_art * sizeof(int32_t) + 15) & ~(size_t)15;
    DAE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    char* block = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&block), 2 * off_bytes + trk_bytes + art_bytes + 16);
    if (e != hipSuccess) return dae_fail(ctx, DAE_ERR_NOMEM, "dae_train_set_create: hipMalloc failed: %s", hipGetErrorString(e));
    dae_train_set* s = new dae_train_set();
    s->device = ctx->device;
    s->block = block;
    s->trk_off = reinterpret_cast<const int64_t*>(block);
    s->art_off = reinterpret_cast<const int64_t*>(block + off_bytes);
    s->trk = reinterpret_cast<const int32_t*>(block + 2 * off_bytes);
    s->art = reinterpret_cast<const int32_t*>(block + 2 * off_bytes + trk_bytes);
    s->n_playlists = n_playlists; s->n_tracks = n_tracks; s->n_items = n_items;
    s->shape = shape;
    e = hipMemcpy(block, trk_off, off_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(block + off_bytes, art_off, off_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && shape.n_trk)
        e = hipMemcpy(block + 2 * off_bytes, trk, (size_t)shape.n_trk * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && shape.n_art)
        e = hipMemcpy(block + 2 * off_bytes + trk_bytes, art, (size_t)shape.n_art * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(block);
        delete s;
        return dae_fail(ctx, DAE_ERR_HIP, "dae_train_set_create: upload failed: %s", hipGetErrorString(e));
    }
    *out = s;
    return DAE_OK;
}

int dae_train_set_destroy(dae_train_set* set)
{
    if (!set) return DAE_OK;
    (void)hipSetDevice(set->device);
    (void)hipDeviceSynchronize();          // a batch that reads the table may still be running
    (void)hipFree(set->block);
    if (set->titles) (void)hipFree(set->titles);
    delete set;
    return DAE_OK;
}

int dae_train_set_attach_titles(dae_train_set* set, const int32_t* titles, int n_playlists, int L, int n_char)
{
    // (no context here: the message goes where dae_create's does, dae_last_error(NULL))
    if (!set) return dae_fail(nullptr, DAE_ERR_ARG, "dae_train_set_attach_titles: null pointer");
    if (set->titles) return dae_fail(nullptr, DAE_ERR_STATE, "dae_train_set_attach_titles: the set already holds titles");
    char msg[256];
    const int rc = dae_train_titles_check(titles, n_playlists, set->n_playlists, L, n_char, msg, sizeof(msg));
    if (rc) return dae_fail(nullptr, rc, "dae_train_set_attach_titles: %s", msg);
    const size_t bytes = (size_t)n_playlists * (size_t)L * sizeof(int32_t);
    hipError_t e = hipSetDevice(set->device);
    if (e != hipSuccess) return dae_fail(nullptr, DAE_ERR_HIP, "dae_train_set_attach_titles: hipSetDevice: %s", hipGetErrorString(e));
    int32_t* d = nullptr;
    e = hipMalloc(reinterpret_cast<void**>(&d), bytes);
    if (e != hipSuccess) return dae_fail(nullptr, DAE_ERR_NOMEM, "dae_train_set_attach_titles: hipMalloc failed: %s", hipGetErrorString(e));
    e = hipMemcpy(d, titles, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return dae_fail(nullptr, DAE_ERR_HIP, "dae_train_set_attach_titles: upload failed: %s", hipGetErrorString(e));
    }
    set->titles = d;
    set->title_len = L;
    return DAE_OK;
}

int dae_train_batch(dae_ctx* ctx, const dae_train_set* set, const int32_t* draw, int B, int x_side,
                    int32_t* x_row_ptr, int32_t* x_col, float* x_val, int x_cap,
                    int32_t* y_row_ptr, int32_t* y_col, float* y_val, int y_cap, int32_t* status)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!set || !draw || !x_row_ptr || !y_row_ptr || !status || (x_cap > 0 && (!x_col || !x_val)) ||
        (y_cap > 0 && (!y_col || !y_val)))
        return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (B < 1 || B > 4096) return dae_fail(ctx, DAE_ERR_ARG, "dae_train_batch: B=%d, must be in [1, 4096]", B);
    if (x_side < 0 || x_side > 2) return dae_fail(ctx, DAE_ERR_ARG, "dae_train_batch: x_side=%d (0 tracks, 1 artists, 2 both)", x_side);
    if (x_cap < 0 || y_cap < 0) return dae_fail(ctx, DAE_ERR_ARG, "dae_train_batch: negative capacity");
    if (set->device != ctx->device) return dae_fail(ctx, DAE_ERR_ARG, "dae_train_batch: the set lives on device %d", set->device);
    // scratch: ycnt | xcnt | rflag [B each], then yk | xk (| tmp when a side can outgrow the LDS buffers) [B * stride each]
    const int64_t stride = set->shape.max_row > 0 ? set->shape.max_row : 1;
    if ((int64_t)B * stride >= (int64_t)1 << 31)
        return dae_fail(ctx, DAE_ERR_ARG, "dae_train_batch: %d rows of up to %lld entries do not fit 32-bit CSR offsets", B,
                        (long long)stride);
    const bool long_sides = set->shape.max_side > FEED_SIDE_CAP;
    const size_t nb = ((size_t)B + 3) & ~(size_t)3;
    const size_t ints = 3 * nb + (long_sides ? 3 : 2) * (size_t)B * (size_t)stride;
    int rc;
    if ((rc = dae_reserve(ctx, ctx->feed_tmp, ints * sizeof(int)))) return rc;
    int* ycnt = static_cast<int*>(ctx->feed_tmp.p);
    int* xcnt = ycnt + nb;
    int* rflag = xcnt + nb;
    int* yk = rflag + nb;
    int* xk = yk + (size_t)B * stride;
    int* tmp = long_sides ? xk + (size_t)B * stride : nullptr;
    hipLaunchKernelGGL(feed_row_kernel, dim3(B), dim3(64), 0, ctx->stream, set->trk, set->trk_off, set->art, set->art_off,
                       set->n_playlists, draw, B, x_side, stride, yk, xk, tmp, ycnt, xcnt, rflag);
    DAE_CHECK_LAUNCH(ctx, "feed_row_kernel");
    hipLaunchKernelGGL(feed_compact_kernel, dim3(B), dim3(256), 0, ctx->stream, ycnt, xcnt, rflag, B, stride, yk, xk,
                       x_row_ptr, x_col, x_val, x_cap, y_row_ptr, y_col, y_val, y_cap, status);
    DAE_CHECK_LAUNCH(ctx, "feed_compact_kernel");
    return DAE_OK;
}

int dae_train_titles(dae_ctx* ctx, const dae_train_set* set, const int32_t* draw, int B, int32_t* titles_out)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!set || !draw || !titles_out) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (B < 1 || B > 4096) return dae_fail(ctx, DAE_ERR_ARG, "dae_train_titles: B=%d, must be in [1, 4096]", B);
    if (set->device != ctx->device) return dae_fail(ctx, DAE_ERR_ARG, "dae_train_titles: the set lives on device %d", set->device);
    if (!set->titles) return dae_fail(ctx, DAE_ERR_STATE, "dae_train_titles: the set holds no titles (dae_train_set_attach_titles)");
    hipLaunchKernelGGL(feed_titles_kernel, dim3((B + 3) / 4), dim3(256), 0, ctx->stream, set->titles, set->n_playlists,
                       set->title_len, draw, B, titles_out);
    DAE_CHECK_LAUNCH(ctx, "feed_titles_kernel");
    return DAE_OK;
}
