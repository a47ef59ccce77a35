// pipeline.hip -- the drivers' loop of the reference (main_challenge.py:72-93, main_train.py:62-96: read a batch, feed it,
// fetch y_pred, rank, next batch) as a C-side streaming pipeline: HOST feeds in, HOST top-k lists out.
//
// What the Python loop of round 3 (models/DAEs.py recommend_iter) did per launch -- stage the COO feed in pinned memory,
// upload, build the CSR and the seed lists on the device, score, fetch -- took ~0.3 ms of interpreter time against 0.05 -
// 0.2 ms of kernels, and threads did not help it (the GIL).  Here the caller's thread only copies a feed into a pinned
// staging buffer (dae_pipeline_submit) and picks finished lists up (dae_pipeline_poll: pointers into pinned result blocks,
// no copy); a library-owned thread issues every launch -- H2D, the feed -> CSR + seed lists, dae_score_topk, the lists' stores --
// on one of `lanes` contexts / streams that take the launches in turn and share ONE packed decoder image.  Consecutive
// feeds are scored in one launch of up to `group_rows` rows: rows are scored independently, so every feed gets the bits
// dae_score_topk returns for it alone.  Seeds are the playlist's own tracks (what both reference drivers pass).
//
// This unit is the C ABI -- the caller's thread: create / destroy, the stream pool, the modes, submit, poll, release.  What the
// caller's thread does on host memory alone is pipeline_stage.h; the library's threads and what they enqueue, pipeline_issue.hip;
// the state all three share, pipeline_state.h.
#include "pipeline_state.h"

static thread_local std::string g_pipe_err;

namespace dae_pipe {

int pfail(dae_pipeline* p, int code, const char* msg)
{
    if (p) { std::lock_guard<std::mutex> g(p->err_mu); p->err = msg; } else g_pipe_err = msg;
    return code;
}
int pfatal(dae_pipeline* p, int code, const char* msg)
{
    if (p) {
        std::lock_guard<std::mutex> g(p->err_mu);
        if (!p->err_code) { p->err = msg; p->err_code = code; }
    }
    return code;
}

static int stage_fail(dae_pipeline* p, const StageErr& e)       // a refusal of pipeline_stage.h as this call's error
{
    return pfail(p, e.kind == STAGE_BUSY ? DAE_PIPE_BUSY : e.kind == STAGE_STATE ? DAE_ERR_STATE : DAE_ERR_ARG, e.msg);
}

// close the open launch: a result block and a lane for it, then over to the worker (caller thread, lock held)
static int close_open(dae_pipeline* p)
{
    if (p->open_slot < 0) return DAE_OK;
    int si = -1;
    if (const StageErr e = p->close_launch(&si)) return stage_fail(p, e);
    p->queue.push_back(si);
    p->cv_worker.notify_one();
    return DAE_OK;
}

// The fp32 re-run after a guard hit: `before` is what the kind of launch does first under issue_mu (on the launch's lane), then the
// same launch again on the fp32 kernels, here and now -- its feed is still in the slot's staging buffers; the lane's context is
// shared with the worker: issue_mu.  Returns with `lk` held again.
template <class Before>
static int guard_rerun(dae_pipeline* p, Slot& S, std::unique_lock<std::mutex>& lk, Before before)
{
    int rc;
    bool ok;
    {
        std::lock_guard<std::mutex> g(p->issue_mu);
        DeviceGuard dev_guard(p->device);
        rc = before(p->lanes[S.lane]);
        if (!rc) rc = pipe_issue(p, S, DAE_DTYPE_F32);
        ok = !rc && pipe_wait_launch(S) == hipSuccess;
    }
    lk.lock();
    if (!ok) return pfatal(p, rc ? rc : DAE_ERR_HIP, "dae_pipeline: the fp32 re-run after a bound-guard hit failed");
    ++p->guard_fallbacks;
    return DAE_OK;
}

}  // namespace dae_pipe
using namespace dae_pipe;

extern "C" {

const char* dae_pipeline_last_error(const dae_pipeline* p)
{
    if (!p) return g_pipe_err.c_str();
    thread_local std::string copy;                           // (the library thread may replace p->err at any time)
    {
        std::lock_guard<std::mutex> g(const_cast<dae_pipeline*>(p)->err_mu);
        copy = p->err;
    }
    return copy.c_str();
}

// Lane and copy streams are taken from a process-wide pool and RETURNED to it, never destroyed: the runtime binds a stream to a
// hardware queue when it is created, and after a pipeline's streams were destroyed the next pipeline's fresh ones came out sharing
// queues -- its lanes' launches queued behind each other (bench.py's host-loop rows run fp32, then exact_bf16, on one model: the
// second pipeline measured 5.8 M playlists/s against 7.3 M as the process's first; scripts/probe/row_diag.py)
// Round 6: the pool is keyed by ROLE as well.  It was first-in first-out over all of a pipeline's streams, so every other pipeline
// of a process got its LANES on streams that had been the copy / out / prep streams before (and the other way round): such a
// pipeline ran 25 - 30 % slower -- 6.1 against 8.4 M playlists/s, instance after instance in the pattern fast, fast, slow, slow
// (scripts/gpu_r6_t14.sh; bench.py's host-loop rows and scripts/bench_loop.py disagreed by exactly that).  A stream now returns to
// the role it was created for: 0 = a lane (kernels of the scoring call), 1 = copies (upload / out), 2 = the CSR build.
static std::mutex g_stream_pool_mu;
struct PooledStream { int device, role; hipStream_t s; };
static std::vector<PooledStream> g_stream_pool;
static hipStream_t pool_take_stream(int device, int role)
{
    {
        std::lock_guard<std::mutex> lk(g_stream_pool_mu);
        for (size_t i = g_stream_pool.size(); i-- > 0;)                        // (last in, first out: a lane gets a lane's stream back)
            if (g_stream_pool[i].device == device && g_stream_pool[i].role == role) {
                hipStream_t s = g_stream_pool[i].s;
                g_stream_pool.erase(g_stream_pool.begin() + (long)i);
                return s;
            }
    }
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    return s;
}
static void pool_give_stream(int device, hipStream_t s, int role)
{
    if (!s) return;
    (void)hipStreamSynchronize(s);
    std::lock_guard<std::mutex> lk(g_stream_pool_mu);
    g_stream_pool.push_back(PooledStream{device, role, s});
}

int dae_pipeline_destroy(dae_pipeline* p)
{
    if (!p) return DAE_OK;
    {
        std::lock_guard<std::mutex> g(p->mu);
        p->stop = true;
    }
    p->cv_worker.notify_all();
    if (p->worker.joinable()) p->worker.join();
    {
        std::lock_guard<std::mutex> g(p->out_mu);
        p->out_stop = true;
    }
    p->cv_out.notify_all();
    if (p->out_worker.joinable()) p->out_worker.join();
    DeviceGuard dev_guard(p->device);
    for (Lane& L : p->lanes) {
        if (L.stream) (void)hipStreamSynchronize(L.stream);
        if (L.tctx) (void)dae_destroy(L.tctx);                  // (borrows lane 0's images: never frees them)
        if (L.ctx) { (void)dae_set_decode_gate(L.ctx, nullptr, nullptr); (void)dae_destroy(L.ctx); }
        pool_give_stream(p->device, L.stream, 0);
    }
    pool_give_stream(p->device, p->copy_stream, 1);
    if (p->out_stream) { (void)hipStreamSynchronize(p->out_stream); pool_give_stream(p->device, p->out_stream, 1); }
    if (p->prep_stream) (void)hipStreamSynchronize(p->prep_stream);
    if (p->prep_tctx) (void)dae_destroy(p->prep_tctx);
    if (p->prep_ctx) (void)dae_destroy(p->prep_ctx);
    pool_give_stream(p->device, p->prep_stream, 2);
    p->mem.free_all();                                       // every buffer, pinned block and event: nothing uses them any more
    delete p;
    return DAE_OK;
}

static int pipeline_create(int device, const float* W_enc, const float* b_enc, const float* W_dec, const float* b_dec,
                           int V, int H, int n_tracks, int dtype, int k, int group_rows, int64_t max_nnz, int lanes,
                           int want_scores, int result_blocks, const TitleW* tw, dae_pipeline** out)
{
    if (!out) return pfail(nullptr, DAE_ERR_ARG, "out is null");
    if (!W_enc || !b_enc || !W_dec || !b_dec) return pfail(nullptr, DAE_ERR_ARG, "null pointer");
    if (k > DAE_MAX_K) return pfail(nullptr, DAE_ERR_ARG, "dae_pipeline_create: k out of [1,1024]");
    static_assert(DAE_MAX_K == 1024, "the message above names the limit");
    if (V <= 0 || H <= 0 || n_tracks <= 0 || n_tracks > V || k < 1 || group_rows < 1 || group_rows > 16384 ||
        max_nnz < 1 || max_nnz >= ((int64_t)1 << 31) || lanes < 1 || lanes > 8)
        return pfail(nullptr, DAE_ERR_ARG, "dae_pipeline_create: bad shape / sizes");
    if (dtype != DAE_DTYPE_F32 && dtype != DAE_DTYPE_BF16 && dtype != DAE_DTYPE_BF16_EXACT)
        return pfail(nullptr, DAE_ERR_ARG, "dae_pipeline_create: unknown dtype");
    const int n_slots = 2 * lanes + 2;                       // launches staged, queued, running or waiting to be polled
    if (result_blocks < n_slots) result_blocks = n_slots;
    dae_pipeline* p = new dae_pipeline();
    p->device = device; p->V = V; p->H = H; p->n_tracks = n_tracks; p->dtype = dtype; p->k = k; p->group_rows = group_rows;
    p->max_nnz = max_nnz; p->want_scores = want_scores ? 1 : 0;
    p->W_enc = W_enc; p->b_enc = b_enc; p->W_dec = W_dec; p->b_dec = b_dec;
    if (tw) { p->has_title = true; p->tw = *tw; }
    p->lanes.resize(lanes);
    p->slots.resize(n_slots);
    p->blocks.resize(result_blocks);
    p->title_len = p->tw.L; p->n_lanes = lanes;
    PipeMem& M = p->mem;
    auto bail = [&](int rc, const char* msg) { const std::string m(msg); dae_pipeline_destroy(p); g_pipe_err = m; return rc; };
    DeviceGuard dev_guard(device);
    { int cur = -1; if (hipGetDevice(&cur) != hipSuccess || cur != device) return bail(DAE_ERR_HIP, "hipSetDevice failed"); }
    if (!(p->copy_stream = pool_take_stream(device, 1))) return bail(DAE_ERR_HIP, "stream creation failed");
    if (!(p->out_stream = pool_take_stream(device, 1))) return bail(DAE_ERR_HIP, "stream creation failed");
    if (!(p->prep_stream = pool_take_stream(device, 2))) return bail(DAE_ERR_HIP, "stream creation failed");
    {
        int rc_p = dae_create(device, &p->prep_ctx);
        if (!rc_p) rc_p = dae_set_stream(p->prep_ctx, p->prep_stream);
        if (rc_p) return bail(rc_p, dae_last_error(p->prep_ctx));
    }
    const size_t rows = (size_t)group_rows, nz = (size_t)max_nnz, kk = (size_t)k;
    const char* msg = "";
    auto images = [&](int i, int which) {                    // lane 0 re-tiles an image, the others borrow it
        return i == 0 ? pipe_pack_images(p, dtype, which, &msg) : pipe_borrow_images(p, i, dtype, which, &msg);
    };
    for (int i = 0; i < lanes; ++i) {
        Lane& L = p->lanes[i];
        int rc = dae_create(device, &L.ctx);
        if (rc) return bail(rc, dae_last_error(nullptr));
        L.stream = pool_take_stream(device, 0);
        L.d_score = M.dev<float>(PipeMem::pad16<float>(rows * kk));
        if (!L.stream || !M.ok) return bail(DAE_ERR_NOMEM, "dae_pipeline_create: allocation failed");
        rc = dae_set_stream(L.ctx, L.stream);
        if (rc) return bail(rc, dae_last_error(L.ctx));
        rc = images(i, IMG_DAE);
        if (rc) return bail(rc, msg);
        if (i == 0 && hipStreamSynchronize(L.stream) != hipSuccess) return bail(DAE_ERR_HIP, "prepack failed");
        (void)dae_set_overlap_hint(L.ctx, lanes);
        if (tw) {
            // the title scorer next to the DAE: its own context on the lane's stream, its "decoder" = Output_W^T / Output_b
            rc = dae_create(device, &L.tctx);
            if (rc) return bail(rc, dae_last_error(nullptr));
            L.d_guard = M.dev<int32_t>(DAE_GUARD_BYTES / sizeof(int32_t));
            if (!M.ok || hipMemsetAsync(L.d_guard, 0, DAE_GUARD_BYTES, L.stream) != hipSuccess)
                return bail(DAE_ERR_NOMEM, "dae_pipeline_create: allocation failed");
            rc = dae_set_stream(L.tctx, L.stream);
            if (rc) return bail(rc, dae_last_error(L.tctx));
            rc = images(i, IMG_TITLE);
            if (rc) return bail(rc, msg);
            // (the scorer is frozen for the life of the pipeline: its convolutions as a table, dae_title_prepack_features)
            rc = dae_title_prepack_features(L.tctx, tw->emb, tw->n_char, tw->E, tw->conv_w, tw->fs.data(), tw->n_sizes, tw->F);
            if (rc) return bail(rc, dae_last_error(L.tctx));
            if (i == 0 && hipStreamSynchronize(L.stream) != hipSuccess) return bail(DAE_ERR_HIP, "prepack failed");
            (void)dae_set_overlap_hint(L.tctx, lanes);
            if (dtype == DAE_DTYPE_F32) { L.has_f32 = true; L.t_has_f32 = true; }
        }
    }
    if (tw) {
        int rc_t = dae_create(device, &p->prep_tctx);
        if (!rc_t) rc_t = dae_set_stream(p->prep_tctx, p->prep_stream);
        if (!rc_t) rc_t = dae_title_prepack_features(p->prep_tctx, tw->emb, tw->n_char, tw->E, tw->conv_w, tw->fs.data(), tw->n_sizes, tw->F);
        if (rc_t) return bail(rc_t, dae_last_error(p->prep_tctx));
    }
    for (Slot& S : p->slots) {
        S.ev_scored = M.event();                             // (in the order the buffers have always been made)
        S.d_idx = M.dev<int32_t>(PipeMem::pad16<int32_t>(rows * kk));
        if (want_scores) S.d_score = M.dev<float>(PipeMem::pad16<float>(rows * kk));
        S.d_flags = M.dev<int32_t>(4);
        S.ev_prep = M.event();
        S.d_rp = M.dev<int32_t>(rows + 1); S.d_col = M.dev<int32_t>(nz); S.d_cval = M.dev<float>(nz);
        S.d_status = M.dev<int32_t>(1);
        S.d_srp = M.dev<int32_t>(rows + 1); S.d_scol = M.dev<int32_t>(nz);
        S.ev_h2d = M.event(); S.ev_gate = M.event();
        S.d_pos = M.dev<int64_t>(nz * 2); S.d_val = M.dev<float>(nz);
        S.h_pos = M.pinned<int64_t>(nz * 2); S.h_val = M.pinned<float>(nz); S.h_flags = M.pinned<int32_t>(8);
        if (tw) {
            S.t_h = M.dev<float>(rows * (size_t)H); S.t_feat = M.dev<float>(rows * (size_t)tw->ld_feat);
            S.t_wt = M.dev<float>(rows); S.t_wp = M.dev<float>(rows);
            S.d_titles = M.dev<int32_t>(rows * (size_t)tw->L); S.d_use = M.dev<float>(rows);
            S.h_titles = M.pinned<int32_t>(rows * (size_t)tw->L); S.h_use = M.pinned<float>(rows);
        }
        if (!M.ok) return bail(DAE_ERR_NOMEM, "dae_pipeline_create: pinned allocation failed");
        S.h_flags[0] = S.h_flags[1] = 0; S.h_flags[2] = -1; S.h_flags[3] = 0; S.h_flags[4] = 0;
    }
    for (OutBlock& b : p->blocks) {
        b.idx = M.pinned<int32_t>(rows * kk + 4);            // (16 bytes past the lists)
        if (want_scores) b.score = M.pinned<float>(rows * kk + 4);
    }
    if (!M.ok) return bail(DAE_ERR_NOMEM, "dae_pipeline_create: pinned allocation failed");
    for (Lane& L : p->lanes) if (hipStreamSynchronize(L.stream) != hipSuccess) return bail(DAE_ERR_HIP, "setup failed");
    p->out_worker = std::thread(pipe_out_worker_main, p);
    p->worker = std::thread(pipe_worker_main, p);
    *out = p;
    return DAE_OK;
}

int dae_pipeline_create(int device, const float* W_enc, const float* b_enc, const float* W_dec, const float* b_dec,
                        int V, int H, int n_tracks, int dtype, int k, int group_rows, int64_t max_nnz, int lanes,
                        int want_scores, int result_blocks, dae_pipeline** out)
{
    return pipeline_create(device, W_enc, b_enc, W_dec, b_dec, V, H, n_tracks, dtype, k, group_rows, max_nnz, lanes, want_scores,
                           result_blocks, nullptr, out);
}

int dae_pipeline_create_titled(int device, const float* W_enc, const float* b_enc, const float* W_dec, const float* b_dec,
                               int V, int H, int n_tracks, const float* emb, int n_char, int E, const float* conv_w,
                               const float* conv_b, const int32_t* filter_sizes, int n_sizes, int F, const float* Output_WT,
                               const float* Output_b, int ld_feat, int L, int dtype, int k, int group_rows, int64_t max_nnz,
                               int lanes, int want_scores, int result_blocks, dae_pipeline** out)
{
    if (!emb || !conv_w || !conv_b || !filter_sizes || !Output_WT || !Output_b) return pfail(nullptr, DAE_ERR_ARG, "null pointer");
    if (n_char < 1 || E < 1 || n_sizes < 1 || n_sizes > DAE_TITLE_MAX_SIZES || F < 1 || L < 1 || ld_feat < n_sizes * F || group_rows > 4096)
        return pfail(nullptr, DAE_ERR_ARG, "dae_pipeline_create_titled: bad title shapes (a titled launch holds at most 4096 rows)");
    TitleW tw;
    tw.emb = emb; tw.conv_w = conv_w; tw.conv_b = conv_b; tw.out_WT = Output_WT; tw.out_b = Output_b;
    tw.n_char = n_char; tw.E = E; tw.n_sizes = n_sizes; tw.F = F; tw.ld_feat = ld_feat; tw.L = L;
    tw.fs.assign(filter_sizes, filter_sizes + n_sizes);
    return pipeline_create(device, W_enc, b_enc, W_dec, b_dec, V, H, n_tracks, dtype, k, group_rows, max_nnz, lanes, want_scores,
                           result_blocks, &tw, out);
}

int dae_pipeline_flush(dae_pipeline* p)
{
    if (!p) return DAE_ERR_ARG;
    std::unique_lock<std::mutex> lk(p->mu);
    if (p->err_code) return p->err_code;
    return close_open(p);
}

static int submit_impl(dae_pipeline* p, const int64_t* positions, const float* values, int values_broadcast, int64_t nnz,
                       int n_rows, const int32_t* titles, const float* titles_use, const int32_t* ans_rp, const int32_t* ans_col,
                       const int32_t* cand_rp, const int32_t* cand_col, uint64_t* ticket_out)
{
    if (!p) return DAE_ERR_ARG;
    const int titled = titles != nullptr ? 1 : 0;
    int64_t n_ans = 0, n_cand = 0;
    int longest = 0;
    // (p->cand, like p->eval, is set once, before the first submit, by the caller's own thread)
    if (p->cand != (cand_rp != nullptr))
        return pfail(p, DAE_ERR_STATE, p->cand ? "dae_pipeline: a candidates pipeline takes dae_pipeline_submit_candidates only"
                                               : "dae_pipeline_submit_candidates: dae_pipeline_enable_candidates was not called");
    if (p->cand)
        if (const StageErr e = p->check_candidates(n_rows, cand_rp, cand_col, &n_cand, &longest)) return stage_fail(p, e);
    // (p->eval is set once, before the first submit, by the caller's own thread)
    if (const StageErr e = p->check_feed(p->eval, positions, values, nnz, n_rows, ans_rp, ans_col, &n_ans)) return stage_fail(p, e);
    const auto t_sub = std::chrono::steady_clock::now();
    if (titled && !p->rows_inside(positions, nnz, n_rows)) return stage_fail(p, p->bad_row());
    std::unique_lock<std::mutex> lk(p->mu);
    if (p->err_code) return p->err_code;
    if (p->open_slot >= 0 && (!p->fits_open(n_rows, nnz, titled, n_ans) || (p->cand && !p->cand_fits_open(n_cand)))) {
        const int rc = close_open(p);
        if (rc) return rc;
    }
    Staged at;
    if (const StageErr e = p->begin(n_rows, nnz, titled, n_ans, &at)) return stage_fail(p, e);
    if (p->cand) p->begin_candidates(&at, n_cand, longest);
    lk.unlock();                                           // the copy runs outside the lock (the worker never touches an open slot)
    if (!p->copy_positions(at, titled, positions, nnz, n_rows)) {
        lk.lock();                                           // nothing of this feed stays: the slot is as it was before the call
        if (p->cand) p->rollback_candidates(at, n_cand);
        p->rollback(at, n_rows, nnz, n_ans);
        return stage_fail(p, p->bad_row());
    }
    p->copy_values(at, values, values_broadcast, nnz);
    if (titled) p->copy_titles(at, titles, titles_use, n_rows);
    if (ans_rp) p->copy_answers(at, ans_rp, ans_col, n_rows, n_ans);
    if (cand_rp) p->copy_candidates(at, cand_rp, cand_col, n_rows, n_cand);
    if (ticket_out) *ticket_out = at.ticket;
    lk.lock();
    if (p->open_is_full_for(n_rows)) (void)close_open(p);   // the next feed of this size would not fit: off it goes
    p->submit_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_sub).count();
    return DAE_OK;
}

int dae_pipeline_submit(dae_pipeline* p, const int64_t* positions, const float* values, int values_broadcast, int64_t nnz,
                        int n_rows, uint64_t* ticket_out)
{
    return submit_impl(p, positions, values, values_broadcast, nnz, n_rows, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ticket_out);
}

int dae_pipeline_submit_titled(dae_pipeline* p, const int64_t* positions, const float* values, int values_broadcast, int64_t nnz,
                               int n_rows, const int32_t* titles, const float* titles_use, uint64_t* ticket_out)
{
    if (!p) return DAE_ERR_ARG;
    if (!p->has_title) return pfail(p, DAE_ERR_STATE, "dae_pipeline_submit_titled: not a titled pipeline (dae_pipeline_create_titled)");
    if (!titles || !titles_use) return pfail(p, DAE_ERR_ARG, "null pointer");
    return submit_impl(p, positions, values, values_broadcast, nnz, n_rows, titles, titles_use, nullptr, nullptr, nullptr, nullptr, ticket_out);
}

int dae_pipeline_submit_eval(dae_pipeline* p, const int64_t* positions, const float* values, int values_broadcast, int64_t nnz,
                             int n_rows, const int32_t* titles, const float* titles_use, const int32_t* ans_row_ptr,
                             const int32_t* ans_col, uint64_t* ticket_out)
{
    if (!p) return DAE_ERR_ARG;
    if (!ans_row_ptr) return pfail(p, DAE_ERR_ARG, "null pointer");
    if ((titles != nullptr) != (titles_use != nullptr)) return pfail(p, DAE_ERR_ARG, "titles and titles_use come together");
    if (titles && !p->has_title) return pfail(p, DAE_ERR_STATE, "dae_pipeline_submit_eval: not a titled pipeline (dae_pipeline_create_titled)");
    return submit_impl(p, positions, values, values_broadcast, nnz, n_rows, titles, titles_use, ans_row_ptr, ans_col, nullptr, nullptr,
                       ticket_out);
}

int dae_pipeline_submit_candidates(dae_pipeline* p, const int64_t* positions, const float* values, int values_broadcast, int64_t nnz,
                                   int n_rows, const int32_t* titles, const float* titles_use, const int32_t* cand_row_ptr,
                                   const int32_t* cand_col, uint64_t* ticket_out)
{
    if (!p) return DAE_ERR_ARG;
    if (!cand_row_ptr) return pfail(p, DAE_ERR_ARG, "null pointer");
    if ((titles != nullptr) != (titles_use != nullptr)) return pfail(p, DAE_ERR_ARG, "titles and titles_use come together");
    if (titles && !p->has_title)
        return pfail(p, DAE_ERR_STATE, "dae_pipeline_submit_candidates: not a titled pipeline (dae_pipeline_create_titled)");
    return submit_impl(p, positions, values, values_broadcast, nnz, n_rows, titles, titles_use, nullptr, nullptr, cand_row_ptr, cand_col,
                       ticket_out);
}

// Before the first submit: the candidates' staging and device arrays per launch slot; in score mode the values' pinned blocks
// take the place of the lists' (which go back: nothing will be copied into them).
int dae_pipeline_enable_candidates(dae_pipeline* p, int64_t max_candidates, int rank, int out_kind)
{
    if (!p) return DAE_ERR_ARG;
    if (max_candidates < 1 || max_candidates >= ((int64_t)1 << 31) || (rank != 0 && rank != 1))
        return pfail(p, DAE_ERR_ARG, "dae_pipeline_enable_candidates: needs 1 <= max_candidates < 2^31 and rank = 0 or 1");
    if (out_kind != DAE_OUT_SCORE && out_kind != DAE_OUT_LOGIT)
        return pfail(p, DAE_ERR_ARG, "dae_pipeline_enable_candidates: out_kind is DAE_OUT_SCORE or DAE_OUT_LOGIT");
    std::unique_lock<std::mutex> lk(p->mu);
    if (p->err_code) return p->err_code;
    if (p->eval) return pfail(p, DAE_ERR_STATE, "dae_pipeline_enable_candidates: an evaluation pipeline (dae_pipeline_enable_eval) takes no candidates");
    if (p->cat) return pfail(p, DAE_ERR_STATE, "dae_pipeline_enable_candidates: a pipeline with a catalogue (dae_pipeline_set_catalogue) takes no candidates");
    if (p->cand || p->next_ticket != 1) return pfail(p, DAE_ERR_STATE, "dae_pipeline_enable_candidates: once, before the first submit");
    if (p->has_title && out_kind != DAE_OUT_SCORE)
        return pfail(p, DAE_ERR_ARG, "dae_pipeline_enable_candidates: DAE_OUT_LOGIT on a titled pipeline -- the title mix has no logit "
                                     "(DAE_OUT_SCORE)");
    // what the candidate kernels take (candidates.hip check_cand_args), refused here instead of at the first launch
    if (p->group_rows > 4096 || (p->H % 4) != 0 || p->H > 1024 || (p->has_title && ((p->tw.ld_feat % 4) != 0 || p->tw.ld_feat > 1024)))
        return pfail(p, DAE_ERR_ARG, "dae_pipeline_enable_candidates: the candidate kernels take launches of at most 4096 rows "
                                     "(group_rows) and hidden / title feature rows that are multiples of 4 up to 1024");
    DeviceGuard dev_guard(p->device);
    const size_t rows = (size_t)p->group_rows, nc = (size_t)max_candidates;
    PipeMem& M = p->mem;
    for (Slot& S : p->slots) {
        S.h_crp = M.pinned<int32_t>(rows + 1); S.h_ccol = M.pinned<int32_t>(nc);
        S.d_crp = M.dev<int32_t>(rows + 1); S.d_ccol = M.dev<int32_t>(nc);
        S.d_cout = M.dev<float>(nc); S.d_cstatus = M.dev<int32_t>(1);
    }
    if (!rank)
        for (OutBlock& b : p->blocks) {
            b.cand = M.pinned<float>(nc + 4);                // (the launch's status word sits behind the values)
            M.give_back(b.idx); M.give_back(b.score);
        }
    if (!M.ok) return pfatal(p, DAE_ERR_NOMEM, "dae_pipeline_enable_candidates: allocation failed");
    p->max_candidates = max_candidates;
    p->cand_rank = rank; p->cand_out_kind = out_kind;
    p->cand = true;
    return DAE_OK;
}

// Before the first submit: the discount table on the device, the answers' staging and the records' blocks; the lists' pinned
// blocks go back (nothing will be copied into them).
int dae_pipeline_enable_eval(dae_pipeline* p, const double* disc_host, int64_t max_answers)
{
    if (!p) return DAE_ERR_ARG;
    if (!disc_host || max_answers < 1 || max_answers >= ((int64_t)1 << 31))
        return pfail(p, DAE_ERR_ARG, "dae_pipeline_enable_eval: needs a discount table and 1 <= max_answers < 2^31");
    std::unique_lock<std::mutex> lk(p->mu);
    if (p->err_code) return p->err_code;
    if (p->cand) return pfail(p, DAE_ERR_STATE, "dae_pipeline_enable_eval: a candidates pipeline (dae_pipeline_enable_candidates) has no evaluation mode");
    if (p->eval || p->next_ticket != 1) return pfail(p, DAE_ERR_STATE, "dae_pipeline_enable_eval: once, before the first submit");
    DeviceGuard dev_guard(p->device);
    const size_t rows = (size_t)p->group_rows, na = (size_t)max_answers;
    PipeMem& M = p->mem;
    p->d_disc = M.dev<double>((size_t)p->k);
    bool ok = M.ok && hipMemcpy(p->d_disc, disc_host, (size_t)p->k * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    for (Slot& S : p->slots) {
        S.h_arp = M.pinned<int32_t>(rows + 1); S.h_acol = M.pinned<int32_t>(na);
        S.d_arp = M.dev<int32_t>(rows + 1); S.d_acol = M.dev<int32_t>(na);
        S.d_rec = M.dev<dae_metric_rec>(rows);
    }
    for (OutBlock& b : p->blocks) {
        b.rec = M.pinned<dae_metric_rec>(rows);
        M.give_back(b.idx); M.give_back(b.score);          // (the lists' blocks: nothing will be copied into them)
    }
    if (!ok || !M.ok) return pfatal(p, DAE_ERR_NOMEM, "dae_pipeline_enable_eval: allocation failed");
    p->max_answers = max_answers;
    p->eval = true;
    return DAE_OK;
}

// Before the first submit: the catalogue's images in the place of the vocabulary's on every lane (lane 0 gathers and tiles them,
// the others borrow: the catalogue's id travels with a shared image) and the slots' buffers for the translated seed lists.
int dae_pipeline_set_catalogue(dae_pipeline* p, const dae_catalogue* cat)
{
    if (!p) return DAE_ERR_ARG;
    if (!cat) return pfail(p, DAE_ERR_ARG, "null pointer");
    std::unique_lock<std::mutex> lk(p->mu);
    if (p->err_code) return p->err_code;
    if (p->cand) return pfail(p, DAE_ERR_STATE, "dae_pipeline_set_catalogue: a candidates pipeline (dae_pipeline_enable_candidates) ranks no catalogue");
    if (p->cat || p->next_ticket != 1) return pfail(p, DAE_ERR_STATE, "dae_pipeline_set_catalogue: once, before the first submit");
    int cat_dev = -1, cat_n = 0, cat_tracks = 0;
    dae_catalogue_shape(cat, &cat_dev, &cat_n, &cat_tracks);
    if (cat_dev != p->device) return pfail(p, DAE_ERR_ARG, "dae_pipeline_set_catalogue: the catalogue lives on another device than the pipeline");
    if (cat_tracks != p->n_tracks)
        return pfail(p, DAE_ERR_ARG, "dae_pipeline_set_catalogue: the catalogue was created over another number of track columns (n_tracks) "
                                     "than the pipeline ranks");
    if (p->has_title && p->dtype == DAE_DTYPE_BF16_EXACT)
        return pfail(p, DAE_ERR_ARG, "dae_pipeline_set_catalogue: a titled pipeline of DAE_DTYPE_BF16_EXACT does not rank inside a catalogue "
                                     "(dae_title_score_catalogue); create it with DAE_DTYPE_F32, the same lists");
    std::lock_guard<std::mutex> g(p->issue_mu);
    DeviceGuard dev_guard(p->device);
    const size_t rows = (size_t)p->group_rows, nz = (size_t)p->max_nnz;
    for (Slot& S : p->slots) {
        S.d_lrp = p->mem.dev<int32_t>(rows + 1); S.d_lcnt = p->mem.dev<int32_t>(rows); S.d_lscol = p->mem.dev<int32_t>(nz);
    }
    if (!p->mem.ok) return pfatal(p, DAE_ERR_NOMEM, "dae_pipeline_set_catalogue: allocation failed");
    p->cat = cat;
    for (Lane& L : p->lanes) PIPE_HIP(p, hipStreamSynchronize(L.stream));
    const char* msg = "";
    int rc = pipe_pack_images(p, p->dtype, IMG_BOTH, &msg);
    if (rc) return pfatal(p, rc, msg);
    PIPE_HIP(p, hipStreamSynchronize(p->lanes[0].stream));
    for (size_t i = 0; i < p->lanes.size(); ++i) {
        Lane& L = p->lanes[i];
        if (!rc && i > 0) rc = pipe_borrow_images(p, (int)i, p->dtype, IMG_BOTH, &msg);
        // (an fp32 image a lane needs later -- a guard re-run, a paused exact mix -- is then the catalogue's: pipe_ensure_f32)
        L.has_f32 = p->has_title && p->dtype == DAE_DTYPE_F32;
        L.t_has_f32 = L.has_f32;
    }
    if (rc) return pfatal(p, rc, msg);
    for (Lane& L : p->lanes) PIPE_HIP(p, hipStreamSynchronize(L.stream));
    return DAE_OK;
}

static int poll_impl(dae_pipeline* p, int wait, uint64_t* ticket, const int32_t** idx, const float** score,
                     const dae_metric_rec** rec, const float** cout, int64_t* n_out, int* n_rows, int* block)
{
    if (!p) return DAE_ERR_ARG;
    if ((!idx && !rec && !cout) || !n_rows || !block) return pfail(p, DAE_ERR_ARG, "null pointer");
    // candidates mode: the values of a scoring pipeline leave through dae_pipeline_poll_candidates, the lists of a ranking one
    // through dae_pipeline_poll
    if (cout && !(p->cand && !p->cand_rank))
        return pfail(p, DAE_ERR_STATE, p->cand ? "dae_pipeline_poll_candidates: a ranking candidates pipeline (rank = 1) hands out lists (dae_pipeline_poll)"
                                               : "dae_pipeline_poll_candidates: dae_pipeline_enable_candidates was not called");
    if (idx && p->cand && !p->cand_rank)
        return pfail(p, DAE_ERR_STATE, "dae_pipeline_poll: a scoring candidates pipeline (rank = 0) hands out values (dae_pipeline_poll_candidates)");
    if (p->eval != (rec != nullptr))
        return pfail(p, DAE_ERR_STATE, p->eval ? "dae_pipeline: an evaluation pipeline hands out records (dae_pipeline_poll_eval)"
                                               : "dae_pipeline_poll_eval: dae_pipeline_enable_eval was not called");
    std::unique_lock<std::mutex> lk(p->mu);
    *n_rows = 0; *block = -1;
    if (idx) *idx = nullptr;
    if (rec) *rec = nullptr;
    if (score) *score = nullptr;
    if (cout) { *cout = nullptr; *n_out = 0; }
    Slot& S = p->slots[p->poll_slot];
    if (S.state == 0) return p->err_code;                    // nothing pending (0 rows), or the worker's error
    if (S.state == 1) {
        if (!wait) return DAE_OK;
        const int rc = close_open(p);                        // the caller waits for a launch that is still open: close it
        if (rc) return rc;
    }
    if (S.state == 2) {
        if (!wait) return DAE_OK;
        p->cv_caller.wait(lk, [&] { return S.state == 3; });
    }
    if (p->err_code) return p->err_code;
    if (S.next_feed == 0) {                                  // first feed of the launch: its results have to be here
        lk.unlock();
        if (!wait) {
            if (*(const volatile int32_t*)(S.h_flags + 3) != S.seq) {                   // (no HIP call while the launch runs ...
                if ((++S.polls & 255) == 0) {                    // ... but a launch that faulted never writes its word: ask now and then)
                    const hipError_t q = pipe_launch_failed(S.ev_scored);
                    if (q != hipSuccess) { lk.lock(); return pfatal(p, DAE_ERR_HIP, hipGetErrorString(q)); }
                }
                return DAE_OK;
            }
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
        } else {
            const auto t_w = std::chrono::steady_clock::now();
            const hipError_t e = pipe_wait_launch(S);
            p->wait_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_w).count();
            if (e != hipSuccess) { lk.lock(); return pfatal(p, DAE_ERR_HIP, hipGetErrorString(e)); }
        }
        if (S.h_flags[0] != 0) {
            lk.lock();
            return pfatal(p, DAE_ERR_ARG, "dae_pipeline: a feed of the launch holds a column index out of range");
        }
        if (p->cand) {
            lk.lock();                                           // (the candidate chain is fp32 whatever the dtype: no guard to ask)
        } else if (S.titled && S.ran_dtype == DAE_DTYPE_BF16_EXACT && S.h_flags[1] != p->lanes[S.lane].guard_seen) {
            // the exact title mix (dae_mix_topk_exact): the title context's guard words moved under this launch -- a recomputed
            // logit left its promised interval (column >= 0), or rows hold more survivors than the refine launch lists (column
            // -2 / -3: scores no bound can tell apart; such rows came back without recommendations) -> the launch again on the
            // fp32 kernels.  Two overflow launches in a row pause the mode for 64 launches (a model whose rows keep
            // overflowing would otherwise pay both passes every time).
            const int rc = guard_rerun(p, S, lk, [&](Lane& L) {
                L.guard_seen = S.h_flags[1];
                if (S.h_flags[2] == -2 || S.h_flags[2] == -3) {
                    if (++p->overflow_streak >= 2) { p->exact_pause = 64; p->overflow_streak = 0; }
                } else {
                    p->overflow_streak = 0;
                }
                return DAE_OK;
            });
            if (rc) return rc;
        } else if (!S.titled && p->dtype == DAE_DTYPE_BF16_EXACT && S.h_flags[1] != 0) {
            // BOUND GUARD (include/dae_hip.h dae_exact_guard_read): a recomputed survivor left its promised interval, the
            // lists of this launch are unproven -> the same launch again on the fp32 kernels (guard_rerun)
            const int rc = guard_rerun(p, S, lk, [&](Lane& L) {
                int32_t nv = 0, col = -1;
                const int rc_g = dae_exact_guard_read(L.ctx, &nv, &col);       // (synchronises the lane, resets the words)
                return rc_g ? rc_g : pipe_ensure_f32(p, S.lane);
            });
            if (rc) return rc;
            S.h_flags[1] = 0;
        } else {
            if (S.titled && S.ran_dtype == DAE_DTYPE_BF16_EXACT) p->overflow_streak = 0;       // (only the caller's thread touches it here)
            lk.lock();
        }
    }
    const auto h = p->hand_out();                            // (the references, and behind a launch's last feed the ring)
    const OutBlock& ob = p->blocks[h.block];
    if (ticket) *ticket = h.feed.ticket;
    int rc_out = DAE_OK;
    if (rec) {
        *rec = ob.rec + h.feed.row0;
    } else if (cout) {
        *cout = ob.cand + h.feed.coff;
        *n_out = h.feed.n_cand;
        // the launch's status word came out with the block: an id outside -1 / [0, V) somewhere in the launch (its slot holds a NaN)
        if (*reinterpret_cast<const int32_t*>(ob.cand + p->max_candidates) != 0) rc_out = DAE_PIPE_BAD_ID;
    } else {
        *idx = ob.idx + (size_t)h.feed.row0 * p->k;
        if (score) *score = p->want_scores ? ob.score + (size_t)h.feed.row0 * p->k : nullptr;
    }
    *n_rows = h.feed.n_rows;
    *block = h.block;
    return rc_out;
}

int dae_pipeline_poll(dae_pipeline* p, int wait, uint64_t* ticket, const int32_t** idx, const float** score, int* n_rows,
                      int* block)
{
    if (p && !idx) return pfail(p, DAE_ERR_ARG, "null pointer");
    return poll_impl(p, wait, ticket, idx, score, nullptr, nullptr, nullptr, n_rows, block);
}

int dae_pipeline_poll_eval(dae_pipeline* p, int wait, uint64_t* ticket, const dae_metric_rec** rec, int* n_rows, int* block)
{
    if (p && !rec) return pfail(p, DAE_ERR_ARG, "null pointer");
    return poll_impl(p, wait, ticket, nullptr, nullptr, rec, nullptr, nullptr, n_rows, block);
}

int dae_pipeline_poll_candidates(dae_pipeline* p, int wait, uint64_t* ticket, const float** out, int64_t* n_out, int* n_rows, int* block)
{
    if (p && (!out || !n_out)) return pfail(p, DAE_ERR_ARG, "null pointer");
    return poll_impl(p, wait, ticket, nullptr, nullptr, nullptr, out, n_out, n_rows, block);
}

int dae_pipeline_release(dae_pipeline* p, int block)
{
    if (!p) return DAE_ERR_ARG;
    std::lock_guard<std::mutex> g(p->mu);
    if (const StageErr e = p->release(block)) return stage_fail(p, e);
    return DAE_OK;
}

int dae_pipeline_exact_margin(dae_pipeline* p, float scale)
{
    if (!p) return DAE_ERR_ARG;
    std::unique_lock<std::mutex> lk(p->mu);
    if (p->err_code) return p->err_code;
    if (p->dtype != DAE_DTYPE_BF16_EXACT) return pfail(p, DAE_ERR_ARG, "dae_pipeline_exact_margin: not an exact_bf16 pipeline");
    for (Slot& S : p->slots)
        if (S.state != 0) return pfail(p, DAE_ERR_STATE, "dae_pipeline_exact_margin: feeds are in flight");
    lk.unlock();
    std::lock_guard<std::mutex> g(p->issue_mu);
    DeviceGuard dev_guard(p->device);
    for (Lane& L : p->lanes) (void)hipStreamSynchronize(L.stream);
    // per image: the margin, lane 0's pack, the borrows -- the DAE's, then the title scorer's (alpha_c, beta_c scale with the margin)
    const char* msg = "";
    for (const int which : {IMG_DAE, IMG_TITLE}) {
        if (which == IMG_TITLE && !p->has_title) break;
        dae_ctx* c0 = which == IMG_DAE ? p->lanes[0].ctx : p->lanes[0].tctx;
        int rc = dae_set_exact_margin(c0, scale);
        if (rc) return pfail(p, rc, dae_last_error(c0));
        rc = pipe_pack_images(p, p->dtype, which, &msg);
        if (rc) return pfail(p, rc, msg);
        if (hipStreamSynchronize(p->lanes[0].stream) != hipSuccess) return pfatal(p, DAE_ERR_HIP, "prepack failed");
        for (size_t i = 1; i < p->lanes.size(); ++i) {
            rc = pipe_borrow_images(p, (int)i, p->dtype, which, &msg);
            if (rc) return pfail(p, rc, msg);
        }
    }
    if (p->has_title) { p->exact_pause = 0; p->overflow_streak = 0; }
    return DAE_OK;
}

int dae_pipeline_times(dae_pipeline* p, uint64_t out4[4])
{
    if (!p || !out4) return DAE_ERR_ARG;
    std::lock_guard<std::mutex> g(p->mu);
    out4[0] = p->issue_ns; out4[1] = p->idle_ns; out4[2] = p->submit_ns; out4[3] = p->wait_ns;
    return DAE_OK;
}

int dae_pipeline_stats(dae_pipeline* p, uint64_t out3[3])
{
    if (!p || !out3) return DAE_ERR_ARG;
    std::lock_guard<std::mutex> g(p->mu);
    out3[0] = p->launches; out3[1] = p->next_ticket - 1; out3[2] = p->guard_fallbacks;
    return DAE_OK;
}

}  // extern "C"
