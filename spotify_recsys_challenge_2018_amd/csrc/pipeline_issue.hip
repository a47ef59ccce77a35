// pipeline_issue.hip -- the streaming pipeline's own threads and everything they enqueue: the worker that issues every launch
// (pipe_issue: H2D, the feed -> CSR + seed lists, the scoring call, the flags' snapshot), the out thread that moves the lists,
// the images the lanes score with, and the wait on a launch's pinned word.  The C ABI is pipeline.hip.
#include "pipeline_state.h"

namespace dae_pipe {

// The caller's wait for a launch makes NO HIP call while the launch runs.  A thread inside hipEventSynchronize -- or asking
// hipEventQuery in a loop -- slows the library thread's enqueueing down (measured on the titled loop, one lane: 0.94 ms per
// launch = staging + issue + device + fetch one after the other, against 0.58 ms of kernels; a consumer that idled 80 us per
// feed OUTSIDE HIP made the loop faster; profiles/r05_notes.md).
// So a wait watches a pinned WORD without any HIP call -- the caller's the launch's SEQUENCE WORD, the last word the out thread
// writes into the slot's pinned flags, once the launch's lists and flags have arrived; the out thread's the "scored" word.
// (A failed launch never writes its word: pipe_launch_failed asks the runtime, every 1 024th spin.)
// ev_scored: recorded by pipe_issue() behind the scoring call on the lane's stream.  Complete but no word yet = the lists are on
// their way out: keep waiting
hipError_t pipe_launch_failed(hipEvent_t ev_scored)
{
    const hipError_t q = hipEventQuery(ev_scored);
    return q == hipErrorNotReady ? hipSuccess : q;
}

static hipError_t wait_word(const volatile int32_t* word, int32_t expect, hipEvent_t ev_scored)
{
    for (int spins = 0; *word != expect; ++spins) {
        if (spins < 200) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(20));
        if ((spins & 1023) == 1023) {
            const hipError_t q = pipe_launch_failed(ev_scored);
            if (q != hipSuccess) return q;
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return hipSuccess;
}

hipError_t pipe_wait_launch(const Slot& S) { return wait_word(S.h_flags + 3, S.seq, S.ev_scored); }

// {csr status, guard violations, guard column} as the launch's own stream leaves them -> the slot's device words (the lane's
// NEXT launch moves the cumulative guard words; the out stream reads this snapshot, not the live words)
namespace {
__global__ void flags_snapshot_kernel(int32_t* dst, const int32_t* status, const int32_t* guard, int32_t* scored_host, int32_t seq)
{
    if (threadIdx.x == 0) {
        dst[0] = status[0];
        dst[1] = guard ? guard[0] : 0;
        dst[2] = guard ? guard[1] : -1;
        if (scored_host) { __threadfence_system(); *scored_host = seq; }         // (the out thread watches this word)
    }
}
}  // namespace

// an image of `dtype` on a context that owns it (lane 0's): the vocabulary's columns, or in catalogue mode the catalogue's rows
// of the same arrays (W [V][ld], b [V]: the DAE's decoder, or the title scorer's Output_W^T / Output_b)
static int pack_image(dae_pipeline* p, dae_ctx* ctx, const float* W, const float* b, int ld, int dtype)
{
    return p->cat ? dae_prepack_decoder_catalogue(ctx, p->cat, W, b, p->V, ld, dtype)
                  : dae_prepack_decoder(ctx, W, b, p->V, ld, 0, p->V, dtype);
}

// Lane 0 packs the images of `dtype` the mask names -- the DAE's and, on a titled pipeline, the title scorer's; the caller
// synchronises lane 0's stream before the other lanes borrow them (pipe_borrow_images).  *msg: what failed, for the caller's own
// error class.
int pipe_pack_images(dae_pipeline* p, int dtype, int which, const char** msg)
{
    Lane& L0 = p->lanes[0];
    if (which & IMG_DAE) {
        const int rc = pack_image(p, L0.ctx, p->W_dec, p->b_dec, p->H, dtype);
        if (rc) { *msg = dae_last_error(L0.ctx); return rc; }
    }
    if ((which & IMG_TITLE) && p->has_title) {
        const int rc = pack_image(p, L0.tctx, p->tw.out_WT, p->tw.out_b, p->tw.ld_feat, dtype);
        if (rc) { *msg = dae_last_error(L0.tctx); return rc; }
    }
    return DAE_OK;
}

int pipe_borrow_images(dae_pipeline* p, int lane, int dtype, int which, const char** msg)
{
    Lane& L0 = p->lanes[0];
    Lane& L = p->lanes[lane];
    if (which & IMG_DAE) {
        const int rc = dae_share_decoder(L.ctx, L0.ctx, dtype);
        if (rc) { *msg = dae_last_error(L.ctx); return rc; }
    }
    if ((which & IMG_TITLE) && p->has_title) {
        const int rc = dae_share_decoder(L.tctx, L0.tctx, dtype);
        if (rc) { *msg = dae_last_error(L.tctx); return rc; }
    }
    return DAE_OK;
}

// fp32 images on a lane (the bound guard's fallback; a paused exact mode): the DAE's and, on a titled pipeline, the title
// scorer's -- lane 0 re-tiles them, the other lanes borrow lane 0's, each only once it needs them (issue_mu held)
int pipe_ensure_f32(dae_pipeline* p, int lane)
{
    Lane& L0 = p->lanes[0];
    Lane& L = p->lanes[lane];
    const char* msg = "";
    if (!L0.has_f32) {
        const int rc = pipe_pack_images(p, DAE_DTYPE_F32, IMG_DAE, &msg);
        if (rc) return pfatal(p, rc, msg);
        PIPE_HIP(p, hipStreamSynchronize(L0.stream));
        L0.has_f32 = true;
    }
    if (p->has_title && !L0.t_has_f32) {
        const int rc = pipe_pack_images(p, DAE_DTYPE_F32, IMG_TITLE, &msg);
        if (rc) return pfatal(p, rc, msg);
        PIPE_HIP(p, hipStreamSynchronize(L0.stream));
        L0.t_has_f32 = true;
    }
    const int borrow = (L.has_f32 ? 0 : IMG_DAE) | (p->has_title && !L.t_has_f32 ? IMG_TITLE : 0);
    if (lane != 0 && borrow) {
        const int rc = pipe_borrow_images(p, lane, DAE_DTYPE_F32, borrow, &msg);
        if (rc) return pfatal(p, rc, msg);
        L.has_f32 = true;
        L.t_has_f32 = p->has_title;
    }
    return DAE_OK;
}

// everything of one launch, asynchronously on its lane's stream (issue_mu held)
int pipe_issue(dae_pipeline* p, Slot& S, int dtype)
{
    Lane& L = p->lanes[S.lane];
    // (plain launches stage 32-bit (row, col) pairs -- the staging copy narrows them -- titled ones the int64 feed)
    PIPE_HIP(p, hipMemcpyAsync(S.d_pos, S.h_pos, (size_t)S.nnz * 2 * (S.titled ? sizeof(int64_t) : sizeof(int32_t)), hipMemcpyHostToDevice,
                               p->copy_stream));
    PIPE_HIP(p, hipMemcpyAsync(S.d_val, S.h_val, (size_t)S.nnz * sizeof(float), hipMemcpyHostToDevice, p->copy_stream));
    if (S.titled) {
        PIPE_HIP(p, hipMemcpyAsync(S.d_titles, S.h_titles, (size_t)S.rows * p->tw.L * sizeof(int32_t), hipMemcpyHostToDevice, p->copy_stream));
        PIPE_HIP(p, hipMemcpyAsync(S.d_use, S.h_use, (size_t)S.rows * sizeof(float), hipMemcpyHostToDevice, p->copy_stream));
    }
    if (p->eval) {
        PIPE_HIP(p, hipMemcpyAsync(S.d_arp, S.h_arp, (size_t)(S.rows + 1) * sizeof(int32_t), hipMemcpyHostToDevice, p->copy_stream));
        if (S.n_ans > 0)
            PIPE_HIP(p, hipMemcpyAsync(S.d_acol, S.h_acol, (size_t)S.n_ans * sizeof(int32_t), hipMemcpyHostToDevice, p->copy_stream));
    }
    if (p->cand) {
        PIPE_HIP(p, hipMemcpyAsync(S.d_crp, S.h_crp, (size_t)(S.rows + 1) * sizeof(int32_t), hipMemcpyHostToDevice, p->copy_stream));
        if (S.n_cand > 0)
            PIPE_HIP(p, hipMemcpyAsync(S.d_ccol, S.h_ccol, (size_t)S.n_cand * sizeof(int32_t), hipMemcpyHostToDevice, p->copy_stream));
    }
    PIPE_HIP(p, hipEventRecord(S.ev_h2d, p->copy_stream));
    if (p->dtype == DAE_DTYPE_F32 && p->lanes.size() > 1 && !p->cand) {       // (a candidates launch has no decode launch to gate)
        // the fp32 filter launch takes every CU, two of them in flight only queue behind each other: this launch's waits for
        // the one issued before it (on another lane) and announces its own end.  One event per launch SLOT: re-recording a
        // lane's event while its previous record was still pending made hipEventRecord wait for it (0.7 ms per launch).
        (void)dae_set_decode_gate(L.ctx, p->last_gate, S.ev_gate);
        p->last_gate = S.ev_gate;
    }
    int rc;
    S.ran_dtype = dtype;
    // NO DOWNLOADS from this thread: a hipMemcpyAsync device-to-host blocks its caller until everything queued before it has
    // run -- whichever stream it is put on (measured: on the lane's stream and on a fetch stream behind an event alike): the
    // library thread sat in those calls for the length of every launch and a second launch was never in flight
    // (0.77 of a titled launch's 0.9 ms of issue time; profiles/r05_notes.md).  The lists stay on the device; the out thread
    // moves them (pipe_out_worker_main).
    int32_t* const out_idx = S.d_idx;
    float* const out_score = p->want_scores ? S.d_score : L.d_score;     // (scores nobody fetches stay on the lane)
    const TitleW& t = p->tw;
    if (S.titled && dtype == DAE_DTYPE_F32 && !p->cand) { rc = pipe_ensure_f32(p, S.lane); if (rc) return rc; }
    // The half that does not depend on the lane's previous launch, on the PREP stream (contexts of its own), behind the upload;
    // the lane's stream only waits for its event.  Plain launches: the feed -> CSR and the seed lists (the playlist's own
    // tracks) in ONE group of four launches (round 6: six + a wider feed).  Titled ones (main_challenge.py:80-90 with DAE_title;
    // score.hip dae_title_prepare / _rank): title features, CSR + seed lists, hidden rows, mixing weights.
    dae_title_bufs tb;
    tb.rp = S.d_rp; tb.col = S.d_col; tb.srp = S.d_srp; tb.sc = S.d_scol; tb.val = S.d_cval;
    tb.h = S.t_h; tb.feat = S.t_feat; tb.wt = S.t_wt; tb.wp = S.t_wp;
    PIPE_HIP(p, hipStreamWaitEvent(p->prep_stream, S.ev_h2d, 0));
    rc = S.titled ? dae_title_prepare(p->prep_tctx, p->prep_ctx, S.d_pos, S.d_val, 0, S.nnz, S.rows, p->V, p->W_enc, p->b_enc, p->H,
                                      S.d_titles, t.L, t.emb, t.n_char, t.E, t.conv_w, t.conv_b, t.fs.data(), t.n_sizes, t.F, t.ld_feat,
                                      S.d_use, p->n_tracks, tb, S.d_status)
                  : dae_launch_coo32_to_csr_seeds(p->prep_ctx, reinterpret_cast<const int32_t*>(S.d_pos), S.d_val, 0, S.nnz, S.rows, p->V,
                                                  S.d_rp, S.d_col, S.d_cval, S.d_status, p->n_tracks, S.d_srp, S.d_scol);
    if (rc) return pfatal(p, rc, dae_last_error(S.titled ? p->prep_tctx : p->prep_ctx));
    if (p->cat) {
        // catalogue mode: the seed lists into the catalogue's columns, still on the prep stream (they depend on the feed alone; the
        // launch's nnz bounds its seeds: nothing is written at or past it); the lane ranks the catalogue's images and maps the
        // lists back (catalogue.hip)
        rc = dae_catalogue_translate_seeds(p->prep_ctx, p->cat, S.d_srp, S.d_scol, S.rows, (int)S.nnz, S.d_lrp, S.d_lcnt, S.d_lscol);
        if (rc) return pfatal(p, rc, dae_last_error(p->prep_ctx));
        tb.srp = S.d_lrp; tb.sc = S.d_lscol;
    }
    PIPE_HIP(p, hipEventRecord(S.ev_prep, p->prep_stream));
    PIPE_HIP(p, hipStreamWaitEvent(L.stream, S.ev_prep, 0));
    if (p->cand) {
        // candidates mode: the value of every listed (row, column) -- fp32 chains over the model's row-major tensors whatever the
        // pipeline's dtype, no packed image -- in the order of the launch's candidate CSR; a ranking pipeline drops a row's repeated
        // columns first (in place: the upload is this launch's own) and ranks the values behind them: the logits (plain) or the
        // mixed values (titled: DAE_OUT_LOGIT, so that out_score holds y), seeds = the playlist's own tracks
        const int nc = (int)S.n_cand;
        PIPE_HIP(p, hipMemsetAsync(S.d_cstatus, 0, sizeof(int32_t), L.stream));
        if (p->cand_rank) {
            rc = dae_candidates_unique(L.ctx, S.rows, p->V, S.d_crp, S.d_ccol, S.d_ccol, nc);
            if (rc) return pfatal(p, rc, dae_last_error(L.ctx));
        }
        if (S.titled) {
            rc = dae_mix_candidates(L.tctx, L.ctx, S.t_h, p->H, p->H, p->W_dec, p->b_dec, S.t_feat, t.ld_feat, t.out_WT, t.out_b, S.t_wt,
                                    S.t_wp, S.rows, p->V, S.d_crp, S.d_ccol, nc, S.d_cout, S.d_cstatus);
            if (rc) return pfatal(p, rc, dae_last_error(L.tctx));
        } else {
            rc = dae_score_candidates(L.ctx, S.d_rp, S.d_col, S.d_cval, p->W_enc, p->b_enc, p->V, p->H, S.rows, p->W_dec, p->b_dec, S.d_crp,
                                      S.d_ccol, nc, p->cand_rank ? DAE_OUT_LOGIT : p->cand_out_kind, S.d_cout, S.d_cstatus);
            if (rc) return pfatal(p, rc, dae_last_error(L.ctx));
        }
        if (p->cand_rank) {
            rc = dae_rank_candidates(L.ctx, S.rows, p->V, S.d_crp, S.d_ccol, S.d_cout, S.cand_cap, S.d_srp, S.d_scol, p->k,
                                     S.titled ? DAE_OUT_LOGIT : p->cand_out_kind, out_score, out_idx);
            if (rc) return pfatal(p, rc, dae_last_error(L.ctx));
        }
    } else if (S.titled) {
        rc = p->cat ? dae_title_rank_catalogue(L.tctx, L.ctx, dtype, S.rows, p->H, t.ld_feat, tb, p->cat, p->k, out_score, out_idx, L.d_guard)
                    : dae_title_rank(L.tctx, L.ctx, dtype, S.rows, p->V, p->H, t.ld_feat, tb, p->n_tracks, p->k, out_score, out_idx, L.d_guard);
        if (rc) return pfatal(p, rc, dae_last_error(L.tctx));
    } else {
        rc = p->cat ? dae_score_topk_catalogue_local(L.ctx, S.d_rp, S.d_col, S.d_cval, p->W_enc, p->b_enc, p->V, p->H, S.rows, dtype, p->cat,
                                                     S.d_lrp, S.d_lscol, p->k, DAE_OUT_SCORE, out_score, out_idx)
                    : dae_score_topk(L.ctx, S.d_rp, S.d_col, S.d_cval, p->W_enc, p->b_enc, p->V, p->H, S.rows, dtype, p->n_tracks,
                                     S.d_srp, S.d_scol, p->k, DAE_OUT_SCORE, out_score, out_idx);
        if (rc) return pfatal(p, rc, dae_last_error(L.ctx));
    }
    if (p->eval) {
        // the rows' metrics from the lists where they are (the answers came up with the feed: ev_h2d -> ev_prep -> this stream).
        // A guard re-run comes through here again, so its records are the fp32 lists'.  Catalogue mode: the lists have been
        // mapped back, candidates and answers are both global columns (an answer outside the catalogue is never hit and counts
        // in the denominators, as a -1 answer does).
        rc = dae_rank_metrics(L.ctx, out_idx, p->k, S.rows, p->k, S.d_arp, S.d_acol, p->d_disc, S.d_rec);
        if (rc) return pfatal(p, rc, dae_last_error(L.ctx));
    }
    // The small words first pass through one device block (flags: status, guard words), so the out thread's copies of a
    // launch are two or three.
    const int32_t* gw = nullptr;                             // the guard words as this launch left them (titled fp32: zeros)
    if (p->cand) {
        // (no bound to guard: fp32 chains)
    } else if (S.titled) {
        gw = L.d_guard;
    } else if (dtype == DAE_DTYPE_BF16_EXACT) {
        rc = dae_exact_guard_words(L.ctx, &gw);
        if (rc) return pfatal(p, rc, dae_last_error(L.ctx));
    }
    // (odd, hence never 0 -- the word's idle value -- and different for every issue: a guard fallback re-issues a slot right
    // after its first issue, whose word is still in h_flags[3]; the counter wraps after 2^30 launches)
    S.seq = (int32_t)(((++p->seq_counter << 1) | 1u) & 0x7FFFFFFFu);
    S.polls = 0;
    hipLaunchKernelGGL(flags_snapshot_kernel, dim3(1), dim3(64), 0, L.stream, S.d_flags, S.d_status, gw,
                       S.h_flags + 4, S.seq);
    PIPE_HIP(p, hipGetLastError());
    PIPE_HIP(p, hipEventRecord(S.ev_scored, L.stream));
    // the copy engine, from the out thread: nothing more to enqueue here
    {
        std::lock_guard<std::mutex> g(p->out_mu);
        p->out_queue.push_back((int)(&S - p->slots.data()));
    }
    p->cv_out.notify_one();
    return DAE_OK;
}

// The out thread: the lists of every issued launch, in issue order, through the copy engine.  The thread makes no HIP call until the
// launch's "scored" word (written by flags_snapshot_kernel, the scoring call's last kernel) has arrived -- a thread parked inside
// hipEventSynchronize slowed the issuing thread's enqueueing down (profiles/r05_notes.md) -- then three asynchronous copies on the
// out stream (nothing is queued there: they do not block), one synchronize, and the sequence word the caller's wait watches.
void pipe_out_worker_main(dae_pipeline* p)
{
    (void)hipSetDevice(p->device);
    for (;;) {
        int si;
        {
            std::unique_lock<std::mutex> lk(p->out_mu);
            p->cv_out.wait(lk, [&] { return p->out_stop || !p->out_queue.empty(); });
            if (p->out_queue.empty()) return;                // (stop, and nothing left to move)
            si = p->out_queue.front();
            p->out_queue.pop_front();
        }
        Slot& S = p->slots[si];
        const int32_t seq = S.seq;
        hipError_t e = wait_word(S.h_flags + 4, seq, S.ev_scored);
        const OutBlock& ob = p->blocks[S.block];
        const size_t nb = (size_t)S.rows * p->k;
        if (p->eval) {
            // the records instead of the lists; the out stream is ordered behind the launch by its event (already complete when
            // the word is seen, so the wait costs nothing and the copies do not rest on the kernel-end write-back alone)
            if (e == hipSuccess) e = hipStreamWaitEvent(p->out_stream, S.ev_scored, 0);
            if (e == hipSuccess) e = hipMemcpyAsync(ob.rec, S.d_rec, (size_t)S.rows * sizeof(dae_metric_rec), hipMemcpyDeviceToHost, p->out_stream);
        } else if (p->cand && !p->cand_rank) {
            // the values instead of the lists, and the candidate kernels' status word behind the block's values
            if (e == hipSuccess) e = hipStreamWaitEvent(p->out_stream, S.ev_scored, 0);
            if (e == hipSuccess && S.n_cand > 0)
                e = hipMemcpyAsync(ob.cand, S.d_cout, (size_t)S.n_cand * sizeof(float), hipMemcpyDeviceToHost, p->out_stream);
            if (e == hipSuccess)
                e = hipMemcpyAsync(ob.cand + p->max_candidates, S.d_cstatus, sizeof(int32_t), hipMemcpyDeviceToHost, p->out_stream);
        } else {
            if (e == hipSuccess) e = hipMemcpyAsync(ob.idx, S.d_idx, nb * sizeof(int32_t), hipMemcpyDeviceToHost, p->out_stream);
            if (e == hipSuccess && p->want_scores) e = hipMemcpyAsync(ob.score, S.d_score, nb * sizeof(float), hipMemcpyDeviceToHost, p->out_stream);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(S.h_flags, S.d_flags, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, p->out_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(p->out_stream);
        if (e != hipSuccess) {
            (void)pfatal(p, DAE_ERR_HIP, hipGetErrorString(e));
            // (the caller's wait ends on the word all the same: it finds err_code set)
        }
        __atomic_thread_fence(__ATOMIC_RELEASE);
        *(volatile int32_t*)(S.h_flags + 3) = seq;
    }
}

void pipe_worker_main(dae_pipeline* p)
{
    (void)hipSetDevice(p->device);
    std::unique_lock<std::mutex> lk(p->mu);
    for (;;) {
        const auto t_idle = std::chrono::steady_clock::now();
        p->cv_worker.wait(lk, [&] { return p->stop || !p->queue.empty(); });
        p->idle_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_idle).count();
        if (p->stop && p->queue.empty()) return;
        const int si = p->queue.front();
        p->queue.pop_front();
        Slot& S = p->slots[si];
        const bool broken = p->err_code != 0;
        lk.unlock();
        const auto t_iss = std::chrono::steady_clock::now();
        if (!broken) {                                       // after an error: drain without touching the device
            std::lock_guard<std::mutex> g(p->issue_mu);
            int dt = p->dtype;
            if (S.titled && dt == DAE_DTYPE_BF16_EXACT && p->exact_pause > 0) { --p->exact_pause; dt = DAE_DTYPE_F32; }
            (void)pipe_issue(p, S, dt);
        }
        lk.lock();
        p->issue_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_iss).count();
        S.state = 3;
        ++p->launches;
        p->cv_caller.notify_all();
    }
}

}  // namespace dae_pipe
