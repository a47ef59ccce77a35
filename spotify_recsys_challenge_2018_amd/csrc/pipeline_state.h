// pipeline_state.h -- the streaming pipeline's state, private to its two units: pipeline.hip (the C ABI: the caller's thread) and
// pipeline_issue.hip (the library's threads and everything they enqueue).  The host half of a slot, the ring and the result
// blocks' counts come from pipeline_stage.h, which knows no device.
#pragma once
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>

#include "dae_internal.h"
#include "pipeline_stage.h"

namespace dae_pipe {

// The one owner of a pipeline's device buffers, pinned blocks and events: it records what it hands out and frees all of it in one
// place, in reverse order (dae_pipeline_destroy, after the threads are joined and the streams synchronised).  A failed allocation
// returns nullptr and clears `ok`: a group of allocations is written straight down and checked once.
struct PipeMem {
    struct Item { void* p; int kind; };                      // kind: 0 device, 1 pinned, 2 event
    std::vector<Item> items;
    bool ok = true;
    template <class T> T* dev(size_t count) { void* q = nullptr; return static_cast<T*>(keep(ok ? hipMalloc(&q, count * sizeof(T)) : hipErrorOutOfMemory, q, 0)); }
    template <class T> T* pinned(size_t count) { void* q = nullptr; return static_cast<T*>(keep(ok ? hipHostMalloc(&q, count * sizeof(T)) : hipErrorOutOfMemory, q, 1)); }
    hipEvent_t event() { hipEvent_t e = nullptr; return static_cast<hipEvent_t>(keep(ok ? hipEventCreateWithFlags(&e, hipEventDisableTiming) : hipErrorOutOfMemory, e, 2)); }
    template <class T> void give_back(T*& q)                 // one pinned block, early
    {
        for (size_t i = 0; i < items.size(); ++i)
            if (q && items[i].p == q) { release(items[i]); items.erase(items.begin() + (long)i); break; }
        q = nullptr;
    }
    void free_all() { while (!items.empty()) { release(items.back()); items.pop_back(); } }
    // elements of T that cover n of them with the byte count rounded up to 16
    template <class T> static size_t pad16(size_t n) { return (n * sizeof(T) + 15) / 16 * 16 / sizeof(T); }

private:
    void* keep(hipError_t e, void* q, int kind)
    {
        if (e != hipSuccess || !q) { ok = false; return nullptr; }
        items.push_back(Item{q, kind});
        return q;
    }
    static void release(const Item& it)
    {
        if (it.kind == 0) (void)hipFree(it.p);
        else if (it.kind == 1) (void)hipHostFree(it.p);
        else (void)hipEventDestroy(static_cast<hipEvent_t>(it.p));
    }
};

struct OutBlock : StageBlock {    // pinned result block of one launch: idx [rows][k] (+ score), handed out by pointer
    int32_t* idx = nullptr; float* score = nullptr;
    dae_metric_rec* rec = nullptr;                    // evaluation mode: the launch's [rows] records (idx is not kept then)
    float* cand = nullptr;                            // candidates mode, scores: [max_candidates] values, then the launch's status word
};

struct Lane {                     // a context + stream + the device buffers its launches reuse in stream order
    dae_ctx* ctx = nullptr;
    hipStream_t stream = nullptr;
    float* d_score = nullptr;     // scores nobody fetches
    bool has_f32 = false;         // (guard fallback) an fp32 image of its own
    // titled pipelines (dae_pipeline_create_titled): the title scorer's context on the same stream, its guard words as the
    // launch left them, the count the previous polled launch of this lane saw (the words are cumulative)
    dae_ctx* tctx = nullptr;
    int32_t* d_guard = nullptr;
    int32_t guard_seen = 0;
    bool t_has_f32 = false;
};

struct TitleW {                   // the title scorer's variables (caller-owned device arrays) and shapes
    const float *emb = nullptr, *conv_w = nullptr, *conv_b = nullptr, *out_WT = nullptr, *out_b = nullptr;
    int n_char = 0, E = 0, n_sizes = 0, F = 0, ld_feat = 0, L = 0;
    std::vector<int32_t> fs;
};

struct Slot : StageSlot {         // one launch: its staging (pipeline_stage.h) and what the device side of it needs
    int32_t* h_flags = nullptr;   // pinned: {csr status, guard violations, guard column, sequence word, "scored" word}
    int64_t* d_pos = nullptr; float* d_val = nullptr;      // the feed on the device (uploaded on the copy stream, ahead of the lane)
    // the launch's CSR and seed lists (plain launches), built on the PREP stream while the lane still scores its previous launch
    int32_t *d_rp = nullptr, *d_col = nullptr, *d_srp = nullptr, *d_scol = nullptr, *d_status = nullptr; float* d_cval = nullptr;
    // catalogue mode (dae_pipeline_set_catalogue): the launch's seed lists in the catalogue's LOCAL columns -- row pointers
    // [group_rows + 1], the rows' counts [group_rows], columns [max_nnz] -- written on the prep stream behind the seed lists.  They
    // belong to the slot, not to a context: the lane's previous launch may still be reading its own
    int32_t *d_lrp = nullptr, *d_lcnt = nullptr, *d_lscol = nullptr;
    float *t_h = nullptr, *t_feat = nullptr, *t_wt = nullptr, *t_wp = nullptr;   // titled: hidden rows, title features, mixing weights
    hipEvent_t ev_prep = nullptr;
    int32_t* d_idx = nullptr; float* d_score = nullptr;    // the launch's lists on the device (moved out on the OUT stream, round 6)
    int32_t* d_flags = nullptr;                            // {csr status, guard violations, guard column} as the launch left them
    hipEvent_t ev_scored = nullptr;                        // the scoring call's last kernel (the out stream waits for it)
    int32_t* d_titles = nullptr; float* d_use = nullptr;
    // evaluation mode (dae_pipeline_enable_eval): the answers on the device, and the records dae_rank_metrics leaves (the out
    // thread moves THEM, d_idx stays on the device)
    int32_t *d_arp = nullptr, *d_acol = nullptr;
    dae_metric_rec* d_rec = nullptr;
    // candidates mode (dae_pipeline_enable_candidates): the launch's candidate CSR on the device, the value per listed id (the
    // scores that go out, or the keys dae_rank_candidates ranks) and the candidate kernels' status word
    int32_t *d_crp = nullptr, *d_ccol = nullptr, *d_cstatus = nullptr;
    float* d_cout = nullptr;
    unsigned polls = 0;           // non-waiting polls of this issue that found its word missing (every 256th asks the runtime)
    int32_t seq = 0;              // the sequence word this launch's last kernel writes into h_flags[3] (the caller's wait watches it)
    int ran_dtype = 0;            // arithmetic the launch was issued with (a paused exact mode issues DAE_DTYPE_F32)
    hipEvent_t ev_h2d = nullptr, ev_gate = nullptr;
};

}  // namespace dae_pipe

struct dae_pipeline : dae_pipe::Stage<dae_pipe::Slot, dae_pipe::OutBlock> {     // (group_rows, max_nnz, max_answers, slots, blocks, tickets and the ring: the base)
    int device = 0, V = 0, H = 0, n_tracks = 0, dtype = 0, k = 0, want_scores = 0;
    const float *W_enc = nullptr, *b_enc = nullptr, *W_dec = nullptr, *b_dec = nullptr;
    dae_pipe::PipeMem mem;                  // every buffer and event below, of the lanes, the slots and the blocks
    std::vector<dae_pipe::Lane> lanes;
    // the feed -> CSR + seed lists of launch n + 1 on a stream (and library context) of their own: five small launches that are
    // independent of the lane's previous launch -- in the lane's stream they were 170 us of a 600 us chain (queued behind the
    // other lanes' decode workgroups, each takes 5 - 10 x its time alone: profiles/r06_notes.md)
    hipStream_t prep_stream = nullptr;
    dae_ctx* prep_ctx = nullptr;
    dae_ctx* prep_tctx = nullptr;         // titled pipelines: the title scorer's context of the prep stream (its convolution table)
    hipStream_t out_stream = nullptr;     // the lists' way out: the out thread's copies
    hipStream_t copy_stream = nullptr;    // uploads: hipMemcpyAsync on a stream that still has kernels queued blocks its caller
                                          // until they have run (measured: 0.43 ms per launch next to the fp32 decode) -- on a
                                          // stream of their own the uploads run ahead and the lane waits for their event
    std::mutex mu;                // states, queue, blocks
    std::mutex issue_mu;          // the lanes' contexts are used by one thread at a time (worker; poll's fp32 re-run)
    std::condition_variable cv_worker, cv_caller;
    std::deque<int> queue;        // slots waiting for the worker, in submission order
    std::thread worker;
    bool stop = false;
    // how a launch's lists reach the host (round 6, measured in profiles/r06_notes.md 5: M playlists/s through the loop, exact /
    // bf16): the copy ENGINE, driven by a thread of its own that makes no HIP call until the launch's "scored" word has arrived
    // (8.3 / 9.05).  Stores straight into the pinned block from the scoring call's last kernel (round 5) lost: 7.9 - 8.1 / 8.8,
    // that kernel sat on its CUs while the link took 4 MB.  (A 32-workgroup copy kernel on a stream of its own lost: 6.7 / 7.5.
    // Without any copy-out the loop runs at 9.9 / 11.4: the link is what the loop pays for.)
    std::thread out_worker;
    std::deque<int> out_queue;
    std::mutex out_mu;
    std::condition_variable cv_out;
    bool out_stop = false;
    std::mutex err_mu;            // err / err_code: written by the library thread and by the caller, read by dae_pipeline_last_error
    std::string err;
    int err_code = 0;
    hipEvent_t last_gate = nullptr;   // fp32, several lanes: the gate event of the launch issued before (dae_set_decode_gate)
    uint64_t guard_fallbacks = 0, launches = 0, seq_counter = 0;
    bool has_title = false;       // dae_pipeline_create_titled
    dae_pipe::TitleW tw;
    int exact_pause = 0, overflow_streak = 0;      // titled + exact: launches left on the fp32 kernels / overflow events in a row
    bool eval = false;            // dae_pipeline_enable_eval: feeds carry answers, records go out instead of lists
    bool cand = false;            // dae_pipeline_enable_candidates: feeds carry candidate ids; their scores, or the k best of them, go out
    int cand_rank = 0, cand_out_kind = 0;
    const dae_catalogue* cat = nullptr;   // dae_pipeline_set_catalogue: every launch ranks ITS columns (the caller keeps it alive)
    double* d_disc = nullptr;     // the caller's discount table [k]
    uint64_t issue_ns = 0, idle_ns = 0, submit_ns = 0, wait_ns = 0;      // where the host side of the loop spends its time (dae_pipeline_times)
};

namespace dae_pipe {

// pfail: an error of THIS call (message only; p null: the calling thread's message); pfatal: the pipeline is broken from here on
// (every later call returns it)
int pfail(dae_pipeline* p, int code, const char* msg);
int pfatal(dae_pipeline* p, int code, const char* msg);

// the calling thread's current device, put back when the call returns: the pipeline's entry points select ITS device for
// their HIP calls, and a multi-GPU process must not find its device changed behind its back
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) (void)hipSetDevice(dev); else prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

#define PIPE_HIP(p, expr)                                                                          \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            char _b[400];                                                                          \
            snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return pfatal((p), DAE_ERR_HIP, _b);                                                   \
        }                                                                                          \
    } while (0)

// pipeline_issue.hip, for pipeline.hip
enum { IMG_DAE = 1, IMG_TITLE = 2, IMG_BOTH = 3 };
int pipe_pack_images(dae_pipeline* p, int dtype, int which, const char** msg);      // (the caller synchronises lane 0)
int pipe_borrow_images(dae_pipeline* p, int lane, int dtype, int which, const char** msg);
int pipe_ensure_f32(dae_pipeline* p, int lane);
int pipe_issue(dae_pipeline* p, Slot& S, int dtype);
hipError_t pipe_launch_failed(hipEvent_t ev_scored);
hipError_t pipe_wait_launch(const Slot& S);
void pipe_worker_main(dae_pipeline* p);
void pipe_out_worker_main(dae_pipeline* p);

}  // namespace dae_pipe
