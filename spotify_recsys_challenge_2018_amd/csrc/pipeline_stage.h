// pipeline_stage.h -- the CALLER THREAD's half of the streaming pipeline (pipeline.hip): what dae_pipeline_submit*, _flush, _poll*
// and _release do that touches no device -- the feed checks, the fit test that closes a launch, the ring of launch slots, the
// staging copies with the rollback of a refused feed, the answers' and the candidates' CSR and the result blocks' reference counts.  Host arithmetic
// on host memory: no HIP, nothing of dae_internal.h, only the standard library (tests/host/pipeline_stage_main.cpp drives it
// without a device).  pipeline.hip calls these under its lock `mu`, except the copies, which run outside it (the worker never
// touches an open slot).  Everything is defined in the class, hence inline: the plain feed's copy stays one inlined pass.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

namespace dae_pipe {

enum { STAGE_OK = 0, STAGE_ARG, STAGE_STATE, STAGE_BUSY };
struct StageErr {                 // kind 0: fine; otherwise the message of the refusal
    int kind; const char* msg;
    explicit operator bool() const { return kind != STAGE_OK; }
};

struct Feed { uint64_t ticket; int row0, n_rows; int64_t coff = 0, n_cand = 0; };   // (coff, n_cand: candidates mode -- the feed's ids in the launch)

struct StageSlot {                // the host side of one launch from staging to its last polled feed; more slots than lanes, so that
    int64_t* h_pos = nullptr;     // the caller stages launch n + lanes while the lanes still score / hand out the ones before
    float* h_val = nullptr;       // (pinned staging of the feed: 32-bit (row, col) pairs of a plain launch, the int64 feed of a titled one)
    int32_t* h_titles = nullptr; float* h_use = nullptr;   // titled pipelines: [group_rows][L] characters, [group_rows] titles_use
    // evaluation mode: the launch's answers as a CSR over its rows, staged and uploaded with the feed
    int32_t *h_arp = nullptr, *h_acol = nullptr;
    int64_t n_ans = 0;
    // candidates mode: the launch's candidate ids as a CSR over its rows, staged and uploaded with the feed; its longest row
    int32_t *h_crp = nullptr, *h_ccol = nullptr;
    int64_t n_cand = 0;
    int cand_cap = 0;
    int titled = 0;               // this launch ranks the title-mixed score (its feeds came through dae_pipeline_submit_titled)
    int state = 0;                // 0 free, 1 staging (open launch), 2 queued for the worker, 3 issued
    int rows = 0; int64_t nnz = 0;
    int block = -1, lane = -1;
    std::vector<Feed> feeds;
    size_t next_feed = 0;         // first feed of the launch not handed out yet
};

struct StageBlock {
    int refs = 0;                 // feeds handed out and not yet released (+1 while its launch is pending)
};

struct Staged {                   // where begin() put a feed (coff, cap_before: begin_candidates())
    int slot; int row0; int64_t off, aoff; uint64_t ticket;
    int64_t coff = 0; int cap_before = 0;
};

template <class SlotT, class BlockT>
struct Stage {
    int group_rows = 0, title_len = 0;                      // the limits of one launch
    int64_t max_nnz = 0, max_answers = 0;
    int64_t max_candidates = 0;                             // candidates mode: the ids one launch may hold
    std::vector<SlotT> slots;
    std::vector<BlockT> blocks;
    uint64_t next_ticket = 1;
    int open_slot = -1;           // slot of the launch being staged
    int next_slot = 0;            // slots take the launches in ring order ...
    int poll_slot = 0;            // ... and are polled in the same order
    int n_lanes = 1, next_lane = 0;   // lanes take the launches in turn

    // what a feed must satisfy before anything is touched; *n_ans: its answers (0 without ans_rp)
    StageErr check_feed(bool eval, const int64_t* positions, const float* values, int64_t nnz, int n_rows, const int32_t* ans_rp,
                        const int32_t* ans_col, int64_t* n_ans) const
    {
        *n_ans = 0;
        if (eval != (ans_rp != nullptr))
            return {STAGE_STATE, eval ? "dae_pipeline: an evaluation pipeline takes dae_pipeline_submit_eval only"
                                      : "dae_pipeline_submit_eval: dae_pipeline_enable_eval was not called"};
        if (ans_rp && n_rows >= 1) {
            for (int r = 0; r < n_rows; ++r)
                if (ans_rp[r + 1] < ans_rp[r]) return {STAGE_ARG, "dae_pipeline_submit_eval: ans_row_ptr decreases"};
            *n_ans = (int64_t)ans_rp[n_rows] - ans_rp[0];
            if (*n_ans > max_answers || (*n_ans > 0 && !ans_col))
                return {STAGE_ARG, "dae_pipeline_submit_eval: a feed's answers must fit one launch (max_answers)"};
        }
        if (n_rows < 1 || n_rows > group_rows || nnz < 0 || nnz > max_nnz || (nnz > 0 && (!positions || !values)))
            return {STAGE_ARG, "dae_pipeline_submit: a feed must fit one launch (rows <= group_rows, nnz <= max_nnz)"};
        return {STAGE_OK, nullptr};
    }

    // a row index outside the feed would land in ANOTHER feed's rows of the launch: checked on the host (the device flags only
    // what leaves the launch).  Titled feeds: this pass of its own, before anything is staged; plain feeds: inside the narrowing
    // copy (ONE pass over the feed -- the caller's thread is what bounds the loop: 17 us of its 33 us per 256-row feed were these
    // two passes, round 6)
    static StageErr bad_row() { return {STAGE_ARG, "dae_pipeline_submit: a row index of the feed is outside [0, n_rows)"}; }
    static bool rows_inside(const int64_t* positions, int64_t nnz, int n_rows)
    {
        for (int64_t i = 0; i < nnz; ++i)
            if (positions[2 * i] < 0 || positions[2 * i] >= n_rows) return false;
        return true;
    }

    // does the feed still fit the open launch?  (a launch ranks EITHER the plain logits or the title-mixed score: feeds of the
    // other kind start a new one)
    bool fits_open(int n_rows, int64_t nnz, int titled, int64_t n_ans) const
    {
        const SlotT& O = slots[open_slot];
        return !(O.rows + n_rows > group_rows || O.nnz + nnz > max_nnz || O.titled != titled || O.n_ans + n_ans > max_answers);
    }
    // the next feed of this size would not fit the open launch's rows: off it goes
    bool open_is_full_for(int n_rows) const { return slots[open_slot].rows + n_rows > group_rows; }

    // close the open launch: a result block and a lane for it; *closed: the slot to hand to the worker
    StageErr close_launch(int* closed)
    {
        SlotT& S = slots[open_slot];
        int b = -1;
        for (size_t i = 0; i < blocks.size(); ++i) if (blocks[i].refs == 0) { b = (int)i; break; }
        if (b < 0) return {STAGE_BUSY, "dae_pipeline: every result block is still held by the caller (dae_pipeline_release)"};
        blocks[b].refs = 1;                                  // the launch's own reference, dropped when its last feed went out
        S.block = b;
        S.lane = next_lane;
        next_lane = (next_lane + 1) % n_lanes;
        S.state = 2;
        S.next_feed = 0;
        *closed = open_slot;
        open_slot = -1;
        return {STAGE_OK, nullptr};
    }

    // a place for the feed in the open launch (opening the next slot of the ring if none is open), and its ticket
    StageErr begin(int n_rows, int64_t nnz, int titled, int64_t n_ans, Staged* at)
    {
        if (open_slot < 0) {
            // the next slot of the ring; it is free once every feed of its previous launch has been handed out
            SlotT& N = slots[next_slot];
            if (N.state != 0) return {STAGE_BUSY, "dae_pipeline_submit: every launch slot holds results that were not polled "
                                                  "yet (poll before submitting more)"};
            open_slot = next_slot;
            next_slot = (next_slot + 1) % (int)slots.size();
            N.state = 1; N.rows = 0; N.nnz = 0; N.n_ans = 0; N.n_cand = 0; N.cand_cap = 0; N.feeds.clear(); N.next_feed = 0; N.titled = titled;
        }
        SlotT& S = slots[open_slot];
        *at = Staged{open_slot, S.rows, S.nnz, S.n_ans, next_ticket++};
        S.feeds.push_back(Feed{at->ticket, at->row0, n_rows});
        S.rows += n_rows; S.nnz += nnz; S.n_ans += n_ans;
        return {STAGE_OK, nullptr};
    }

    // a refused feed (the plain copy found a bad row): nothing of it stays, the slot and the ring are as before its begin()
    void rollback(const Staged& at, int n_rows, int64_t nnz, int64_t n_ans)
    {
        SlotT& S = slots[at.slot];
        S.feeds.pop_back(); S.rows -= n_rows; S.nnz -= nnz; S.n_ans -= n_ans; --next_ticket;
        if (S.feeds.empty()) { S.state = 0; next_slot = open_slot; open_slot = -1; }      // (it had opened the slot)
    }

    // the feed's (row, col) pairs into the launch's staging, rows shifted to their place in the launch.  false: a row index of a
    // PLAIN feed is outside [0, n_rows) (a titled feed's rows were checked before: rows_inside) -- roll the feed back
    bool copy_positions(const Staged& at, int titled, const int64_t* positions, int64_t nnz, int n_rows)
    {
        SlotT& S = slots[at.slot];
        const int row0 = at.row0;
        if (titled) {
            int64_t* dp = S.h_pos + 2 * at.off;
            if (row0 == 0) {
                if (nnz > 0) memcpy(dp, positions, (size_t)nnz * 2 * sizeof(int64_t));
            } else {
                for (int64_t i = 0; i < nnz; ++i) { dp[2 * i] = positions[2 * i] + row0; dp[2 * i + 1] = positions[2 * i + 1]; }
            }
            return true;
        }
        // 32-bit pairs: the row shifted to its place in the launch, a column that does not fit 32 bits becomes -1 (out of range for
        // the device's own check, like any column >= V); the row check of the feed rides along
        int32_t* dp = reinterpret_cast<int32_t*>(S.h_pos) + 2 * at.off;
        uint64_t bad = 0;
        const uint64_t nr = (uint64_t)n_rows;
        for (int64_t i = 0; i < nnz; ++i) {
            const int64_t r = positions[2 * i], c = positions[2 * i + 1];
            bad |= (uint64_t)((uint64_t)r >= nr);
            dp[2 * i] = (int32_t)((uint32_t)r + (uint32_t)row0);     // (a bad row's word is rolled back: let it wrap, not overflow)
            dp[2 * i + 1] = ((uint64_t)c > (uint64_t)INT32_MAX) ? -1 : (int32_t)c;
        }
        return bad == 0;
    }

    void copy_values(const Staged& at, const float* values, int values_broadcast, int64_t nnz)
    {
        if (nnz <= 0) return;                                    // (an empty feed may come without arrays)
        float* dv = slots[at.slot].h_val + at.off;
        if (values_broadcast) { const float v = values[0]; for (int64_t i = 0; i < nnz; ++i) dv[i] = v; }
        else memcpy(dv, values, (size_t)nnz * sizeof(float));
    }

    void copy_titles(const Staged& at, const int32_t* titles, const float* titles_use, int n_rows)
    {
        SlotT& S = slots[at.slot];
        memcpy(S.h_titles + (size_t)at.row0 * title_len, titles, (size_t)n_rows * title_len * sizeof(int32_t));
        memcpy(S.h_use + at.row0, titles_use, (size_t)n_rows * sizeof(float));
    }

    // the feed's answers behind the launch's, offsets in the launch's CSR
    void copy_answers(const Staged& at, const int32_t* ans_rp, const int32_t* ans_col, int n_rows, int64_t n_ans)
    {
        SlotT& S = slots[at.slot];
        const int32_t base = ans_rp[0];
        if (at.row0 == 0) S.h_arp[0] = 0;
        for (int r = 0; r < n_rows; ++r) S.h_arp[at.row0 + r + 1] = (int32_t)(at.aoff + (ans_rp[r + 1] - base));
        if (n_ans > 0) memcpy(S.h_acol + at.aoff, ans_col + base, (size_t)n_ans * sizeof(int32_t));
    }

    // ---- candidates mode (dae_pipeline_enable_candidates): every feed brings its candidate ids as a host CSR ------------------------
    // what the feed's candidates must satisfy before anything is touched; *n_cand: its ids, *longest: its longest row
    StageErr check_candidates(int n_rows, const int32_t* cand_rp, const int32_t* cand_col, int64_t* n_cand, int* longest) const
    {
        *n_cand = 0; *longest = 0;
        if (!cand_rp) return {STAGE_ARG, "dae_pipeline_submit_candidates: cand_row_ptr is null"};
        if (n_rows < 1 || n_rows > group_rows)
            return {STAGE_ARG, "dae_pipeline_submit: a feed must fit one launch (rows <= group_rows, nnz <= max_nnz)"};
        int64_t big = 0;
        for (int r = 0; r < n_rows; ++r) {
            const int64_t len = (int64_t)cand_rp[r + 1] - cand_rp[r];
            if (len < 0) return {STAGE_ARG, "dae_pipeline_submit_candidates: cand_row_ptr decreases"};
            if (len > big) big = len;
        }
        const int64_t n = (int64_t)cand_rp[n_rows] - cand_rp[0];
        if (n > max_candidates)
            return {STAGE_ARG, "dae_pipeline_submit_candidates: a feed's candidates must fit one launch (max_candidates); score "
                               "this feed per batch"};
        if (n > 0 && !cand_col) return {STAGE_ARG, "dae_pipeline_submit_candidates: cand_col is null"};
        *n_cand = n; *longest = (int)big;
        return {STAGE_OK, nullptr};
    }
    // would the feed's ids still fit the open launch?  (beside fits_open)
    bool cand_fits_open(int64_t n_cand) const { return slots[open_slot].n_cand + n_cand <= max_candidates; }
    // behind begin(): the feed's place in the launch's candidate CSR
    void begin_candidates(Staged* at, int64_t n_cand, int longest)
    {
        SlotT& S = slots[at->slot];
        at->coff = S.n_cand; at->cap_before = S.cand_cap;
        S.feeds.back().coff = S.n_cand; S.feeds.back().n_cand = n_cand;
        S.n_cand += n_cand;
        if (longest > S.cand_cap) S.cand_cap = longest;
    }
    // before rollback(): the refused feed's ids leave the launch's counts
    void rollback_candidates(const Staged& at, int64_t n_cand)
    {
        SlotT& S = slots[at.slot];
        S.n_cand -= n_cand; S.cand_cap = at.cap_before;
    }
    // the feed's candidates behind the launch's, row pointers in the launch's CSR (any base in, 0 out)
    void copy_candidates(const Staged& at, const int32_t* cand_rp, const int32_t* cand_col, int n_rows, int64_t n_cand)
    {
        SlotT& S = slots[at.slot];
        const int32_t base = cand_rp[0];
        if (at.row0 == 0) S.h_crp[0] = 0;
        for (int r = 0; r < n_rows; ++r) S.h_crp[at.row0 + r + 1] = (int32_t)(at.coff + (cand_rp[r + 1] - base));
        if (n_cand > 0) memcpy(S.h_ccol + at.coff, cand_col + base, (size_t)n_cand * sizeof(int32_t));
    }

    // the next feed of the launch at poll_slot goes out: the caller's reference to its block; behind the launch's last feed the
    // slot is free again and the ring moves on
    struct HandOut { Feed feed; int block; };
    HandOut hand_out()
    {
        SlotT& S = slots[poll_slot];
        BlockT& ob = blocks[S.block];
        const HandOut h{S.feeds[S.next_feed], S.block};
        ++ob.refs;                                               // the caller's reference to the block (dae_pipeline_release)
        if (++S.next_feed == S.feeds.size()) {                   // last feed of the launch: the slot is free again
            --ob.refs;                                           // (the launch's own reference)
            S.state = 0; S.block = -1;
            poll_slot = (poll_slot + 1) % (int)slots.size();
        }
        return h;
    }

    StageErr release(int block)
    {
        if (block < 0 || block >= (int)blocks.size() || blocks[block].refs <= 0)
            return {STAGE_ARG, "dae_pipeline_release: not a block that is out"};
        --blocks[block].refs;
        return {STAGE_OK, nullptr};
    }
};

}  // namespace dae_pipe
