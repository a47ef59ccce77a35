// Stand-alone program (no device, no HIP): the candidate staging of the streaming pipeline's candidates mode, csrc/pipeline_stage.h,
// driven in the order pipeline.hip's submit_impl / flush / poll / release drive it (minus the locks and the worker: a queued launch
// is marked issued by hand) against a straightforward model -- concatenate the candidate ids of a launch's feeds, rebase the row
// pointers.  Every staging buffer is a heap block of exactly the size dae_pipeline_enable_candidates gives it, so a write past a
// launch's limits is a heap overflow under -fsanitize=address.  Exits 0 and prints "all checks passed".
#include <stdio.h>

#include <deque>
#include <memory>
#include <string>

#include "pipeline_stage.h"

using namespace dae_pipe;

namespace {

int g_failed = 0, g_checks = 0;
void check(bool ok, const std::string& what)
{
    ++g_checks;
    if (!ok && ++g_failed <= 20) printf("FAILED: %s\n", what.c_str());
}

struct FeedIn {                   // one feed as a caller passes it: two entries per row, and its candidates
    std::vector<int64_t> pos; std::vector<float> val; int n_rows = 0;
    std::vector<int32_t> crp, ccol;
    int64_t nnz() const { return (int64_t)pos.size() / 2; }
};

struct Launch { std::vector<int32_t> crp{0}, ccol; std::vector<Feed> feeds; int cap = 0; };      // the model of a launch

struct Rig {
    Stage<StageSlot, StageBlock> st;
    std::deque<int> queue;
    std::vector<std::unique_ptr<char[]>> heap;
    std::vector<Launch> model;
    std::vector<std::vector<int>> closed;                    // every closed launch's feed sizes (rows), in order
    std::vector<int64_t> closed_ids;                         // ... and its candidate ids

    template <class T> T* block(size_t count) { heap.emplace_back(new char[count * sizeof(T)]); return reinterpret_cast<T*>(heap.back().get()); }
    Rig(int group_rows, int64_t max_nnz, int lanes, int64_t max_candidates, int blocks = 0)
    {
        st.group_rows = group_rows; st.max_nnz = max_nnz; st.max_candidates = max_candidates; st.n_lanes = lanes;
        st.slots.resize(2 * lanes + 2);
        st.blocks.resize(blocks > 0 ? blocks : (int)st.slots.size());
        model.resize(st.slots.size());
        for (StageSlot& S : st.slots) {                      // the sizes of pipeline_create / dae_pipeline_enable_candidates
            S.h_pos = block<int64_t>((size_t)max_nnz * 2);
            S.h_val = block<float>((size_t)max_nnz);
            S.h_crp = block<int32_t>((size_t)group_rows + 1);
            S.h_ccol = block<int32_t>((size_t)max_candidates);
        }
    }
    int close_open()
    {
        if (st.open_slot < 0) return STAGE_OK;
        int si = -1;
        if (const StageErr e = st.close_launch(&si)) return e.kind;
        queue.push_back(si);
        std::vector<int> sizes;
        for (const Feed& f : st.slots[si].feeds) sizes.push_back(f.n_rows);
        closed.push_back(sizes);
        closed_ids.push_back(st.slots[si].n_cand);
        return STAGE_OK;
    }
    // submit_impl of pipeline.hip on a candidates pipeline, call for call
    int submit(const FeedIn& f, uint64_t* ticket = nullptr)
    {
        const int64_t nnz = f.nnz();
        int64_t n_ans = 0, n_cand = 0;
        int longest = 0;
        const int32_t* crp = f.crp.empty() ? nullptr : f.crp.data();
        if (const StageErr e = st.check_candidates(f.n_rows, crp, f.ccol.data(), &n_cand, &longest)) return e.kind;
        if (const StageErr e = st.check_feed(false, f.pos.data(), f.val.data(), nnz, f.n_rows, nullptr, nullptr, &n_ans)) return e.kind;
        if (st.open_slot >= 0 && (!st.fits_open(f.n_rows, nnz, 0, n_ans) || !st.cand_fits_open(n_cand))) {
            const int rc = close_open();
            if (rc) return rc;
        }
        Staged at;
        if (const StageErr e = st.begin(f.n_rows, nnz, 0, n_ans, &at)) return e.kind;
        st.begin_candidates(&at, n_cand, longest);
        if (!st.copy_positions(at, 0, f.pos.data(), nnz, f.n_rows)) {
            st.rollback_candidates(at, n_cand);
            st.rollback(at, f.n_rows, nnz, n_ans);
            return st.bad_row().kind;
        }
        st.copy_values(at, f.val.data(), 0, nnz);
        st.copy_candidates(at, crp, f.ccol.data(), f.n_rows, n_cand);
        if (ticket) *ticket = at.ticket;
        Launch& M = model[at.slot];
        if (at.row0 == 0) M = Launch();
        Feed mf{at.ticket, at.row0, f.n_rows};
        mf.coff = (int64_t)M.ccol.size(); mf.n_cand = n_cand;
        for (int r = 0; r < f.n_rows; ++r) {
            const int len = crp[r + 1] - crp[r];
            M.crp.push_back(M.crp.back() + len);
            if (len > M.cap) M.cap = len;
        }
        for (int64_t a = 0; a < n_cand; ++a) M.ccol.push_back(f.ccol[crp[0] + a]);
        M.feeds.push_back(mf);
        const int slot = at.slot;
        if (st.open_is_full_for(f.n_rows)) (void)close_open();
        verify(slot, "after submit");
        return STAGE_OK;
    }
    void verify(int si, const char* when)
    {
        const StageSlot& S = st.slots[si];
        const Launch& M = model[si];
        const std::string w = std::string(when) + ", slot " + std::to_string(si) + ": ";
        bool ok = S.feeds.size() == M.feeds.size() && S.n_cand == (int64_t)M.ccol.size() && S.cand_cap == M.cap;
        int rows = 0;
        for (size_t i = 0; ok && i < M.feeds.size(); ++i) {
            ok = S.feeds[i].ticket == M.feeds[i].ticket && S.feeds[i].row0 == rows && S.feeds[i].n_rows == M.feeds[i].n_rows &&
                 S.feeds[i].coff == M.feeds[i].coff && S.feeds[i].n_cand == M.feeds[i].n_cand;
            rows += M.feeds[i].n_rows;
        }
        check(ok && S.rows == rows, w + "counts, longest row, per-feed offsets and tickets");
        if (!ok) return;
        bool csr = true;
        if (rows > 0) for (int r = 0; r <= rows; ++r) csr = csr && S.h_crp[r] == M.crp[r];
        for (size_t i = 0; i < M.ccol.size(); ++i) csr = csr && S.h_ccol[i] == M.ccol[i];
        check(csr, w + "the launch's candidate CSR");
    }
    void issue_all() { for (int si : queue) st.slots[si].state = 3; queue.clear(); }
    bool poll(bool release_it, Feed* feed = nullptr, int* block = nullptr)
    {
        const StageSlot& S = st.slots[st.poll_slot];
        if (S.state != 3) return false;
        const auto h = st.hand_out();
        if (feed) *feed = h.feed;
        if (block) *block = h.block;
        if (release_it) check(!st.release(h.block), "release of a block that is out");
        return true;
    }
};

// a feed of n_rows rows with `per_row` candidates each (ids tell the feed and the slot apart), behind `lead` foreign ids
FeedIn make_feed(int id, int n_rows, int per_row, int lead = 0)
{
    FeedIn f;
    f.n_rows = n_rows;
    for (int i = 0; i < n_rows * 2; ++i) { f.pos.push_back(i % n_rows); f.pos.push_back(id * 100 + i); f.val.push_back(1.0f); }
    for (int i = 0; i < lead; ++i) f.ccol.push_back(-777);
    f.crp.push_back(lead);
    for (int r = 0; r < n_rows; ++r) {
        for (int a = 0; a < per_row; ++a) f.ccol.push_back(id * 1000 + r * 10 + a);
        f.crp.push_back((int32_t)f.ccol.size());
    }
    return f;
}

void test_capacity()
{
    // 10 ids a row, max_candidates 1000, rows never close a launch (group_rows 4096): a launch closes exactly when the next
    // feed's ids would pass max_candidates -- 40 + 40 rows fit (800), + 30 would be 1100; 30 + 70 = 1000 fits exactly
    Rig R(4096, 1 << 16, 2, 1000);
    const int rows[] = {40, 40, 30, 70, 1, 100};
    for (int i = 0; i < 6; ++i) check(R.submit(make_feed(i, rows[i], 10)) == STAGE_OK, "capacity: feed taken");
    check(R.close_open() == STAGE_OK, "capacity: flush");
    const std::vector<std::vector<int>> want = {{40, 40}, {30, 70}, {1}, {100}};
    check(R.closed == want, "capacity: launches close on candidate capacity");
    check(R.closed_ids == std::vector<int64_t>({800, 1000, 10, 1000}), "capacity: ids per launch");
    // rows close a launch as before: group_rows 64, few ids
    Rig Q(64, 1 << 16, 2, 1000);
    const int qrows[] = {30, 30, 30, 4, 60};
    for (int i = 0; i < 5; ++i) check(Q.submit(make_feed(i, qrows[i], 1)) == STAGE_OK, "capacity: feed taken (rows)");
    check(Q.close_open() == STAGE_OK, "capacity: flush (rows)");
    const std::vector<std::vector<int>> qwant = {{30, 30}, {30, 4}, {60}};
    check(Q.closed == qwant, "capacity: launches close on rows");
}

void test_offsets()
{
    Rig R(64, 1 << 12, 1, 200);
    FeedIn a = make_feed(1, 3, 4, 5);                        // a row pointer that starts at 5
    a.crp = {5, 9, 9, 17};                                   // an empty row, a longer one
    FeedIn z = make_feed(2, 2, 0);                           // no candidates at all
    FeedIn zn = z;
    zn.ccol.clear();                                         // ... and no array for them
    FeedIn b = make_feed(3, 2, 3);
    check(R.submit(a) == STAGE_OK && R.submit(z) == STAGE_OK && R.submit(zn) == STAGE_OK && R.submit(b) == STAGE_OK, "offsets: feeds taken");
    const StageSlot& S = R.st.slots[0];
    const int32_t want_rp[] = {0, 4, 4, 12, 12, 12, 12, 12, 15, 18};
    check(!memcmp(S.h_crp, want_rp, sizeof(want_rp)), "offsets: rebased to 0, each feed's pointers continue the launch's");
    check(S.n_cand == 18 && S.cand_cap == 8 && S.h_ccol[0] == a.ccol[5] && S.h_ccol[12] == b.ccol[0], "offsets: ids behind each other, longest row");
    check(S.feeds[0].coff == 0 && S.feeds[0].n_cand == 12 && S.feeds[1].coff == 12 && S.feeds[1].n_cand == 0 && S.feeds[2].n_cand == 0 &&
          S.feeds[3].coff == 12 && S.feeds[3].n_cand == 6, "offsets: per-feed offsets; a feed with zero candidates is accepted");
    check(R.close_open() == STAGE_OK, "offsets: flush");
    R.issue_all();
    Feed f;
    int64_t at = 0;
    for (int i = 0; i < 4; ++i) {
        check(R.poll(true, &f) && f.coff == at, "offsets: the feeds go out with their offsets");
        at += f.n_cand;
    }
}

void test_refusals()
{
    Rig R(64, 1 << 12, 1, 100);
    check(R.submit(make_feed(0, 4, 5)) == STAGE_OK && R.submit(make_feed(1, 3, 2)) == STAGE_OK, "refusals: two feeds");
    const StageSlot& S = R.st.slots[0];
    const std::vector<int32_t> rp(S.h_crp, S.h_crp + 8), ids(S.h_ccol, S.h_ccol + 26);
    auto unchanged = [&](const std::string& tag) {
        check(S.rows == 7 && S.nnz == 14 && S.n_cand == 26 && S.cand_cap == 5 && S.feeds.size() == 2 && R.st.next_ticket == 3 &&
              R.st.open_slot == 0 && R.st.next_slot == 1 && S.state == 1, tag + ": the ring and the counts are as they were");
        check(!memcmp(rp.data(), S.h_crp, rp.size() * 4) && !memcmp(ids.data(), S.h_ccol, ids.size() * 4), tag + ": nothing staged");
        R.verify(0, tag.c_str());
    };
    check(R.submit(make_feed(2, 11, 10)) == STAGE_ARG, "refusals: more ids than max_candidates in one feed");
    unchanged("too many ids");
    FeedIn d = make_feed(3, 3, 4);
    d.crp = {0, 8, 4, 12};
    check(R.submit(d) == STAGE_ARG, "refusals: a descending cand_row_ptr");
    unchanged("descending row_ptr");
    FeedIn n = make_feed(4, 2, 4);
    n.crp = {8, 4, 0};                                       // negative counts throughout
    check(R.submit(n) == STAGE_ARG, "refusals: negative counts");
    unchanged("negative counts");
    FeedIn c = make_feed(5, 2, 4);
    int64_t nc = 0; int lg = 0;
    check(R.st.check_candidates(2, c.crp.data(), nullptr, &nc, &lg).kind == STAGE_ARG, "refusals: ids without cand_col");
    check(R.st.check_candidates(2, nullptr, c.ccol.data(), &nc, &lg).kind == STAGE_ARG, "refusals: no cand_row_ptr");
    FeedIn w = make_feed(6, 65, 1);
    check(R.submit(w) == STAGE_ARG, "refusals: more rows than group_rows");
    unchanged("too many rows");
    // a bad row index of the feed itself is found by the staging copy, AFTER begin(): the candidates are rolled back with it
    FeedIn p = make_feed(7, 6, 9);
    p.pos[2 * 3] = 6;
    check(R.submit(p) == STAGE_ARG, "refusals: a row index outside the feed");
    unchanged("bad row");
    uint64_t t = 0;
    check(R.submit(make_feed(8, 2, 7), &t) == STAGE_OK && t == 3 && S.n_cand == 40 && S.cand_cap == 7 && S.h_crp[9] == 40,
          "refusals: the pipeline takes the next feed where the refused ones would have gone");
    // ... and as the first feed of a launch the slot is free again
    Rig Q(8, 1 << 12, 1, 100);
    FeedIn q = make_feed(9, 4, 3);
    q.pos[0] = -1;
    check(Q.submit(q) == STAGE_ARG && Q.st.open_slot == -1 && Q.st.next_slot == 0 && Q.st.slots[0].state == 0 && Q.st.slots[0].n_cand == 0 &&
          Q.st.slots[0].cand_cap == 0 && Q.st.next_ticket == 1, "refusals: a refused first feed leaves its slot free");
    check(Q.submit(make_feed(10, 4, 3), &t) == STAGE_OK && t == 1 && Q.st.open_slot == 0, "refusals: and the next feed opens it");
}

void test_blocks()
{
    Rig R(16, 1 << 10, 1, 64, 4);                            // 4 slots, 4 blocks
    check(R.submit(make_feed(0, 4, 2)) == STAGE_OK && R.submit(make_feed(1, 4, 3)) == STAGE_OK && R.close_open() == STAGE_OK, "blocks: a launch of two feeds");
    check(R.st.slots[0].block == 0 && R.st.blocks[0].refs == 1, "blocks: the launch's own reference");
    R.issue_all();
    int b0 = -1, b1 = -1;
    Feed f0, f1;
    check(R.poll(false, &f0, &b0) && R.st.blocks[0].refs == 2 && R.st.slots[0].state == 3, "blocks: the caller's reference to the first feed's values");
    check(R.poll(false, &f1, &b1) && b0 == 0 && b1 == 0 && R.st.blocks[0].refs == 2 && R.st.slots[0].state == 0,
          "blocks: the launch's reference goes with its last feed");
    check(f0.coff == 0 && f0.n_cand == 8 && f1.coff == 8 && f1.n_cand == 12, "blocks: both views lie in the one block");
    for (int i = 0; i < 3; ++i) check(R.submit(make_feed(2 + i, 16, 1)) == STAGE_OK, "blocks: three more launches");
    check(R.st.slots[1].block == 1 && R.st.slots[2].block == 2 && R.st.slots[3].block == 3, "blocks: block 0 is not reused while its values are out");
    check(R.submit(make_feed(5, 16, 1)) == STAGE_OK && R.close_open() == STAGE_BUSY, "blocks: with every block held the launch cannot close");
    check(!R.st.release(0) && R.close_open() == STAGE_BUSY && !R.st.release(0) && R.st.blocks[0].refs == 0, "blocks: both views released");
    check(R.st.release(0).kind == STAGE_ARG && R.close_open() == STAGE_OK && R.st.slots[0].block == 0, "blocks: now block 0 is reused");
}

}  // namespace

int main()
{
    test_capacity();
    test_offsets();
    test_refusals();
    test_blocks();
    printf("%d checks, %d failed\n", g_checks, g_failed);
    if (g_failed) return 1;
    printf("all checks passed\n");
    return 0;
}
