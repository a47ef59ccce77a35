// Stand-alone program (no device, no HIP): the caller thread's half of the streaming pipeline, csrc/pipeline_stage.h, driven
// in the order pipeline.hip's submit / flush / poll / release drive it (minus the locks and the worker: a queued launch is marked
// issued by hand) against a straightforward model -- concatenate the feeds of a launch, shift the rows.  Every staging buffer is
// a heap block of exactly the size pipeline_create gives it, so a write past a launch's limits is a heap overflow under
// -fsanitize=address.  Exits 0 and prints "all checks passed".
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

struct FeedIn {                   // one feed as a caller passes it
    std::vector<int64_t> pos; std::vector<float> val; int bcast = 0; int n_rows = 0;
    std::vector<int32_t> titles; std::vector<float> use;      // titled feeds
    std::vector<int32_t> arp, acol;                          // evaluation feeds
    int64_t nnz() const { return (int64_t)pos.size() / 2; }
};

struct Launch {                   // the model: what a launch's staging must hold
    std::vector<int64_t> row, col; std::vector<float> val;
    std::vector<int32_t> titles, arp{0}, acol; std::vector<float> use;
    std::vector<Feed> feeds; int titled = 0;
};

struct Rig {
    Stage<StageSlot, StageBlock> st;
    bool eval = false;
    std::deque<int> queue;        // closed launches, in order (what the worker would take)
    std::vector<std::unique_ptr<char[]>> heap;
    std::vector<Launch> model;    // per slot: the launch it holds now
    std::vector<std::vector<int>> closed;                    // every closed launch's feed sizes, in order
    std::vector<uint64_t> out_tickets;

    template <class T> T* block(size_t count) { heap.emplace_back(new char[count * sizeof(T)]); return reinterpret_cast<T*>(heap.back().get()); }
    Rig(int group_rows, int64_t max_nnz, int lanes, int title_len = 0, int64_t max_answers = 0, int blocks = 0)
    {
        st.group_rows = group_rows; st.max_nnz = max_nnz; st.title_len = title_len; st.max_answers = max_answers; st.n_lanes = lanes;
        eval = max_answers > 0;
        st.slots.resize(2 * lanes + 2);
        st.blocks.resize(blocks > 0 ? blocks : (int)st.slots.size());
        model.resize(st.slots.size());
        const size_t rows = (size_t)group_rows, nz = (size_t)max_nnz;
        for (StageSlot& S : st.slots) {                      // the sizes of pipeline_create / dae_pipeline_enable_eval
            S.h_pos = block<int64_t>(nz * 2);
            S.h_val = block<float>(nz);
            if (title_len) { S.h_titles = block<int32_t>(rows * title_len); S.h_use = block<float>(rows); }
            if (eval) { S.h_arp = block<int32_t>(rows + 1); S.h_acol = block<int32_t>((size_t)max_answers); }
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
        return STAGE_OK;
    }
    // submit_impl of pipeline.hip, call for call
    int submit(const FeedIn& f, uint64_t* ticket = nullptr)
    {
        const int titled = f.titles.empty() ? 0 : 1;
        const int64_t nnz = f.nnz();
        const int32_t* arp = f.arp.empty() ? nullptr : f.arp.data();
        int64_t n_ans = 0;
        if (const StageErr e = st.check_feed(eval, f.pos.data(), f.val.data(), nnz, f.n_rows, arp, f.acol.data(), &n_ans)) return e.kind;
        if (titled && !st.rows_inside(f.pos.data(), nnz, f.n_rows)) return st.bad_row().kind;
        if (st.open_slot >= 0 && !st.fits_open(f.n_rows, nnz, titled, n_ans)) {
            const int rc = close_open();
            if (rc) return rc;
        }
        Staged at;
        if (const StageErr e = st.begin(f.n_rows, nnz, titled, n_ans, &at)) return e.kind;
        if (!st.copy_positions(at, titled, f.pos.data(), nnz, f.n_rows)) {
            st.rollback(at, f.n_rows, nnz, n_ans);
            return st.bad_row().kind;
        }
        st.copy_values(at, f.val.data(), f.bcast, nnz);
        if (titled) st.copy_titles(at, f.titles.data(), f.use.data(), f.n_rows);
        if (arp) st.copy_answers(at, arp, f.acol.data(), f.n_rows, n_ans);
        if (ticket) *ticket = at.ticket;
        // the model: the feed behind the launch's earlier ones
        Launch& M = model[at.slot];
        if (at.row0 == 0) M = Launch();
        M.titled = titled;
        for (int64_t i = 0; i < nnz; ++i) {
            M.row.push_back(f.pos[2 * i] + at.row0);
            const int64_t c = f.pos[2 * i + 1];
            M.col.push_back(titled ? c : (c < 0 || c > INT32_MAX ? -1 : c));
            M.val.push_back(f.bcast ? f.val[0] : f.val[i]);
        }
        M.titles.insert(M.titles.end(), f.titles.begin(), f.titles.end());
        M.use.insert(M.use.end(), f.use.begin(), f.use.end());
        for (int r = 0; arp && r < f.n_rows; ++r) M.arp.push_back(M.arp.back() + (arp[r + 1] - arp[r]));
        for (int64_t a = 0; a < n_ans; ++a) M.acol.push_back(f.acol[arp[0] + a]);
        M.feeds.push_back(Feed{at.ticket, at.row0, f.n_rows});
        const int slot = at.slot;
        if (st.open_is_full_for(f.n_rows)) (void)close_open();
        verify(slot, "after submit");
        return STAGE_OK;
    }
    // the slot's staging and counts against the model
    void verify(int si, const char* when)
    {
        const StageSlot& S = st.slots[si];
        const Launch& M = model[si];
        const std::string w = std::string(when) + ", slot " + std::to_string(si) + ": ";
        bool ok = S.nnz == (int64_t)M.row.size() && S.titled == M.titled && S.feeds.size() == M.feeds.size() &&
                  S.n_ans == (int64_t)M.acol.size();
        int rows = 0;
        for (size_t i = 0; ok && i < M.feeds.size(); ++i) {
            ok = S.feeds[i].ticket == M.feeds[i].ticket && S.feeds[i].row0 == rows && S.feeds[i].n_rows == M.feeds[i].n_rows;
            rows += M.feeds[i].n_rows;
        }
        check(ok && S.rows == rows, w + "counts, row0 and tickets of the feeds");
        if (!ok) return;
        const int32_t* p32 = reinterpret_cast<const int32_t*>(S.h_pos);
        bool words = true;
        for (int64_t i = 0; i < S.nnz; ++i) {
            if (S.titled) words = words && S.h_pos[2 * i] == M.row[i] && S.h_pos[2 * i + 1] == M.col[i];
            else words = words && p32[2 * i] == M.row[i] && p32[2 * i + 1] == M.col[i];
            words = words && S.h_val[i] == M.val[i];
        }
        check(words, w + "staged (row, col) pairs and values");
        bool extra = true;
        for (size_t i = 0; i < M.titles.size(); ++i) extra = extra && S.h_titles[i] == M.titles[i];
        for (size_t i = 0; i < M.use.size(); ++i) extra = extra && S.h_use[i] == M.use[i];
        if (eval && rows > 0) for (int r = 0; r <= rows; ++r) extra = extra && S.h_arp[r] == M.arp[r];
        for (size_t i = 0; i < M.acol.size(); ++i) extra = extra && S.h_acol[i] == M.acol[i];
        check(extra, w + "titles, titles_use and the answers' CSR");
    }
    void issue_all() { for (int si : queue) st.slots[si].state = 3; queue.clear(); }
    // poll: the next feed of the launch at poll_slot, if that launch was issued; its block's caller reference released when asked
    bool poll(bool release_it, int* block = nullptr)
    {
        const StageSlot& S = st.slots[st.poll_slot];
        if (S.state != 3) return false;
        const int before = st.poll_slot;
        const bool last = S.next_feed + 1 == S.feeds.size();
        const auto h = st.hand_out();
        out_tickets.push_back(h.feed.ticket);
        check(st.poll_slot == (last ? (before + 1) % (int)st.slots.size() : before), "poll_slot advances at a launch's last feed only");
        check(last == (st.slots[before].state == 0), "the slot is free behind its last feed only");
        if (block) *block = h.block;
        if (release_it) check(!st.release(h.block), "release of a block that is out");
        return true;
    }
};

FeedIn make_feed(int id, int n_rows, int per_row, int answers_per_row = 0, int title_len = 0)
{
    FeedIn f;
    f.n_rows = n_rows;
    for (int i = 0; i < n_rows * per_row; ++i) {
        f.pos.push_back(i % n_rows);
        f.pos.push_back((id * 1000 + i * 7) % 100000);
        f.val.push_back(id + 0.5f * i);
    }
    for (int i = 0; i < n_rows * title_len; ++i) f.titles.push_back(id * 31 + i);
    for (int i = 0; title_len && i < n_rows; ++i) f.use.push_back(i & 1 ? 1.f : 0.f);
    if (answers_per_row) {
        f.arp.push_back(0);
        for (int r = 0; r < n_rows; ++r) {
            for (int a = 0; a < answers_per_row; ++a) f.acol.push_back(id * 100 + r + a);
            f.arp.push_back((int32_t)f.acol.size());
        }
    }
    return f;
}

const std::vector<int> kSizes = {64, 17, 64, 1, 40, 64, 64, 5, 64, 33, 64, 64};      // test_native_pipeline_orders_lends_and_recovers

// all of kSizes through a rig (draining one launch whenever the ring is busy); the launch boundaries, tickets 1..n, hand-out order
void order_case(const char* name, Rig& R, int per_row, int answers_per_row, const std::vector<std::vector<int>>& want)
{
    uint64_t next = 1;
    for (size_t i = 0; i < kSizes.size(); ++i) {
        const FeedIn f = make_feed((int)i, kSizes[i], per_row, answers_per_row);
        uint64_t t = 0;
        int rc = R.submit(f, &t);
        if (rc == STAGE_BUSY) {                              // drain the oldest launch, then the same feed again
            R.issue_all();
            while (R.poll(true)) if (R.st.slots[R.st.poll_slot].next_feed == 0) break;
            rc = R.submit(f, &t);
        }
        check(rc == STAGE_OK, std::string(name) + ": feed " + std::to_string(i) + " taken");
        check(t == next++, std::string(name) + ": tickets count 1..n without gaps");
    }
    check(R.close_open() == STAGE_OK, std::string(name) + ": flush");
    R.issue_all();
    while (R.poll(true)) {}
    check(R.closed == want, std::string(name) + ": launch boundaries");
    bool in_order = R.out_tickets.size() == kSizes.size();
    for (size_t i = 0; in_order && i < R.out_tickets.size(); ++i) in_order = R.out_tickets[i] == i + 1;
    check(in_order, std::string(name) + ": hand-out order equals submission order");
    for (const StageBlock& b : R.st.blocks) check(b.refs == 0, std::string(name) + ": every block is back");
}

void test_order()
{
    // rows close the launches: a feed goes off as soon as the next one of its size would not fit
    { Rig R(160, 1 << 16, 2); order_case("rows", R, 3, 0, {{64, 17, 64}, {1, 40, 64}, {64, 5, 64}, {33, 64}, {64}}); }
    // 2 entries per row, max_nnz 200: nnz closes a launch before rows do (8 launches through 6 slots: the ring wraps)
    { Rig R(160, 200, 2); order_case("nnz", R, 2, 0, {{64, 17}, {64, 1}, {40}, {64}, {64, 5}, {64, 33}, {64}, {64}}); }
    // 1 answer per row, max_answers 130
    { Rig R(160, 1 << 16, 2, 0, 130); order_case("answers", R, 3, 1, {{64, 17}, {64, 1, 40}, {64, 64}, {5, 64, 33}, {64, 64}}); }
}

void test_kinds()
{
    Rig R(160, 4096, 2, 5);
    check(R.submit(make_feed(0, 8, 2)) == STAGE_OK && R.submit(make_feed(1, 8, 2, 0, 5)) == STAGE_OK, "kinds: plain, then titled");
    check(R.closed.size() == 1 && R.st.slots[0].titled == 0 && R.st.slots[1].titled == 1 && R.st.open_slot == 1,
          "kinds: a titled feed after a plain one starts a new launch");
    check(R.submit(make_feed(2, 8, 2, 0, 5)) == STAGE_OK && R.st.slots[1].feeds.size() == 2, "kinds: titled feeds share a launch");
    check(R.submit(make_feed(3, 8, 2)) == STAGE_OK && R.closed.size() == 2 && R.st.open_slot == 2 && R.st.slots[2].titled == 0,
          "kinds: a plain feed after a titled one starts a new launch");
    for (int si = 0; si < 3; ++si) R.verify(si, "kinds");
}

void test_narrowing()
{
    Rig R(16, 64, 1);
    FeedIn a = make_feed(0, 4, 2);
    FeedIn b;
    b.n_rows = 3;
    b.pos = {0, (int64_t)1 << 40, 1, -5, 2, INT32_MAX, 2, (int64_t)INT32_MAX + 1, 1, 0};
    b.val = {2.5f};
    b.bcast = 1;
    check(R.submit(a) == STAGE_OK && R.submit(b) == STAGE_OK, "narrowing: feeds taken");
    const StageSlot& S = R.st.slots[0];
    const int32_t* p = reinterpret_cast<const int32_t*>(S.h_pos) + 2 * a.nnz();
    check(p[0] == 4 && p[2] == 5 && p[4] == 6 && p[8] == 5, "narrowing: rows shifted by row0");
    check(p[1] == -1, "narrowing: a column of 2^40 becomes -1");
    check(p[3] == -1, "narrowing: a negative column becomes -1");
    check(p[5] == INT32_MAX && p[7] == -1 && p[9] == 0, "narrowing: INT32_MAX stays, INT32_MAX + 1 does not");
    bool bc = true;
    for (int i = 0; i < 5; ++i) bc = bc && S.h_val[a.nnz() + i] == 2.5f;
    check(bc, "narrowing: values_broadcast fills nnz values");
    FeedIn e;
    e.n_rows = 2;                                            // nnz = 0, no arrays at all
    uint64_t t = 0;
    check(R.submit(e, &t) == STAGE_OK && t == 3 && S.rows == 9 && S.nnz == a.nnz() + 5, "narrowing: nnz = 0 is taken");
    e.bcast = 1;
    check(R.submit(e) == STAGE_OK && S.rows == 11, "narrowing: nnz = 0 with values_broadcast is taken");
}

void test_refusal()
{
    {
        const int n_rows = 5;
        const int64_t bad_rows[] = {n_rows, -1, (int64_t)1 << 32, INT64_MAX};
        for (const int64_t bad : bad_rows) {
            const std::string tag = "refusal (row " + std::to_string(bad) + "): ";
            FeedIn poison = make_feed(7, n_rows, 3);
            poison.pos[2 * 8] = bad;
            const FeedIn good = make_feed(8, n_rows, 3);
            {   // as the first feed of a launch
                Rig R(32, 256, 1);
                check(R.submit(make_feed(0, 16, 2)) == STAGE_OK && R.submit(make_feed(1, 16, 2)) == STAGE_OK && R.closed.size() == 1,
                      tag + "a full launch before");
                const int ns = R.st.next_slot, os = R.st.open_slot;
                const uint64_t nt = R.st.next_ticket;
                check(R.submit(poison) == STAGE_ARG, tag + "refused as a first feed");
                check(R.st.next_slot == ns && R.st.open_slot == os && os == -1 && R.st.next_ticket == nt, tag + "ring and ticket as before");
                check(R.st.slots[ns].state == 0 && R.st.slots[ns].rows == 0 && R.st.slots[ns].nnz == 0 && R.st.slots[ns].feeds.empty(),
                      tag + "the slot is free");
                uint64_t t = 0;
                check(R.submit(good, &t) == STAGE_OK && t == nt && R.st.open_slot == ns, tag + "the next feed gets its ticket and slot");
            }
            {   // as a later feed of a launch: the same good feed lands where the refused one would have
                Rig R(32, 256, 1), Q(32, 256, 1);
                for (Rig* r : {&R, &Q}) check(r->submit(make_feed(0, 9, 2)) == STAGE_OK && r->submit(make_feed(1, 3, 4)) == STAGE_OK, tag + "two feeds");
                check(R.submit(poison) == STAGE_ARG, tag + "refused as a later feed");
                R.verify(0, "after a refused later feed");   // the earlier feeds' words, counts and tickets
                check(R.st.open_slot == 0 && R.st.next_slot == 1 && R.st.next_ticket == 3 && R.st.slots[0].state == 1, tag + "the launch stays open");
                uint64_t tr = 0, tq = 0;
                check(R.submit(good, &tr) == STAGE_OK && Q.submit(good, &tq) == STAGE_OK && tr == tq && tr == 3, tag + "same ticket as without the refusal");
                const StageSlot &A = R.st.slots[0], &B = Q.st.slots[0];
                check(A.rows == B.rows && A.nnz == B.nnz && !memcmp(A.h_pos, B.h_pos, (size_t)A.nnz * 2 * sizeof(int32_t)) &&
                      !memcmp(A.h_val, B.h_val, (size_t)A.nnz * sizeof(float)), tag + "same staging as without the refusal");
            }
            {   // as a titled feed: nothing of it is staged
                Rig R(32, 256, 1, 4);
                check(R.submit(make_feed(0, 9, 2, 0, 4)) == STAGE_OK, tag + "a titled feed");
                FeedIn tp = make_feed(7, n_rows, 3, 0, 4);
                tp.pos[2 * 8] = bad;
                const StageSlot& S = R.st.slots[0];
                const std::vector<int64_t> words(S.h_pos, S.h_pos + 2 * S.nnz);
                check(R.submit(tp) == STAGE_ARG, tag + "refused as a titled feed");
                check(S.rows == 9 && S.nnz == 18 && S.feeds.size() == 1 && R.st.next_ticket == 2 && R.st.open_slot == 0, tag + "counts untouched");
                check(!memcmp(words.data(), S.h_pos, (size_t)S.nnz * 2 * sizeof(int64_t)), tag + "nothing staged");
                R.verify(0, "after a refused titled feed");
            }
        }
    }
}

void test_answers()
{
    Rig R(16, 64, 1, 0, 12);
    FeedIn a = make_feed(0, 3, 2);
    a.acol = {900, 901, 7, -1, 7, 7, 902};                   // (900, 901 and 902 belong to other feeds of the caller's array)
    a.arp = {2, 4, 4, 6};                                    // does not start at 0; an empty row; -1 and duplicates
    FeedIn b = make_feed(1, 2, 2);
    b.acol = {11, 12, 13};
    b.arp = {0, 1, 3};
    check(R.submit(a) == STAGE_OK && R.submit(b) == STAGE_OK, "answers: feeds taken");
    const StageSlot& S = R.st.slots[0];
    const int32_t want_rp[] = {0, 2, 2, 4, 5, 7}, want_col[] = {7, -1, 7, 7, 11, 12, 13};
    check(!memcmp(S.h_arp, want_rp, sizeof(want_rp)), "answers: rebased to 0, the second feed's pointers continue the first's");
    check(S.n_ans == 7 && !memcmp(S.h_acol, want_col, sizeof(want_col)), "answers: -1 and duplicates copied as they are");
    FeedIn c = make_feed(2, 2, 2);
    c.acol = {1, 2, 3};
    c.arp = {0, 2, 1};
    check(R.submit(c) == STAGE_ARG && S.rows == 5 && R.st.next_ticket == 3, "answers: a decreasing ans_row_ptr is refused");
    c.arp = {0, 2, 3};
    int64_t na = 0;
    check(R.st.check_feed(true, c.pos.data(), c.val.data(), c.nnz(), 2, c.arp.data(), nullptr, &na).kind == STAGE_ARG,
          "answers: answers without ans_col are refused");
    FeedIn d = make_feed(3, 2, 2, 7);                        // 14 answers > max_answers
    check(R.submit(d) == STAGE_ARG, "answers: more than max_answers are refused");
    check(R.submit(make_feed(4, 2, 2)) == STAGE_STATE, "answers: a feed without answers is refused by an evaluation pipeline");
    Rig P(16, 64, 1);
    check(P.submit(make_feed(5, 2, 2, 1)) == STAGE_STATE, "answers: a feed with answers is refused by a plain pipeline");
    check(R.submit(make_feed(6, 2, 2, 3)) == STAGE_OK && R.closed.size() == 1 && R.st.slots[1].n_ans == 6 && R.st.slots[1].h_arp[2] == 6,
          "answers: a feed whose answers do not fit the open launch starts a new one");
}

void test_sizes()
{
    Rig R(16, 64, 1);
    FeedIn f = make_feed(0, 17, 1);
    check(R.submit(f) == STAGE_ARG, "sizes: more rows than group_rows");
    check(R.submit(make_feed(0, 16, 5)) == STAGE_ARG, "sizes: more entries than max_nnz");
    FeedIn z;
    check(R.submit(z) == STAGE_ARG, "sizes: no rows");
    check(R.st.next_ticket == 1 && R.st.open_slot == -1, "sizes: nothing changed");
}

void test_busy()
{
    const int lanes = 2;
    Rig R(8, 64, lanes);
    const int n_slots = 2 * lanes + 2;
    for (int i = 0; i < n_slots; ++i) check(R.submit(make_feed(i, 8, 2)) == STAGE_OK, "busy: one full launch per slot");
    check((int)R.closed.size() == n_slots, "busy: every slot holds a closed launch");
    R.issue_all();
    const int ns = R.st.next_slot, ps = R.st.poll_slot;
    const uint64_t nt = R.st.next_ticket;
    check(R.submit(make_feed(99, 4, 2)) == STAGE_BUSY, "busy: the submit that needs slot n_slots + 1 reports busy");
    check(R.st.next_slot == ns && R.st.poll_slot == ps && R.st.next_ticket == nt && R.st.open_slot == -1, "busy: nothing changed");
    check(R.poll(true), "busy: the first launch's only feed handed out");
    uint64_t t = 0;
    check(R.submit(make_feed(99, 4, 2), &t) == STAGE_OK && t == nt && R.st.open_slot == 0, "busy: then it succeeds, in the freed slot");
}

void test_blocks()
{
    Rig R(16, 64, 1, 0, 0, 4);                               // 4 slots, 4 blocks
    check(R.st.release(0).kind == STAGE_ARG && R.st.release(-1).kind == STAGE_ARG && R.st.release(4).kind == STAGE_ARG,
          "blocks: releasing a block that is not out is refused");
    check(R.submit(make_feed(0, 4, 2)) == STAGE_OK && R.submit(make_feed(1, 4, 2)) == STAGE_OK && R.close_open() == STAGE_OK, "blocks: a launch of two feeds");
    check(R.st.slots[0].block == 0 && R.st.blocks[0].refs == 1, "blocks: the launch's own reference");
    R.issue_all();
    int b0 = -1, b1 = -1;
    check(R.poll(false, &b0) && R.st.blocks[0].refs == 2 && R.st.slots[0].state == 3, "blocks: the caller's reference to the first feed");
    check(R.poll(false, &b1) && b0 == 0 && b1 == 0 && R.st.blocks[0].refs == 2 && R.st.slots[0].state == 0,
          "blocks: the launch's reference goes with its last feed");
    for (int i = 0; i < 3; ++i) check(R.submit(make_feed(2 + i, 16, 1)) == STAGE_OK, "blocks: three more launches");
    check(R.st.slots[1].block == 1 && R.st.slots[2].block == 2 && R.st.slots[3].block == 3, "blocks: block 0 is not reused while it is out");
    check(R.submit(make_feed(5, 16, 1)) == STAGE_OK && R.st.open_slot == 0 && R.st.slots[0].state == 1 && R.queue.size() == 3,
          "blocks: with every block held the launch cannot close (it stays staged)");
    check(R.close_open() == STAGE_BUSY, "blocks: flush reports busy");
    check(!R.st.release(0) && R.close_open() == STAGE_BUSY, "blocks: one caller's reference is not enough");
    check(!R.st.release(0) && R.st.blocks[0].refs == 0, "blocks: both released");
    check(R.st.release(0).kind == STAGE_ARG, "blocks: a third release is refused");
    check(R.close_open() == STAGE_OK && R.st.slots[0].block == 0, "blocks: now block 0 is reused");
}

}  // namespace

int main()
{
    test_order();
    test_kinds();
    test_narrowing();
    test_refusal();
    test_answers();
    test_sizes();
    test_busy();
    test_blocks();
    printf("%d checks, %d failed\n", g_checks, g_failed);
    if (g_failed) return 1;
    printf("all checks passed\n");
    return 0;
}
