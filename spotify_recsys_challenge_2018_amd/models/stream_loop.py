"""The streamed loop of `recommend_iter` / `evaluate_iter` (models/DAEs.py) on the library's pipeline (`_lib.Pipeline`):
feed preparation (numpy in, numpy out), the loop, the model's pipeline cache.  The loop knows the pipeline only by `submit`,
`submit_eval`, `submit_candidates`, `poll`, `poll_eval`, `poll_candidates`, `flush`, `stats`, `close`, `pending`, `group_rows`, `max_nnz`, `max_answers`, `title_len`, `users`
and `h` (None once closed), and the model not at all: tests/test_stream_loop_cpu.py drives it with a stand-in and no device."""
from collections import deque
from itertools import chain

import numpy as np

from .. import _lib

SEEDS_FROM_INPUT = "input"      # recommend(seeds=SEEDS_FROM_INPUT): the seeds are the track columns of the input feed


def title_block(titles, titles_use, n_batch, title_len):
    """A feed's title items -> (titles [n_batch, title_len] int32, -1 where a row has none; use [n_batch] float32), or
    (None, None) when titles_use is all zero: the plain DAE, as DAE_title.recommend decides."""
    u = np.asarray(titles_use, np.float32).reshape(-1)[:n_batch]
    if not (u.size and np.any(u)):
        return None, None
    block = np.full((n_batch, title_len), -1, np.int32)
    nt = min(len(titles), n_batch)
    if nt:
        if not isinstance(titles, np.ndarray):
            titles = [([-1] * title_len) if x is None else x for x in titles[:nt]]
        block[:nt] = np.asarray(titles, np.int64).reshape(-1, title_len)[:nt]
    use = np.zeros(n_batch, np.float32)
    use[:min(u.size, nt)] = u[:nt]                                # (no title, no use)
    return block, use


def answers_csr(answers, n_rows, n_batch):
    """One id list per row of a feed -> (row_ptr int32 [n_batch + 1], col int32), a CSR over the launch's n_batch rows; None
    for a feed of more than n_batch rows (no launch slot: `takes_feed`)."""
    if len(answers) != n_rows:
        raise ValueError("evaluate_iter: %d answer lists for a feed of %d rows" % (len(answers), n_rows))
    if n_rows > n_batch:
        return None
    row_ptr = np.zeros(n_batch + 1, np.int32)
    np.cumsum(np.fromiter(map(len, answers), np.int64, n_rows), out=row_ptr[1:n_rows + 1])
    row_ptr[n_rows + 1:] = row_ptr[n_rows]
    return row_ptr, np.fromiter(chain.from_iterable(answers), np.int32, int(row_ptr[-1]))


def candidates_csr(candidates, n_rows, n_batch, n_cols):
    """A feed's candidates, as the per-batch calls take them, -> (row_ptr int32 [n_batch + 1], col int32): the host CSR
    `Pipeline.submit_candidates` stages, over the launch's n_batch rows (the rows behind n_rows are empty).  A 2-D int array
    [rows, C] with -1 padding goes without a pass over its rows: row_ptr = arange * C and the array's own memory as col (an
    int32 C-contiguous array is not copied).  An id outside -1 / [0, n_cols) raises ValueError, as `candidates_to_csr` does."""
    row_ptr = np.empty(n_batch + 1, np.int32)
    if isinstance(candidates, np.ndarray) and candidates.ndim == 2:
        if candidates.dtype.kind not in "iu":
            raise ValueError("candidates: an integer array is required, got %s" % candidates.dtype)
        rows, width = candidates.shape
        if rows > n_rows:
            raise ValueError("candidates: %d rows for a feed of %d" % (rows, n_rows))
        if rows * width >= 2 ** 31:
            raise ValueError("candidates: %d entries do not fit the int32 offsets of the CSR" % (rows * width))
        row_ptr[:rows + 1] = np.arange(rows + 1, dtype=np.int64) * width
        row_ptr[rows + 1:] = rows * width
        col = candidates.reshape(-1)
    else:
        rows = len(candidates)
        if rows > n_rows:
            raise ValueError("candidates: %d rows for a feed of %d" % (rows, n_rows))
        lens = np.fromiter(map(len, candidates), np.int64, rows)
        total = int(lens.sum())
        if total >= 2 ** 31:
            raise ValueError("candidates: %d entries do not fit the int32 offsets of the CSR" % total)
        row_ptr[0] = 0
        np.cumsum(lens, out=row_ptr[1:rows + 1])
        row_ptr[rows + 1:] = total
        col = np.fromiter(chain.from_iterable(candidates), np.int64, total)
    if col.size and (col.min() < -1 or col.max() >= n_cols):
        bad = col[(col < -1) | (col >= n_cols)][0]
        raise ValueError("candidate id %d out of range: -1 (padding) or [0, %d)" % (bad, n_cols))
    return row_ptr, np.ascontiguousarray(col, np.int32)


def candidates_result(values, candidates, row_ptr, n_rows):
    """A feed's values in the caller's form (`DAE_tied._cand_result`): [n_rows, C] for the 2-D form (-inf on the rows behind
    the array), else one float32 array per row."""
    if isinstance(candidates, np.ndarray) and candidates.ndim == 2:
        if candidates.shape[0] == n_rows:
            return values.reshape(candidates.shape)
        out = np.full((n_rows, candidates.shape[1]), -np.inf, np.float32)
        out[:candidates.shape[0]] = values.reshape(candidates.shape)
        return out
    return [values[row_ptr[r]:row_ptr[r + 1]] for r in range(n_rows)]


def stream_candidates(pipe, feeds, fallback, n_batch, n_cols, want_scores=True, cache=None, key=None):
    """`feeds` through a pipeline in candidates mode: one result per feed, in feed order.  feeds yield (feed, candidates) --
    `feed` what `stream` takes, `candidates` a list of per-row id sequences or a 2-D int array with -1 padding.  A scoring
    pipeline (`pipe.cand_rank` False) yields the listed pairs' values in the form of `candidates`, a ranking one (idx [n_rows, k],
    score or None).  fallback(feed, candidates) -> the same from the per-batch call, for the feeds the pipeline does not take:
    explicit seed lists under a ranking pipeline, more rows / entries / candidate ids than a launch slot holds."""
    submit, flush, rank = pipe.submit_candidates, pipe.flush, pipe.cand_rank
    poll = pipe.poll if rank else pipe.poll_candidates
    title_len, max_nnz, max_cand = pipe.title_len, pipe.max_nnz, pipe.max_candidates
    pending = deque()            # per pending feed: (rows it asked for, its candidates, their row_ptr)
    per_launch = max(1, pipe.group_rows // max(1, n_batch))
    n_fed = 0

    def out(r):
        n, cands, rp = pending.popleft()
        if rank:
            if n == n_batch:
                return r[0], (r[1] if want_scores else None)
            return r[0][:n], (r[1][:n] if want_scores else None)
        return candidates_result(r[0], cands, rp, n)
    clean = False
    pipe.users += 1
    try:
        for f, cands in feeds:
            x_positions, x_ones, seeds, n_rows = f[:4]
            n = n_batch if n_rows is None else int(n_rows)
            if n > n_batch:
                raise ValueError("n_rows = %d exceeds the model's batch of %d" % (n, n_batch))
            rp, col = candidates_csr(cands, n, n_batch, n_cols)      # (refused here: nothing of this feed is uploaded)
            titles = use = None
            if len(f) > 5 and f[4] is not None and f[5] is not None and title_len is not None:
                titles, use = title_block(f[4], f[5], n_batch, title_len)
            nnz = int(np.shape(x_positions)[0]) if np.ndim(x_positions) == 2 else len(x_positions)
            seeds_ok = (isinstance(seeds, str) and seeds == SEEDS_FROM_INPUT) or not rank
            if not (seeds_ok and nnz <= max_nnz and col.size <= max_cand):
                flush()                                          # in order: behind everything queued before it
                while pipe.pending:
                    yield out(poll(True))
                yield fallback(f, cands)
                continue
            while not submit(x_positions, x_ones, n_batch, (rp, col), titles, use):
                yield out(poll(True))
            pending.append((n, cands, rp))
            n_fed += 1
            if n_fed % per_launch == 0 or titles is not None:
                while True:
                    r = poll(False)
                    if r is None:
                        break
                    yield out(r)
        flush()
        while pipe.pending:
            yield out(poll(True))
        clean = True
    except _lib.DaeError as e:
        if "out of range" in str(e) or "outside" in str(e):
            raise ValueError(str(e))
        raise
    finally:
        pipe.users -= 1
        cached = cache is not None and cache.get(key, (None, None))[1] is pipe
        if not clean or (cached and pipe.users == 0 and len(cache) > 1):
            if cached:
                cache.pop(key, None)
            pipe.close()


def takes_feed(seeds, n_rows, nnz, n_answers, titles_dropped, n_batch, max_nnz, max_answers):
    """Does the pipeline take this feed?  Not explicit seed lists, not more rows / entries / answers than a launch slot holds,
    and not titles it would drop (the feed carries some, the model is a DAE_title, the pipeline has no title scorer)."""
    return (isinstance(seeds, str) and seeds == SEEDS_FROM_INPUT and n_rows <= n_batch and nnz <= max_nnz
            and n_answers <= max_answers and not titles_dropped)


def stream(pipe, feeds, fallback, n_batch, want_scores=True, eval_mode=False, mixes_titles=False, on_guard=None,
           cache=None, key=None):
    """`feeds` through `pipe`: one result per feed, in feed order.  feeds yield (x_positions, x_ones, seeds, n_rows[, titles,
    titles_use]), out come (idx [n_rows, k], score or None); eval_mode: feeds yield (feed, answers), out come the rows' metric
    records.  A feed is fed as the graph's n_batch rows (DAEs.py:34) and handed out as the n_rows it asked for.  fallback(feed)
    -> (idx, score): the per-batch path, for the feeds `takes_feed` refuses.  mixes_titles: the model is a DAE_title.  on_guard(n):
    told at the end how many launches the exact mode's guard had re-scored.  cache, key: where `pipe` is cached as (gen, pipe)."""
    submit, submit_eval, flush, poll = pipe.submit, pipe.submit_eval, pipe.flush, pipe.poll
    if eval_mode:
        from ..utils.metrics import rank_records
        poll = pipe.poll_eval
    title_len, max_nnz, max_answers = pipe.title_len, pipe.max_nnz, (pipe.max_answers if eval_mode else 0)
    drops_titles = mixes_titles and title_len is None
    rows_out = deque()           # rows each pending feed asked for
    # results arrive a LAUNCH at a time: asking the pipeline after every feed whether something is ready is a foreign call
    # per feed for an answer that changes once per launch (the caller's thread is what bounds the bf16 loops: round 6)
    per_launch = max(1, pipe.group_rows // max(1, n_batch))
    n_fed, ans, n_ans = 0, None, 0

    def out(r):
        n = rows_out.popleft()
        if eval_mode:
            return r if n == n_batch else r[:n]
        if n == n_batch:
            return r[0], (r[1] if want_scores else None)
        return r[0][:n], (r[1][:n] if want_scores else None)
    clean = False
    fallbacks0 = pipe.stats()["guard_fallbacks"] if on_guard is not None else 0
    pipe.users += 1                                              # (`pipeline_for` never closes a pipeline a loop is running on)
    try:
        for f in feeds:
            if eval_mode:
                f, answers = f
            x_positions, x_ones, seeds, n_rows = f[:4]
            n = n_batch if n_rows is None else int(n_rows)
            titles = use = None
            if len(f) > 5 and f[4] is not None and f[5] is not None and title_len is not None:
                titles, use = title_block(f[4], f[5], n_batch, title_len)
            if eval_mode:
                ans = answers_csr(answers, n, n_batch)
                n_ans = int(ans[0][-1]) if ans is not None else 0
            nnz = int(np.shape(x_positions)[0]) if np.ndim(x_positions) == 2 else len(x_positions)
            if not takes_feed(seeds, n, nnz, n_ans, drops_titles and len(f) > 4, n_batch, max_nnz, max_answers):
                flush()                                          # in order: behind everything queued before it
                while pipe.pending:
                    yield out(poll(True))
                idx, score = fallback(f)
                yield rank_records(idx, answers) if eval_mode else (idx, (score if want_scores else None))
                continue
            # (every lane full: hand the oldest lists out first)
            while not (submit_eval(x_positions, x_ones, n_batch, ans, titles, use) if eval_mode
                       else submit(x_positions, x_ones, n_batch, titles, use)):
                yield out(poll(True))
            rows_out.append(n)
            n_fed += 1
            if n_fed % per_launch == 0 or titles is not None:
                while True:                                      # ... and whatever else is ready, without waiting
                    r = poll(False)
                    if r is None:
                        break
                    yield out(r)
        flush()
        while pipe.pending:
            yield out(poll(True))
        clean = True
    except _lib.DaeError as e:
        if "out of range" in str(e) or "outside" in str(e):
            raise ValueError(str(e))
        raise
    finally:
        pipe.users -= 1
        if on_guard is not None and pipe.h is not None:
            n_fb = pipe.stats()["guard_fallbacks"] - fallbacks0
            if n_fb > 0:             # (the lists that went out are the fp32 kernels': the pipeline re-scored those launches itself)
                on_guard(n_fb)
        # an error, or a consumer that stopped early: feeds may be queued -- this pipeline is not reused.  A clean end, but
        # another key's pipeline was created while this loop ran: one stays
        cached = cache is not None and cache.get(key, (None, None))[1] is pipe
        if not clean or (cached and pipe.users == 0 and len(cache) > 1):
            if cached:
                cache.pop(key, None)
            pipe.close()


def pipeline_for(model, scorer, dtype, k, want_scores, eval_mode=False, catalogue=None, candidates=None):
    """-> (key, pipeline) out of `model._pipes`: created on first use, and again after the weights, the title variables of
    `scorer` (the Char_CNN its launches mix in, or None) or the exact margin changed.  catalogue: an open CatalogueHandle of
    `model` -> a pipeline in catalogue mode (`Pipeline.set_catalogue`: images of its own, gathered from the model's current
    weights); the handle remembers it and closes it before it frees its column tables."""
    key = (int(dtype), int(k), bool(want_scores), model.n_batch) + (("eval",) if eval_mode else ())
    if catalogue is not None:
        key += (("catalogue", id(catalogue)),)
    if candidates is not None:   # (rank, out_kind, max_candidates): a pipeline in candidates mode (`Pipeline.enable_candidates`)
        key += (("candidates",) + tuple(candidates),)
    # (dae_set_exact_margin on the model's contexts -- the guard's test hook -- reaches the pipeline's own images as well)
    margins = [getattr(c, "_exact_margin", 1.0) for c in ([model.ctx] + ([] if scorer is None else [scorer.ctx]))]
    margin = next((m_ for m_ in margins if m_ != 1.0), 1.0)
    gen = (model._weights_gen, None if scorer is None else scorer._params_gen, margin)
    cache = model._pipes
    ent = cache.get(key)
    if ent is not None and (ent[0] != gen or ent[1].h is None):
        ent[1].close()
        ent = None
    if ent is None:
        import torch
        # one pipeline at a time per model: each holds (2 lanes + 2) staging slots of pinned + device memory and a dozen
        # result blocks -- a caller that alternates dtypes pays a re-creation, not half a gigabyte of pinned memory
        for key_, (_g, old) in list(cache.items()):
            if old.users > 0:                    # a loop of another (dtype, k, scores) key is still running on it (two loops
                continue                         # interleaved): it closes with that loop
            if model.keep_pipelines:             # (diagnosis: scripts/probe/row_diag.py)
                model._old_pipes.append(old)
            else:
                old.close()
            cache.pop(key_, None)
        model._flush_rows_adam()
        torch.cuda.current_stream(model.device_index).synchronize()      # the weights are final before another thread reads them
        # (titled launches: the fp32 rule -- 5 feeds of 150 = 750 rows of the 96- / 128-row groups, as the Python loop ran them)
        group = model._coalesce_count(dtype if scorer is None else None) * model.n_batch
        if scorer is not None or candidates is not None:     # (the title kernels' and the candidate kernels' rows per launch)
            group = min(group, 4096)
        # three lanes: measured best in every mode (batch 256, playlists/s through the loop, 2 / 3 / 4 lanes: fp32 0.98 /
        # 1.29 / 1.06 M, exact_bf16 4.1 / 4.8 / 4.2 M, bf16 5.3 / 6.3 / 5.6 M -- profiles/r04_notes.md)
        pipe = _lib.Pipeline(model.weights["encoder_h"], model.biases["encoder_b"], model.weights["decoder_h"],
                             model.biases["decoder_b"], model.n_tracks, dtype=dtype, k=k, group_rows=group,
                             max_nnz=max(1 << 18, group * 1024), lanes=int(model.n_lanes or 3), want_scores=want_scores,
                             device_index=model.device_index, title=scorer)
        if catalogue is not None:
            try:
                pipe.set_catalogue(catalogue.cat)
            except _lib.DaeError:
                pipe.close()
                raise
            catalogue._pipes = [q for q in catalogue._pipes if q.h is not None] + [pipe]
        if margin != 1.0 and dtype == _lib.DAE_DTYPE_BF16_EXACT:
            pipe.exact_margin(margin)
        if candidates is not None:
            try:
                pipe.enable_candidates(max_candidates=candidates[2], rank=candidates[0], out_kind=candidates[1])
            except _lib.DaeError:
                pipe.close()
                raise
        if eval_mode:            # (the challenge's playlists hold at most 250 tracks; a feed with more answers than a launch
            pipe.enable_eval(max_answers=max(1 << 16, group * 256))      # slot takes goes the per-batch way)
        ent = cache[key] = (gen, pipe)
    return key, ent[1]
