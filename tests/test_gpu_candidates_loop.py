"""GPU (-m gpu): caller-given candidates on the streaming pipeline (the candidates mode of csrc/pipeline*.hip) and the
de-duplication kernel (csrc/candidates.hip dae_candidates_unique).  The contract is the pipeline's own -- rows are independent --
so every comparison is `==` on the 32-bit words against the per-batch calls on each feed alone: dae_score_candidates
(+ dae_rank_candidates behind a HOST de-duplication) at the C level, `score_candidates` / `rank_candidates` at the models'.

What the sentinel test can see: the pinned result block (pre-filled through the pointer an earlier poll handed out) keeps its
sentinel behind the launch's last value.  The slot's DEVICE array has no read-back; the candidate kernels' own bound (nothing at or
past n_cand) is tests/test_gpu_candidates.py's."""
import ctypes
import pickle

import numpy as np
import pytest

from oracle import title_numpy as tn
from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.models.DAEs import (DAE, DAE_tied, DAE_title, SEEDS_FROM_INPUT, candidates_to_csr,
                                                            coo_to_csr)
from spotify_recsys_challenge_2018_amd.models.title_models import get_model
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights

pytestmark = pytest.mark.gpu
U32 = np.uint32
SHAPES = {"generic": (3000, 2500, 64), "h256": (20000, 17000, 256)}        # V, n_tracks, hidden
N_CHAR, TITLE = 41, (25, [3, 5], 40, 25)                                   # E, filter sizes, F, title length


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(U32), b.view(U32))


_W = {}


def _weights(name, tied=False):
    """Host weights and their device copies, made once per shape and left unchanged."""
    key = (name, tied)
    if key not in _W:
        V, NT, H = SHAPES[name]
        W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=H + 1, bias="zipf", n_tracks=NT, tied=tied)
        b_enc = (np.random.default_rng(H + 7).standard_normal(H) * 0.1).astype(np.float32)
        host = dict(W_enc=W_enc, b_enc=b_enc, W_dec=W_dec, b_dec=b_dec, V=V, NT=NT, H=H)
        host["dev"] = tuple(_dev(host[n]) for n in ("W_enc", "b_enc", "W_dec", "b_dec"))
        _W[key] = host
    return _W[key]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _cand_lists(n_rows, rng, V, NT, max_len=40, empty_feed=False):
    """Ragged lists: empty rows, -1 padding, duplicates, artist columns, the last track column and column V - 1."""
    if empty_feed:
        return [[] for _ in range(n_rows)]
    out = []
    for r in range(n_rows):
        n = int(rng.integers(0, max_len))
        c = rng.integers(0, V, n)
        if n >= 4:
            c[1] = c[0]                                                    # a duplicate
            c[2] = -1
            c[3] = [NT - 1, V - 1, NT, 0][r % 4]
        out.append(c if r % 5 != 3 else c[:0])                             # every fifth row is empty
    return out


def _stream_inputs(sizes, w, seed, max_len=40, empty_at=4, short_from=None):
    """short_from: feeds of that many rows or more get lists a quarter as long, so that the stream's largest feed (which sizes
    max_candidates) holds fewer ids than two of its medium feeds together: launches then close on candidate capacity."""
    rng = np.random.default_rng(seed)
    feeds = []
    for i, n in enumerate(sizes):
        pos, ones, _seeds = make_playlists(n, w["NT"], w["V"] - w["NT"], seed=seed * 100 + i)
        ml = max_len // 4 if short_from is not None and n >= short_from else max_len
        feeds.append((pos, ones, n, _cand_lists(n, rng, w["V"], w["NT"], ml, empty_feed=(i == empty_at))))
    return feeds


def _launches(feeds_ids_rows, group_rows, max_candidates):
    """The pipeline's closing rule (csrc/pipeline_stage.h) -> (launches, how many of them closed on candidate capacity)."""
    launches, by_cand, rows, ids = 0, 0, 0, 0
    for n_rows, n_ids in feeds_ids_rows:
        if rows and (rows + n_rows > group_rows or ids + n_ids > max_candidates):
            launches += 1
            by_cand += rows + n_rows <= group_rows
            rows = ids = 0
        rows, ids = rows + n_rows, ids + n_ids
        if rows + n_rows > group_rows:
            launches, rows, ids = launches + 1, 0, 0
    return launches + (1 if rows else 0), by_cand


def _per_batch(ctx, w, pos, ones, n, lists, kind=None, rank_k=None, rank_kind=_lib.DAE_OUT_SCORE):
    """The reference: the per-batch calls on this feed alone.  kind: the listed pairs' values; rank_k: (idx, score) behind a
    host de-duplication."""
    import torch
    W_enc, b_enc, W_dec, b_dec = w["dev"]
    rp, col, val = coo_to_csr(pos, ones, n, w["V"])
    csr = (_dev(rp), _dev(col), _dev(val))
    crp, ccol = candidates_to_csr(lists, n, w["V"], unique=rank_k is not None)
    nc = int(ccol.size)
    cand = (_dev(crp), _dev(ccol if nc else np.zeros(1, np.int32)))
    out = torch.empty(max(nc, 1), dtype=torch.float32, device="cuda")
    ctx.score_candidates(csr[0], csr[1], csr[2], W_enc, b_enc, W_dec, b_dec, cand, nc, out,
                         out_kind=_lib.DAE_OUT_LOGIT if rank_k else kind)
    if rank_k is None:
        return out.cpu().numpy()[:nc]
    srp, sc = ctx.seeds_from_csr(csr[0], csr[1], w["NT"])
    score = torch.empty((n, rank_k), dtype=torch.float32, device="cuda")
    idx = torch.empty((n, rank_k), dtype=torch.int32, device="cuda")
    ctx.rank_candidates(w["V"], cand, out, int(np.diff(crp).max()), srp, sc, rank_k, score, idx, out_kind=rank_kind)
    return idx.cpu().numpy(), score.cpu().numpy()


def _pipe(w, group_rows, k=1, want_scores=True, **kw):
    W_enc, b_enc, W_dec, b_dec = w["dev"]
    return _lib.Pipeline(W_enc, b_enc, W_dec, b_dec, w["NT"], dtype=_lib.DAE_DTYPE_F32, k=k, group_rows=group_rows, max_nnz=1 << 16,
                         lanes=2, want_scores=want_scores, **kw)


def _raw_csr(lists, n):
    """The host CSR of the lists without a range check: the C level takes any id."""
    rp = np.zeros(n + 1, np.int32)
    rp[1:len(lists) + 1] = np.cumsum([len(c) for c in lists])
    rp[len(lists) + 1:] = rp[len(lists)]
    return rp, np.concatenate([np.asarray(c, np.int64) for c in lists] + [np.zeros(0, np.int64)]).astype(np.int32)


SIZES = {16: [6, 7, 1, 16, 3, 9, 2, 5, 4], 256: [6, 7, 1, 250, 3, 100, 100, 56, 30]}


@pytest.mark.parametrize("name,group_rows", [("generic", 16), ("generic", 256), ("h256", 256)])
def test_pipeline_scores_equal_the_per_batch_call_per_feed(ctx, name, group_rows):
    w = _weights(name)
    feeds = _stream_inputs(SIZES[group_rows], w, seed=group_rows, short_from=group_rows - 6)
    csrs = [_raw_csr(lists, n) for _p, _o, n, lists in feeds]
    max_cand = max(int(c[1].size) for c in csrs)                           # the largest feed fits alone: nothing is refused
    want_launches, by_cand = _launches([(n, int(c[1].size)) for (_p, _o, n, _l), c in zip(feeds, csrs)], group_rows, max_cand)
    assert by_cand >= 1
    for kind in (_lib.DAE_OUT_SCORE, _lib.DAE_OUT_LOGIT):
        pipe = _pipe(w, group_rows)
        try:
            pipe.enable_candidates(max_candidates=max_cand, rank=False, out_kind=kind)
            for (pos, ones, n, _lists), c in zip(feeds, csrs):
                assert pipe.submit_candidates(pos, ones, n, c)
            pipe.flush()
            got = [pipe.poll_candidates(True, copy=True) for _ in feeds]
            assert pipe.poll_candidates(True) is None
            st = pipe.stats()
            assert st["feeds"] == len(feeds) and st["launches"] == want_launches
        finally:
            pipe.close()
        for (pos, ones, n, lists), c, (values, bad) in zip(feeds, csrs, got):
            assert not bad and values.shape == (c[1].size,)
            assert _bits_equal(values, _per_batch(ctx, w, pos, ones, n, lists, kind=kind))
            assert np.isneginf(values[c[1] == -1]).all()
    assert got[4][0].size == 0                                             # the feed without candidates


@pytest.mark.parametrize("name,group_rows,k", [("generic", 16, 1), ("generic", 256, 10), ("generic", 256, 500), ("h256", 256, 10)])
def test_pipeline_ranks_equal_the_per_batch_call_per_feed(ctx, name, group_rows, k):
    w = _weights(name)
    feeds = _stream_inputs(SIZES[group_rows], w, seed=group_rows + 1, max_len=700 if k == 500 else 40, short_from=group_rows - 6)
    csrs = [_raw_csr(lists, n) for _p, _o, n, lists in feeds]
    max_cand = max(int(c[1].size) for c in csrs)
    pipe = _pipe(w, group_rows, k=k)
    try:
        pipe.enable_candidates(max_candidates=max_cand, rank=True, out_kind=_lib.DAE_OUT_SCORE)
        for (pos, ones, n, _lists), c in zip(feeds, csrs):
            assert pipe.submit_candidates(pos, ones, n, c)
        pipe.flush()
        got = [pipe.poll(True, copy=True) for _ in feeds]
    finally:
        pipe.close()
    fewer = 0
    for (pos, ones, n, lists), (idx, score) in zip(feeds, got):
        widx, wscore = _per_batch(ctx, w, pos, ones, n, lists, rank_k=k)
        assert idx.shape == (n, k) and np.array_equal(idx, widx) and _bits_equal(score, wscore)
        fewer += int((idx[:, -1] == -1).sum())
        for r in range(n):                                                 # every column once, however often it was listed
            real = idx[r][idx[r] >= 0]
            assert len(set(real.tolist())) == real.size
    assert fewer > 0 or k == 1                                             # rows with fewer than k candidates end in (-1, -inf)


# ---- the models' generators --------------------------------------------------------------------------------------------------------
def _model(cls, w, batch):
    class C:
        save = "/tmp/_cand_loop_unused"; lr = 0.01; reg_lambda = 0.0; initval = "NULL"
    C.batch, C.n_input, C.hidden, C.n_tracks, C.decode_dtype = batch, w["V"], w["H"], w["NT"], "f32"
    m = cls(C())
    m._host_init = lambda: [w["W_enc"], w["W_dec"], w["b_enc"], w["b_dec"]]
    m.fit()
    return m


def _same(a, b):
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_bits_equal(x, y) for x, y in zip(a, b))
    return _bits_equal(a, b)


@pytest.mark.parametrize("cls,tied", [(DAE, False), (DAE_tied, True)])
def test_model_generators_equal_the_per_batch_calls(cls, tied):
    w = _weights("generic", tied=tied)
    m = _model(cls, w, batch=250)
    m.coalesce = 2                                                         # launches of 500 rows: feeds share and split launches
    raw = _stream_inputs([6, 7, 1, 250, 3, 100, 250, 56, 30], w, seed=5)
    rng = np.random.default_rng(3)
    cands = [lists for _p, _o, _n, lists in raw]
    cands[1] = rng.integers(-1, w["V"], (7, 33)).astype(np.int32)          # the 2-D forms, with -1 padding
    cands[6] = rng.integers(-1, w["V"], (200, 12)).astype(np.int64)        # (fewer rows than the feed)
    feeds = [((pos, ones, SEEDS_FROM_INPUT, n), c) for (pos, ones, n, _l), c in zip(raw, cands)]
    m.cand_launch_ids = 4000                                               # launches close on ids; feed 3 or 6 may go per batch
    try:
        for kind in ("sigmoid", "logit"):
            got = list(m.score_candidates_iter(iter(feeds), kind=kind))
            assert len(got) == len(feeds)
            for (f, c), g in zip(feeds, got):
                assert _same(g, m.score_candidates(f[0], f[1], c, n_rows=f[3], kind=kind))
        for k in (1, 10, 500):
            got = list(m.rank_candidates_iter(iter(feeds), k=k))
            for (f, c), (idx, score) in zip(feeds, got):
                widx, wscore = m.rank_candidates(f[0], f[1], c, SEEDS_FROM_INPUT, k=k, n_rows=f[3])
                assert np.array_equal(idx, widx) and _bits_equal(score, wscore)
        assert all(s is None for _i, s in m.rank_candidates_iter(iter(feeds[:3]), k=10, want_scores=False))
        # the identity the per-batch call documents
        for f, _c in feeds[:4]:
            idx, score = m.recommend(f[0], f[1], SEEDS_FROM_INPUT, k=50, n_rows=f[3])
            (got_one,) = list(m.score_candidates_iter([(f, idx)]))
            assert _bits_equal(got_one, score)
        with pytest.raises(ValueError, match="out of range"):
            list(m.score_candidates_iter([(feeds[0][0], [[w["V"]]])]))
    finally:
        m.close_pipelines()


def _dae_title(tmp_path, w, batch):
    E, fs, F, L = TITLE

    class Conf:
        lr = 0.01; reg_lambda = 0.0; charsize = N_CHAR; char_model = 'Char_CNN'; save = "/tmp/_cand_loop_unused"
        initval = "NULL"; title_lr = 0.002
    c = Conf()
    c.batch, c.n_input, c.n_output, c.n_tracks, c.hidden = batch, w["V"], w["V"], w["NT"], w["H"]
    c.char_emb, c.filter_size, c.filter_num, c.strmaxlen = E, list(fs), F, L
    pk = tmp_path / "w_dae"
    with open(pk, "wb") as f:
        pickle.dump([w["W_enc"], w["W_dec"], w["b_enc"], w["b_dec"]], f)
    c.DAEval = str(pk)
    mt = get_model(c)
    mt.fit(tn.make_params(N_CHAR, E, fs, F, c.n_output, seed=4))
    m = DAE_title(c, mt)
    m.fit()
    return m


def _titled_feeds(raw, batch, seed):
    """Feeds with titles in use, feeds with none in use, and rows with titles_use 0 inside a titled feed."""
    L = TITLE[3]
    rng = np.random.default_rng(seed)
    feeds = []
    for i, (pos, ones, n, lists) in enumerate(raw):
        titles = rng.integers(0, N_CHAR, (batch, L))
        for r in range(batch):
            titles[r, int(rng.integers(1, L + 1)):] = -1
        use = np.zeros(batch, np.float32)
        if i % 3 != 1:                                                     # every third feed: no title in use
            use[:n] = (np.arange(n) % 3 != 0)
            if n == 1:
                use[0] = 1.0
        feeds.append(((pos, ones, SEEDS_FROM_INPUT, n, titles, use), lists))
    return feeds


def test_titled_generators_equal_the_per_batch_calls(tmp_path):
    w = _weights("generic")
    batch = 48
    m = _dae_title(tmp_path, w, batch)
    m.coalesce = 3
    feeds = _titled_feeds(_stream_inputs([6, 7, 1, 48, 3, 40, 48, 20, 30], w, seed=8), batch, seed=9)
    m.cand_launch_ids = 1500
    try:
        got = list(m.score_candidates_iter(iter(feeds)))
        for (f, c), g in zip(feeds, got):
            assert _same(g, m.score_candidates(f[0], f[1], c, n_rows=f[3], titles=f[4], titles_use=f[5]))
        for k in (1, 10, 500):
            got = list(m.rank_candidates_iter(iter(feeds), k=k))
            for (f, c), (idx, score) in zip(feeds, got):
                widx, wscore = m.rank_candidates(f[0], f[1], c, SEEDS_FROM_INPUT, k=k, n_rows=f[3], titles=f[4], titles_use=f[5])
                assert np.array_equal(idx, widx) and _bits_equal(score, wscore)
        for f, _c in feeds[:3]:                                            # the identity, titled (feed 1 has no title in use)
            idx, score = m.recommend(f[0], f[1], SEEDS_FROM_INPUT, k=50, n_rows=f[3], dtype="f32", titles=f[4], titles_use=f[5])
            (got_one,) = list(m.score_candidates_iter([(f, idx)]))
            assert _bits_equal(got_one, score)
        with pytest.raises(ValueError, match="sigmoid"):
            m.score_candidates_iter(iter(feeds), kind="logit")
    finally:
        m.close_pipelines()


# ---- de-duplication at the C level ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [3000, 1 << 20])                             # (the second: a bitmap past 64 KiB of LDS)
def test_candidates_unique(ctx, V):
    import torch
    rng = np.random.default_rng(V)
    lens = [0, 1, 255, 256, 257, 3000, 2, 0, 700]
    rows = []
    for n in lens:
        c = rng.integers(0, max(3, n // 8), n).astype(np.int64)            # heavy repetition
        c[rng.random(n) < 0.1] = -1
        c[rng.random(n) < 0.05] = V + 5                                    # out of range: passes through
        c[rng.random(n) < 0.05] = -9
        c[rng.random(n) < 0.1] = V - 1
        rows.append(c)
    rows[6] = np.array([7, 7])
    rp, col = _raw_csr(rows, len(rows))
    n_cand = int(col.size) - 5                                             # the last 5 ids lie past the caller's n_cand
    SENT = -12345
    for in_place in (False, True):
        d_in = _dev(col)
        d_out = d_in if in_place else torch.full((col.size,), SENT, dtype=torch.int32, device="cuda")
        ctx.candidates_unique(V, (_dev(rp), d_in), n_cand, out=None if in_place else d_out)
        out = d_out.cpu().numpy()
        assert np.array_equal(out[n_cand:], col[n_cand:] if in_place else np.full(5, SENT, np.int32))
        if not in_place:
            assert np.array_equal(d_in.cpu().numpy(), col)
        for r in range(len(rows)):
            a, b = int(rp[r]), min(int(rp[r + 1]), n_cand)
            src, dst = col[a:b], out[a:b]
            inr = (src >= 0) & (src < V)
            assert np.array_equal(np.sort(dst[(dst >= 0) & (dst < V)]), np.unique(src[inr]))      # each surviving column once
            assert np.array_equal(dst[~inr], src[~inr])                    # -1 and out-of-range ids untouched
            changed = dst != src
            assert (dst[changed] == -1).all() and inr[changed].all()       # every other slot: -1 in the place of a repeat
    with pytest.raises(_lib.DaeError, match="too wide for the LDS bitmap"):
        ctx.candidates_unique(_lib.DAE_CAND_UNIQUE_MAX_V + 1, (_dev(rp), _dev(col)), n_cand)


def test_rank_behind_the_kernel_equals_rank_behind_a_host_deduplication(ctx):
    import torch
    w = _weights("generic")
    n = 9
    pos, ones, _s = make_playlists(n, w["NT"], w["V"] - w["NT"], seed=77)
    rng = np.random.default_rng(78)
    lists = [rng.integers(-1, 200, L) for L in (0, 1, 255, 256, 257, 3000, 40, 2, 600)]
    W_enc, b_enc, W_dec, b_dec = w["dev"]
    rp, col, val = coo_to_csr(pos, ones, n, w["V"])
    csr = (_dev(rp), _dev(col), _dev(val))
    crp, ccol = candidates_to_csr(lists, n, w["V"])
    cand = (_dev(crp), _dev(ccol))
    ctx.candidates_unique(w["V"], cand, int(ccol.size))
    key = torch.empty(ccol.size, dtype=torch.float32, device="cuda")
    ctx.score_candidates(csr[0], csr[1], csr[2], W_enc, b_enc, W_dec, b_dec, cand, int(ccol.size), key, out_kind=_lib.DAE_OUT_LOGIT)
    srp, sc = ctx.seeds_from_csr(csr[0], csr[1], w["NT"])
    for k in (1, 10, 500):
        score = torch.empty((n, k), dtype=torch.float32, device="cuda")
        idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
        ctx.rank_candidates(w["V"], cand, key, 3000, srp, sc, k, score, idx)
        widx, wscore = _per_batch(ctx, w, pos, ones, n, lists, rank_k=k)
        assert np.array_equal(idx.cpu().numpy(), widx) and _bits_equal(score.cpu().numpy(), wscore)


# ---- nothing written past its end; the status word ----------------------------------------------------------------------------------
def test_result_block_keeps_its_sentinel_and_a_bad_id_marks_its_launch_only(ctx):
    w = _weights("generic")
    MAXC, SENT = 500, np.float32(-7.25)
    feeds = _stream_inputs([5, 9, 4], w, seed=21, empty_at=-1)
    csrs = [_raw_csr(lists, n) for _p, _o, n, lists in feeds]
    pipe = _pipe(w, 64)
    try:
        pipe.enable_candidates(max_candidates=MAXC, rank=False, out_kind=_lib.DAE_OUT_LOGIT)
        # one launch in flight at a time and every view dropped before the next: each launch gets result block 0.  The first
        # feed of a launch sits at the block's start, so its view's address is the block's
        pos, ones, n, _l = feeds[0]
        assert pipe.submit_candidates(pos, ones, n, csrs[0])
        pipe.flush()
        values, bad = pipe.poll_candidates(True)
        base = values.ctypes.data
        del values
        block = np.frombuffer((ctypes.c_float * MAXC).from_address(base), dtype=np.float32)
        block[:] = SENT
        # a launch of two feeds; the second holds two bad ids
        c1 = (csrs[1][0], csrs[1][1].copy())
        bad_at = [3, int(c1[1].size) - 1]
        c1[1][bad_at[0]], c1[1][bad_at[1]] = w["V"], -2
        for (pos, ones, n, _l), c in ((feeds[0], csrs[0]), (feeds[1], c1)):
            assert pipe.submit_candidates(pos, ones, n, c)
        pipe.flush()
        v0, bad0 = pipe.poll_candidates(True)
        v1, bad1 = pipe.poll_candidates(True)
        n0, n1 = int(csrs[0][1].size), int(c1[1].size)
        assert v0.ctypes.data == base and v1.ctypes.data == base + 4 * n0 and v0.size == n0 and v1.size == n1
        assert bad0 and bad1                                               # the word is the launch's: both of its feeds carry it
        assert (block[n0 + n1:] == SENT).all() and n0 + n1 < MAXC          # the float behind the launch's values, and all after it
        assert _bits_equal(v0, _per_batch(ctx, w, *feeds[0][:3], feeds[0][3], kind=_lib.DAE_OUT_LOGIT))
        want1 = _per_batch(ctx, w, *feeds[1][:3], feeds[1][3], kind=_lib.DAE_OUT_LOGIT)
        nan = np.isnan(v1)
        assert np.nonzero(nan)[0].tolist() == bad_at                       # NaN at the bad ids' slots only
        assert _bits_equal(v1[~nan], want1[~nan])
        del v0, v1
        # the next launch is clean: its word is not the last one's
        pos, ones, n, _l = feeds[2]
        assert pipe.submit_candidates(pos, ones, n, csrs[2])
        pipe.flush()
        v2, bad2 = pipe.poll_candidates(True)
        assert not bad2 and _bits_equal(v2, _per_batch(ctx, w, pos, ones, n, feeds[2][3], kind=_lib.DAE_OUT_LOGIT))
        del v2, block
    finally:
        pipe.close()


# ---- state refusals, by message -------------------------------------------------------------------------------------------------------
def _answers(pipe, w, rank):
    """The pipeline still takes and answers a valid feed."""
    pos, ones, _s = make_playlists(3, w["NT"], w["V"] - w["NT"], seed=1)
    assert pipe.submit_candidates(pos, ones, 3, candidates_to_csr([[1, 2], [], [3]], 3, w["V"]))
    pipe.flush()
    r = pipe.poll(True, copy=True) if rank else pipe.poll_candidates(True, copy=True)
    assert r is not None and (r[0].shape == (3, pipe.k) if rank else r[0].size == 3)


def _refused(pipe, match, call, *args):
    with pytest.raises(_lib.DaeError, match=match):
        pipe._check(call(pipe.h, *args))


def test_state_refusals(ctx, tmp_path):
    w = _weights("generic")
    lib = _lib.load()
    pos, ones, _s = make_playlists(3, w["NT"], w["V"] - w["NT"], seed=1)
    vp = ctypes.c_void_p
    feed_args = (vp(pos.ctypes.data), vp(ones.ctypes.data), 0, len(ones), 3)
    arp, acol = np.array([0, 1, 1, 2], np.int32), np.array([4, 5], np.int32)
    disc = np.ones(4, np.float64)
    for rank in (False, True):
        pipe = _pipe(w, 64, k=4)
        try:
            pipe.enable_candidates(max_candidates=100, rank=rank)
            _refused(pipe, "once, before the first submit", lib.dae_pipeline_enable_candidates, 100, 0, 0)       # twice
            _refused(pipe, "candidates pipeline", lib.dae_pipeline_enable_eval, vp(disc.ctypes.data), 100)
            cat = _lib.Catalogue(ctx, _dev(np.arange(0, 100, dtype=np.int32)), w["NT"])
            _refused(pipe, "candidates pipeline", lib.dae_pipeline_set_catalogue, cat.h)
            _refused(pipe, "takes dae_pipeline_submit_candidates only", lib.dae_pipeline_submit, *feed_args, None)
            _refused(pipe, "takes dae_pipeline_submit_candidates only", lib.dae_pipeline_submit_eval, *feed_args, None, None,
                     vp(arp.ctypes.data), vp(acol.ctypes.data), None)
            _answers(pipe, w, rank)
            t, n, b = ctypes.c_uint64(), ctypes.c_int(), ctypes.c_int()
            if rank:
                cp, cn = ctypes.POINTER(ctypes.c_float)(), ctypes.c_int64()
                _refused(pipe, "hands out lists", lib.dae_pipeline_poll_candidates, 1, ctypes.byref(t), ctypes.byref(cp), ctypes.byref(cn),
                         ctypes.byref(n), ctypes.byref(b))
            else:
                ip = ctypes.POINTER(ctypes.c_int32)()
                _refused(pipe, "hands out values", lib.dae_pipeline_poll, 1, ctypes.byref(t), ctypes.byref(ip), None, ctypes.byref(n),
                         ctypes.byref(b))
            _refused(pipe, "once, before the first submit", lib.dae_pipeline_enable_candidates, 100, 0, 0)       # after a submit
            _answers(pipe, w, rank)
            cat.close()
        finally:
            pipe.close()
    # the other modes refuse in turn; a pipeline without the mode refuses its calls
    pipe = _pipe(w, 64, k=4)
    try:
        crp, ccol = candidates_to_csr([[1, 2], [], [3]], 3, w["V"])
        _refused(pipe, "dae_pipeline_enable_candidates was not called", lib.dae_pipeline_submit_candidates, *feed_args, None, None,
                 vp(crp.ctypes.data), vp(ccol.ctypes.data), None)
        pipe.enable_eval(max_answers=100)
        _refused(pipe, "evaluation pipeline", lib.dae_pipeline_enable_candidates, 100, 0, 0)
    finally:
        pipe.close()
    pipe = _pipe(w, 64, k=4)
    try:
        cat = _lib.Catalogue(ctx, _dev(np.arange(0, 100, dtype=np.int32)), w["NT"])
        pipe.set_catalogue(cat)
        _refused(pipe, "with a catalogue", lib.dae_pipeline_enable_candidates, 100, 0, 0)
        assert pipe.submit(pos, ones, 3) and pipe.poll(True, copy=True)[0].shape == (3, 4)
    finally:
        pipe.close()
        cat.close()
    # DAE_OUT_LOGIT on a titled pipeline
    m = _dae_title(tmp_path, w, 24)
    try:
        m.sync_params()
        tp = _lib.Pipeline(m.weights["encoder_h"], m.biases["encoder_b"], m.weights["decoder_h"], m.biases["decoder_b"], w["NT"],
                           k=4, group_rows=48, max_nnz=1 << 14, lanes=1, title=m.title_model)
        try:
            with pytest.raises(_lib.DaeError, match="DAE_OUT_LOGIT on a titled pipeline"):
                tp.enable_candidates(max_candidates=100, out_kind=_lib.DAE_OUT_LOGIT)
            tp.enable_candidates(max_candidates=100, out_kind=_lib.DAE_OUT_SCORE)
            _answers(tp, w, False)
        finally:
            tp.close()
    finally:
        m.close_pipelines()


# ---- full size ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("titled", [False, True], ids=["plain", "titled"])
def test_full_size_stream_equals_the_per_batch_call_on_sampled_feeds(tmp_path, titled):
    V, NT, H, B, C = 170000, 140000, 256, 256, 1000
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=3, bias="zipf", n_tracks=NT)
    w = dict(W_enc=W_enc, b_enc=b_enc, W_dec=W_dec, b_dec=b_dec, V=V, NT=NT, H=H)
    m = _dae_title(tmp_path, w, B) if titled else _model(DAE, w, B)
    rng = np.random.default_rng(4)
    feeds = []
    for i in range(6):
        pos, ones, _s = make_playlists(B, NT, V - NT, seed=40 + i)
        f = (pos, ones, SEEDS_FROM_INPUT, B)
        if titled:
            titles = rng.integers(0, N_CHAR, (B, TITLE[3]))
            f += (titles, (np.arange(B) % 4 != 0).astype(np.float32))
        feeds.append((f, rng.integers(0, V, (B, C)).astype(np.int32)))
    try:
        got = list(m.score_candidates_iter(iter(feeds)))
        ranked = list(m.rank_candidates_iter(iter(feeds), k=500))
        for i in (0, 3, 5):                                                # sampled feeds
            f, c = feeds[i]
            kw = dict(titles=f[4], titles_use=f[5]) if titled else {}
            assert _bits_equal(got[i], m.score_candidates(f[0], f[1], c, **kw))
            widx, wscore = m.rank_candidates(f[0], f[1], c, SEEDS_FROM_INPUT, k=500, **kw)
            assert np.array_equal(ranked[i][0], widx) and _bits_equal(ranked[i][1], wscore)
    finally:
        m.close_pipelines()
