"""GPU (-m gpu): scoring and ranking caller-given candidate columns (csrc/candidates.hip) against the CPU oracle and against
the library's own dense routes.  Every comparison is `==` on the float bits: the candidate kernels run the canonical fp32 chain
of the dense decode (oracle/dae_oracle.c orc_decode) per listed (row, column)."""
import pickle

import numpy as np
import pytest

import oracle
from oracle import title_numpy as tn
from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.models.DAEs import (DAE, DAE_tied, DAE_title, SEEDS_FROM_INPUT, candidates_to_csr,
                                                            coo_to_csr)
from spotify_recsys_challenge_2018_amd.models.title_models import get_model
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights

pytestmark = pytest.mark.gpu
V, NT = 1000, 700
CHUNK = _lib.DAE_CAND_CHUNK
U32 = np.uint32


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(U32), b.view(U32))


_PROBLEMS = {}


def _problem(H, B, tied=False):
    """Weights, a batch (row 1 -- row 0 of a one-row batch -- has no input: h = sigmoid(b_enc)) and the oracle's hidden rows
    and dense logits / scores, computed once per shape and left unchanged."""
    key = (H, B, tied)
    if key not in _PROBLEMS:
        W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=H + B, bias="zipf", n_tracks=NT, tied=tied)
        b_enc = (np.random.default_rng(H + 7).standard_normal(H) * 0.1).astype(np.float32)
        pos, ones, seeds = make_playlists(B, NT, V - NT, seed=B + 1)
        empty = min(1, B - 1)
        keep = pos[:, 0] != empty
        pos, ones = pos[keep], ones[keep]
        seeds[empty] = []
        rp, col, val = coo_to_csr(pos, ones, B, V)
        h = oracle.encode(rp, col, val, W_enc, b_enc)
        assert _bits_equal(h[empty], oracle.sigmoid(b_enc))
        _PROBLEMS[key] = dict(W_enc=W_enc, b_enc=b_enc, W_dec=W_dec, b_dec=b_dec, pos=pos, ones=ones, seeds=seeds, rp=rp,
                              col=col, val=val, h=h, z=oracle.decode(h, W_dec, b_dec),
                              y=oracle.decode(h, W_dec, b_dec, apply_sigmoid=True), H=H, B=B)
    return _PROBLEMS[key]


def _random_lists(B, seed, max_len=300):
    """Unsorted lists, tracks and artists mixed, repeats allowed; one row lists every column in order."""
    rng = np.random.default_rng(seed)
    lists = [rng.integers(0, V, int(rng.integers(0, max_len))) for _ in range(B)]
    lists[B // 2] = np.arange(V)
    return lists


def _gather(dense, lists):
    return np.concatenate([dense[r, np.asarray(c, np.int64)] for r, c in enumerate(lists)] + [np.zeros(0, np.float32)])


def _decode_candidates(ctx, p, lists, kind, score_call=False):
    import torch
    B = p["B"]
    rp, col = candidates_to_csr(lists, B, V)
    n = int(col.size)
    cand = (_dev(rp), _dev(col if n else np.zeros(1, np.int32)))
    out = torch.full((n + 3,), 7.0, dtype=torch.float32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    W_dec, b_dec = _dev(p["W_dec"]), _dev(p["b_dec"])
    if score_call:
        ctx.score_candidates(_dev(p["rp"]), _dev(p["col"] if p["col"].size else np.zeros(1, np.int32)),
                             _dev(p["val"] if p["val"].size else np.zeros(1, np.float32)), _dev(p["W_enc"]), _dev(p["b_enc"]),
                             W_dec, b_dec, cand, n, out, out_kind=kind, status=status)
    else:
        ctx.decode_candidates(_dev(p["h"]), W_dec, b_dec, cand, n, out, out_kind=kind, status=status)
    o = out.cpu().numpy()
    assert (o[n:] == 7.0).all()                                  # nothing written past the list
    assert int(status.item()) == 0
    return o[:n]


@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("H", [4, 36, 100, 256, 260, 1024])
def test_oracle_parity(ctx, H, B):
    """decode_candidates == oracle.decode gathered, score_candidates == oracle.encode + oracle.decode gathered, both kinds."""
    p = _problem(H, B)
    lists = _random_lists(B, seed=H * 7 + B)
    for kind, dense in ((_lib.DAE_OUT_LOGIT, p["z"]), (_lib.DAE_OUT_SCORE, p["y"])):
        want = _gather(dense, lists)
        assert _bits_equal(_decode_candidates(ctx, p, lists, kind), want)
        assert _bits_equal(_decode_candidates(ctx, p, lists, kind, score_call=True), want)


@pytest.mark.parametrize("H,B", [(36, 3), (256, 130)])
def test_oracle_parity_tied_weights(ctx, H, B):
    """The decoder tensor IS the encoder matrix (DAE_tied): the same two calls against the same oracle."""
    p = _problem(H, B, tied=True)
    assert p["W_dec"] is p["W_enc"]
    lists = _random_lists(B, seed=H + B)
    for kind, dense in ((_lib.DAE_OUT_LOGIT, p["z"]), (_lib.DAE_OUT_SCORE, p["y"])):
        want = _gather(dense, lists)
        assert _bits_equal(_decode_candidates(ctx, p, lists, kind), want)
        assert _bits_equal(_decode_candidates(ctx, p, lists, kind, score_call=True), want)


@pytest.mark.parametrize("L", [0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 5000])
def test_row_lengths(ctx, L):
    """A row of every length at which the workgroup mapping changes, as the first and as the last row of the batch, around
    rows of other lengths; 5000 entries exceed the vocabulary: repeats."""
    p = _problem(36, 5)
    rng = np.random.default_rng(L)
    row = rng.integers(0, V, L)
    lists = [row, rng.integers(0, V, 70), np.arange(V)[::-1], rng.integers(0, V, CHUNK + 3), row[::-1]]
    got = _decode_candidates(ctx, p, lists, _lib.DAE_OUT_LOGIT)
    assert _bits_equal(got, _gather(p["z"], lists))


def test_all_rows_empty_and_many_rows(ctx):
    p = _problem(36, 130)
    assert _decode_candidates(ctx, p, [[] for _ in range(130)], _lib.DAE_OUT_LOGIT).size == 0
    lists = [[(7 * r) % V] if r % 3 else [] for r in range(130)]          # more workgroup ids than candidates
    assert _bits_equal(_decode_candidates(ctx, p, lists, _lib.DAE_OUT_SCORE), _gather(p["y"], lists))


def test_bad_ids_through_the_c_abi(ctx):
    """A device-resident list with V, -2 and -1: NaN, NaN and the status bit; -inf and no flag; every other slot correct.  The
    kernel tests the id before it forms an address: a bounds check, nothing is dereferenced."""
    import torch
    p = _problem(36, 3)
    lists = [[V, -2, -1, 5, 999], [], [-1, 0, 17]]
    rp = np.array([0, 5, 5, 8], np.int32)
    col = np.concatenate([np.asarray(c, np.int32) for c in lists])
    out = torch.full((8,), 7.0, dtype=torch.float32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.decode_candidates(_dev(p["h"]), _dev(p["W_dec"]), _dev(p["b_dec"]), (_dev(rp), _dev(col)), 8, out,
                          out_kind=_lib.DAE_OUT_LOGIT, status=status)
    o = out.cpu().numpy()
    assert np.isnan(o[0]) and np.isnan(o[1]) and int(status.item()) & 1
    assert o[2] == -np.inf and o[5] == -np.inf
    assert _bits_equal(o[3:5], p["z"][0, [5, 999]]) and _bits_equal(o[6:8], p["z"][2, [0, 17]])
    status.zero_()
    col2 = np.array([-1, 3, -1], np.int32)                                # padding alone raises no flag
    ctx.decode_candidates(_dev(p["h"]), _dev(p["W_dec"]), _dev(p["b_dec"]), (_dev(np.array([0, 3, 3, 3], np.int32)), _dev(col2)),
                          3, out, out_kind=_lib.DAE_OUT_LOGIT, status=status)
    o = out.cpu().numpy()
    assert int(status.item()) == 0 and o[0] == -np.inf and o[2] == -np.inf and _bits_equal(o[1:2], p["z"][0, [3]])


# ---- the models' methods ---------------------------------------------------------------------------------------------------
def _model(cls, p, n_tracks=NT, decode_dtype="f32"):
    class C:
        save = "/tmp/_cand_unused"; n_input = V; lr = 0.01; reg_lambda = 0.0; initval = "NULL"
    C.batch, C.hidden, C.n_tracks, C.decode_dtype = p["B"], p["H"], n_tracks, decode_dtype
    m = cls(C())
    m._host_init = lambda: [p["W_enc"], p["W_dec"], p["b_enc"], p["b_dec"]]
    m.fit()
    return m


@pytest.mark.parametrize("cls,tied", [(DAE, False), (DAE_tied, True)])
def test_model_score_candidates(cls, tied):
    p = _problem(36, 5, tied=tied)
    m = _model(cls, p)
    lists = _random_lists(5, seed=3)
    lists[4] = []
    for kind, dense in (("sigmoid", p["y"]), ("logit", p["z"])):
        got = m.score_candidates(p["pos"], p["ones"], lists, kind=kind)
        assert len(got) == 5 and all(_bits_equal(g, dense[r, np.asarray(c, np.int64)]) for r, (g, c) in enumerate(zip(got, lists)))
    got = m.score_candidates(p["pos"], p["ones"], lists[:2], n_rows=2)    # a short batch
    assert len(got) == 2 and _bits_equal(got[1], p["y"][1, lists[1]])
    a = np.array([[3, 999, -1], [-1, -1, -1], [5, 5, 0]], np.int64)       # the 2-D form with padding
    got = m.score_candidates(p["pos"], p["ones"], a, n_rows=3)
    want = np.where(a >= 0, p["y"][np.arange(3)[:, None], np.maximum(a, 0)], -np.inf).astype(np.float32)
    assert got.shape == (3, 3) and _bits_equal(got, want)
    with pytest.raises(ValueError, match="out of range"):
        m.score_candidates(p["pos"], p["ones"], [[V]])


@pytest.mark.parametrize("k", [500, 10])
@pytest.mark.parametrize("dtype", ["f32", "exact_bf16"])
def test_round_trip_with_recommend(dtype, k):
    """score_candidates(feed, idx) == score for (idx, score) = recommend(feed, k): at k = 500 over 300 tracks the lists end in
    (-1, -inf); fp32 and exact_bf16 lists carry the same fp32 scores."""
    p = _problem(128, 6)
    m = _model(DAE, p, n_tracks=300)
    idx, score = m.recommend(p["pos"], p["ones"], p["seeds"], k=k, dtype=dtype)
    assert (idx[:, -1] == -1).all() if k == 500 else (idx >= 0).all()
    got = m.score_candidates(p["pos"], p["ones"], idx)
    assert _bits_equal(got, score)


def _ranked(z, y, cands, seeds, k):
    idx = np.full((len(cands), k), -1, np.int32)
    score = np.full((len(cands), k), -np.inf, np.float32)
    for r, c in enumerate(cands):
        c = np.setdiff1d(np.unique(np.asarray(c, np.int64)), np.asarray(seeds[r], np.int64))
        c = c[c >= 0]
        order = np.lexsort((c, -z[r, c].astype(np.float64)))[:k]          # logit descending, then column ascending
        idx[r, :len(order)] = c[order]
        score[r, :len(order)] = y[r, c[order]]
    return idx, score


def test_rank_candidates():
    rng = np.random.default_rng(11)
    W_enc, b_enc, W_dec, b_dec = (a.copy() for a in make_weights(V, 36, seed=5, bias="zipf", n_tracks=NT))
    W_dec[11] = W_dec[10]; W_dec[500] = W_dec[10]
    b_dec[11] = b_dec[10]; b_dec[500] = b_dec[10]                         # three columns that tie bit for bit
    B = 6
    pos, ones, seeds = make_playlists(B, NT, V - NT, seed=9)
    p = dict(W_enc=W_enc, b_enc=b_enc, W_dec=W_dec, b_dec=b_dec, B=B, H=36)
    rp, col, val = coo_to_csr(pos, ones, B, V)
    h = oracle.encode(rp, col, val, W_enc, b_enc)
    z, y = oracle.decode(h, W_dec, b_dec), oracle.decode(h, W_dec, b_dec, apply_sigmoid=True)
    assert z[0, 10] == z[0, 11] == z[0, 500]
    m = _model(DAE, p)
    cands = [np.concatenate([[500, 11, 10, 11, 10], rng.integers(0, V, 40)]),          # given twice: ranked once
             [], np.concatenate([[11, 500, 10], rng.permutation(V)[:400]]), rng.integers(0, V, 3000),
             np.concatenate([seeds[4], [10, 500, 11]]).astype(np.int64), [-1, 7, -1, 7]]
    for k in (1, 50, 1024):                       # 1024 and 50 exceed some rows' candidate counts
        idx, score = m.rank_candidates(pos, ones, cands, seeds, k=k)
        widx, wscore = _ranked(z, y, cands, seeds, k)
        assert np.array_equal(idx, widx) and _bits_equal(score, wscore)
    idx, _s = m.rank_candidates(pos, ones, cands, [[] for _ in range(B)], k=1024)
    for r in (0, 2):
        where = [int(np.nonzero(idx[r] == c)[0][0]) for c in (10, 11, 500)]
        assert where[1] == where[0] + 1 and where[2] == where[0] + 2      # the tie comes out in column order
    assert (idx[1] == -1).all()
    # every track as a candidate: `recommend`, explicit seeds and the input's own
    for sd in (seeds, SEEDS_FROM_INPUT):
        ri, rs = m.recommend(pos, ones, sd, k=500)
        ci, cs = m.rank_candidates(pos, ones, [np.arange(NT)] * B, sd, k=500)
        assert np.array_equal(ci, ri) and _bits_equal(cs, rs)


# ---- the title mix ---------------------------------------------------------------------------------------------------------
N_CHAR = 41
TITLE_SHAPES = {"shipped": (50, [3, 5, 7, 9], 100, 25), "wave24": (25, [3, 5], 40, 25)}      # E, filter sizes, F, strmaxlen


def _dae_title(tmp_path, E, fs, F, L):
    class Conf:
        lr = 0.01; reg_lambda = 0.0; charsize = N_CHAR; char_model = 'Char_CNN'; save = "/tmp/_cand_unused"
        initval = "NULL"; title_lr = 0.002; batch = 24; n_input = 1500; n_output = 1500; n_tracks = 1200; hidden = 64
    c = Conf()
    c.char_emb, c.filter_size, c.filter_num, c.strmaxlen = E, list(fs), F, L
    W_enc, b_enc, W_dec, b_dec = make_weights(c.n_input, c.hidden, seed=1, bias="zipf", n_tracks=c.n_tracks)
    b_enc = (np.random.default_rng(2).standard_normal(c.hidden) * 0.1).astype(np.float32)
    pk = tmp_path / "w_dae"
    with open(pk, "wb") as f:
        pickle.dump([W_enc, W_dec, b_enc, b_dec], f)
    c.DAEval = str(pk)
    mt = get_model(c)
    mt.fit(tn.make_params(N_CHAR, E, fs, F, c.n_output, seed=4))
    m = DAE_title(c, mt)
    m.fit()
    return m, c


@pytest.mark.parametrize("name", sorted(TITLE_SHAPES))
def test_titled(tmp_path, name):
    """DAE_title.score_candidates == mixed_scores gathered, rows with titles_use 0 and 1 in one batch and a row without input;
    rank_candidates over all tracks == the titled recommend."""
    E, fs, F, L = TITLE_SHAPES[name]
    m, c = _dae_title(tmp_path, E, fs, F, L)
    B, nv = c.batch, c.n_input
    pos, ones, seeds = make_playlists(B, c.n_tracks, nv - c.n_tracks, seed=5)
    keep = pos[:, 0] != 4                                                 # row 4: no input, a title in use
    pos, ones = pos[keep], ones[keep]
    seeds[4] = []
    rng = np.random.default_rng(6)
    titles = rng.integers(0, N_CHAR, (B, L))
    for r in range(B):
        titles[r, int(rng.integers(0, L + 1)):] = -1
    use = (np.arange(B) % 3 != 0).astype(np.float32)
    y = m.mixed_scores(pos, ones, titles, use).cpu().numpy()
    lists = [rng.integers(0, nv, int(rng.integers(0, 400))) for _ in range(B)]
    lists[1] = np.arange(nv)
    lists[2] = []
    got = m.score_candidates(pos, ones, lists, titles=titles, titles_use=use)
    assert len(got) == B and all(_bits_equal(g, y[r, np.asarray(cl, np.int64)]) for r, (g, cl) in enumerate(zip(got, lists)))
    with pytest.raises(ValueError, match="logit"):
        m.score_candidates(pos, ones, lists, kind="logit", titles=titles, titles_use=use)
    ri, rs = m.recommend(pos, ones, seeds, k=100, titles=titles, titles_use=use)
    ci, cs = m.rank_candidates(pos, ones, [np.arange(c.n_tracks)] * B, seeds, k=100, titles=titles, titles_use=use)
    assert np.array_equal(ci, ri) and _bits_equal(cs, rs)
    # without titles in use: the base class's call
    plain = m.score_candidates(pos, ones, lists[:3], n_rows=3, titles=titles, titles_use=np.zeros(B))
    want = DAE.score_candidates(m, pos, ones, lists[:3], n_rows=3)
    assert all(_bits_equal(a, b) for a, b in zip(plain, want))


def test_a_model_with_a_scoring_shard_refuses_before_any_launch():
    p = _problem(36, 5)
    m = _model(DAE, p)
    m.shard_scoring(0, 2)
    before = m.ctx.lib.dae_scratch_bytes(m.ctx.h)
    with pytest.raises(_lib.DaeError, match="scoring shard"):
        m.score_candidates(p["pos"], p["ones"], [[1, 2]])
    with pytest.raises(_lib.DaeError, match="scoring shard"):
        m.rank_candidates(p["pos"], p["ones"], [[1, 2]], p["seeds"], k=5)
    assert m.ctx.lib.dae_scratch_bytes(m.ctx.h) == before and m._csr_status is None      # nothing uploaded, nothing reserved
