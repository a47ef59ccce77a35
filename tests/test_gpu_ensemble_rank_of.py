"""GPU (-m gpu): ranks under the ensemble -- dae_ensemble_candidates, dae_ensemble_rank_of, DAE_ensemble.rank_of / fit_alphas and
the drivers' keys (DESIGN.md 4e "Ranks under the ensemble").

Expected values never come from the code under test.  Per member oracle.encode -> oracle.decode(sigmoid) (the shapes, feeds,
members and title scorers of tests/test_gpu_ensemble.py, computed once and shared with it), combined by its `_chain` in numpy
float32 in the contract's order, title_numpy.mix_weights for the titled cases; oracle.topk(k = n_tracks, seeds, DAE_OUT_LOGIT)
over y is the whole canonical ordering of a row and a column's rank its place in it.  Ranks are compared as integers, scores by
their bits, every listed answer is compared.  A case's reference is computed once and shared."""
import os
import pickle
import re
import shutil

import numpy as np
import pytest

import oracle
from oracle import title_numpy as tn
from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.models.DAEs import DAE, DAE_title, SEEDS_FROM_INPUT, coo_to_csr, seeds_to_csr
from spotify_recsys_challenge_2018_amd.models.ensemble import DAE_ensemble
from spotify_recsys_challenge_2018_amd.models.title_models import get_model
from spotify_recsys_challenge_2018_amd.utils import metrics as met
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights
from test_gpu_ensemble import (BIG, MID, NO_INPUT, SMALL, ZERO_ALPHA, Ctxs, _alphas, _bits, _call, _chain, _dev, _feed, _member,
                               _nt32, _poison, _some, _title)
from test_gpu_rank_of_mix import _csr, _okey, _order_and_place, _stable_plan

pytestmark = pytest.mark.gpu
F32 = _lib.DAE_DTYPE_F32
DUP_SEED_ROW = 4


# ---- a case and its reference: computed once, shared, left unchanged ---------------------------------------------------------------
CASES = {
    # shape, members (hidden, kind) in the order of the sum, title feature width or None, a seed CSR given
    "M1-small": (SMALL, [(64, "plain")], None, True),
    "M2-mid-h256-x40-last": (MID, [(96, "plain"), (256, "x40")], None, True),
    "M2-mid-no-seed-csr": (MID, [(96, "plain"), (256, "x40")], None, False),
    "M1-big-x40-every-other-score-ties": (BIG, [(256, "x40")], None, True),
    "M3-big-h256-last": (BIG, [(320, "plain"), (64, "dup"), (256, "plain")], None, True),
    "M4-big-generic-last": (BIG, [(256, "plain"), (256, "x40"), (64, "dup"), (320, "plain")], None, True),
    "titled-M1-mid": (MID, [(96, "plain")], 128, True),
    "titled-M3-big": (BIG, [(256, "plain"), (256, "x40"), (320, "plain")], 256, True),
    "titled-M2-small": (SMALL, [(64, "plain"), (96, "plain")], 64, True),
}
_REFS = {}


def _ref(name):
    """-> dict: the members, the weights a_m as the call takes them, y [B, n_tracks], the seeds (row 0 none, row 1 250, row 2 its
    own top 50 under y, row DUP_SEED_ROW one listed twice), the canonical order and every track's place in it."""
    if name in _REFS:
        return _REFS[name]
    shape, spec, F, seeded = CASES[name]
    V, nt, B = shape
    members = [_member(shape, H, kind) for H, kind in spec]
    title = _title(shape, F) if F else None
    alpha = list(_alphas(len(members), B))
    sig = [m["s"][:, :nt] for m in members]
    if title is not None:
        a = [(x * title["w_p"]).astype(np.float32) for x in alpha]
        y = _chain(sig, a, title["ts"], title["w_t"])
    else:
        a, y = alpha, _chain(sig, alpha)
    if seeded:
        rng = np.random.default_rng(V + B)
        seeds = [sorted(set(int(c) for c in s)) for s in _feed(shape)["seeds"]]
        seeds[0] = []
        seeds[1] = np.sort(np.concatenate([np.arange(100), 100 + rng.permutation(nt - 100)[:150]])).tolist()
        seeds[2] = sorted(int(c) for c in np.lexsort((np.arange(nt), -_okey(y[2])))[:50])
        seeds[DUP_SEED_ROW] = (seeds[DUP_SEED_ROW] or [7]) + (seeds[DUP_SEED_ROW] or [7])[:1]
        srp, sc = _csr(seeds, B)
    else:
        seeds, srp, sc = [[] for _ in range(B)], None, None
    order, place = _order_and_place(y, nt, srp, sc)
    hr = F if F else spec[-1][0]                                  # the ranking scorer's row width: the plan's H
    _REFS[name] = dict(shape=shape, V=V, nt=nt, B=B, members=members, title=title, a=a, y=y, seeds=seeds, srp=srp, sc=sc,
                       order=order, place=place, hr=hr)
    return _REFS[name]


def _prefix(p, n):
    """The first n rows of a case as a case of its own (rows are independent)."""
    q = dict(p)
    q["B"] = n
    q["members"] = [dict(m, h=m["h"][:n]) for m in p["members"]]
    q["a"] = [x[:n] for x in p["a"]]
    if p["title"] is not None:
        q["title"] = dict(p["title"], feat=p["title"]["feat"][:n], w_t=p["title"]["w_t"][:n])
    for k in ("y", "order", "place"):
        q[k] = p[k][:n]
    q["seeds"] = p["seeds"][:n]
    if p["srp"] is not None:
        q["srp"], q["sc"] = p["srp"][:n + 1], p["sc"][:p["srp"][n]]
    return q


def _want(p, lists):
    """(ranks, scores) of the listed answers by the reference, flattened in list order."""
    nt, V = p["nt"], p["V"]
    ranks, scores = [], []
    for r, cs in enumerate(lists):
        yr, pr = p["y"][r], p["place"][r]
        for c in np.asarray(cs, np.int64):
            ok = 0 <= c < nt
            ranks.append(int(pr[c]) if ok else -1)
            scores.append(yr[c] if ok and pr[c] >= 0 else (np.float32(-np.inf) if -1 <= c < V else np.float32(np.nan)))
    return np.asarray(ranks, np.int32), np.asarray(scores, np.float32)


def _list_of(p, r, L, rng):
    """A row's answers, L of them: its best and its worst rankable column, padding, an artist, a seed, a repeat, then random
    tracks -- shuffled."""
    nt, V = p["nt"], p["V"]
    o = p["order"][r]
    o = o[o >= 0]
    special = [int(o[0]), int(o[-1]), -1, nt + (r % (V - nt)), int(o[0])]
    if p["seeds"][r]:
        special.insert(2, int(p["seeds"][r][0]))
    cs = np.asarray((special + rng.integers(0, nt, max(L - len(special), 0)).tolist())[:L], np.int64)
    return rng.permutation(cs)


def _edge_lists(p, C, seed):
    """Row lengths 0, 1, C, C + 1, 3 C + 5 on the first rows, an edge length on the last one too; the rows without input and the
    row of zero weights are asked; the others hold 0 or 1 answer, so the batch's average stays small."""
    B = p["B"]
    rng = np.random.default_rng(seed)
    lens = [r % 2 for r in range(B)]
    for r in NO_INPUT:
        if r < B:
            lens[r] = 9
    if B > 5:
        lens[B - 1] = C + 1
        lens[5] = 7
    for r, L in zip(range(5), (0, 1, C, C + 1, 3 * C + 5)):
        lens[r] = L
    return [_list_of(p, r, L, rng) for r, L in enumerate(lens)]


def _tensors(cx, p):
    """What a call takes besides the lists, on the device; the decoder tensors are the ones the contexts were packed from."""
    M = len(p["members"])
    t = dict(hs=[_dev(m["h"]) for m in p["members"]], a=[_dev(x) for x in p["a"]], Wd=cx.keep[0:2 * M:2], bd=cx.keep[1:2 * M:2], kw={})
    if p["title"] is not None:
        t["kw"] = dict(feat=_dev(p["title"]["feat"]), OutW_T=cx.keep[2 * M], Out_b=cx.keep[2 * M + 1], w_title=_dev(p["title"]["w_t"]))
    return t


def _rank_of(cx, p, lists, status_want=0, seeds=True):
    """One dae_ensemble_rank_of through the ctypes wrapper -> (ranks, scores) on the host; nothing may be written past n_ans."""
    import torch
    rp, col = _csr(lists, p["B"])
    n = int(col.size)
    ans = (_dev(rp), _dev(_some(col, np.int32)))
    rank = torch.full((n + 3,), -7, dtype=torch.int32, device="cuda")
    score = torch.full((n + 3,), 7.0, dtype=torch.float32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    srp, sc = (_dev(p["srp"]), _dev(_some(p["sc"], np.int32))) if seeds and p["srp"] is not None else (None, None)
    t = _tensors(cx, p)
    cx.ranker().ensemble_rank_of(cx.m, t["hs"], t["a"], t["Wd"], t["bd"], p["nt"], srp, sc, ans, n, rank, out_score=score,
                                 status=status, **t["kw"])
    r, s = rank.cpu().numpy(), score.cpu().numpy()
    assert (r[n:] == -7).all() and (s[n:] == 7.0).all(), "the slack past n_ans was written"
    assert int(status.item()) == status_want
    return r[:n], s[:n]


def _scratch(cx):
    return sum(c.lib.dae_scratch_bytes(c.h) for c in cx.m + ([cx.t] if cx.t is not None else []))


# ---- 1. against the oracle through the C ABI ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_rank_of_is_the_oracle_order_twice_with_poisoned_scratch(name):
    p = _ref(name)
    shape, V, nt, B = p["shape"], p["V"], p["nt"], p["B"]
    plan, lists = _stable_plan(B, p["hr"], lambda C: _edge_lists(p, C, seed=B + p["hr"]))
    C = plan["capacity"]
    assert {0, 1, C, C + 1, 3 * C + 5} <= {len(x) for x in lists} and len(lists[B - 1]) in (C + 1, 3 * C + 5)
    wr, ws = _want(p, lists)
    # what the lists and the case hold: rank 0, a row's last rank, every kind of unrankable answer; the row of zero weights ties
    n_rankable = int((p["order"][4] >= 0).sum())
    assert 0 in wr and (n_rankable - 1) in wr and -1 in wr
    assert (p["y"][ZERO_ALPHA] == 0).all() or p["title"] is not None
    if p["srp"] is not None:
        assert not p["seeds"][0] and len(p["seeds"][1]) == 250 and len(p["seeds"][2]) == 50
        assert len(p["seeds"][DUP_SEED_ROW]) == len(set(p["seeds"][DUP_SEED_ROW])) + 1
    if name == "M1-big-x40-every-other-score-ties":
        assert max(np.unique(p["y"][0], return_counts=True)[1]) > 300          # hundreds of tied y
    if name == "M2-mid-h256-x40-last":                                         # the ranking member's sigmoids saturate: hundreds of ties
        assert max(np.unique(p["members"][1]["s"][0, :nt], return_counts=True)[1]) > 300
    cx = Ctxs(p["members"], p["title"])
    try:
        for rep in range(2):
            r, s = _rank_of(cx, p, lists)
            bad = np.nonzero(r != wr)[0]
            assert bad.size == 0, (plan, "call %d" % rep, bad[:10], r[bad[:10]], wr[bad[:10]])
            assert np.array_equal(_bits(s), _bits(ws)), "scores differ (call %d)" % rep
            if rep == 0:
                _poison(cx, p["members"], shape, p["title"])
    finally:
        cx.close()


# ---- 2. dae_ensemble_candidates alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec, F", [
    pytest.param([(96, "plain"), (256, "x40")], 128, id="titled-M2"),
    pytest.param([(96, "plain"), (256, "x40"), (64, "plain")] * 3, None, id="M9-two-combining-launches"),
    pytest.param([(64, "plain")], None, id="M1"),
])
def test_candidates_are_the_numpy_chain_at_every_listed_pair(spec, F):
    """Every listed pair, artists included, by bits; -1 gives -inf; an id >= V gives NaN and status bit 0.  The call needs no image:
    the contexts are fresh."""
    import torch
    shape = MID
    V, nt, B = shape
    members = [_member(shape, H, kind) for H, kind in spec]
    title = _title(shape, F) if F else None
    M = len(members)
    alpha = list(_alphas(M, B, seed=2))
    sig = {id(m): oracle.decode(m["h"], m["W"][2], m["W"][3], 0, V, apply_sigmoid=True) for m in members}
    if title is not None:
        a = [(x * title["w_p"]).astype(np.float32) for x in alpha]
        y = _chain([sig[id(m)] for m in members], a, oracle.decode(title["feat"], title["OutW_T"], title["Out_b"], 0, V, apply_sigmoid=True),
                   title["w_t"])
    else:
        a, y = alpha, _chain([sig[id(m)] for m in members], alpha)
    rng = np.random.default_rng(M + 40)
    lists = [rng.integers(0, V, (0, 1, 300, 257, 5)[r % 5]) for r in range(B)]
    lists[2][:3] = (-1, nt, V - 1)
    ctxs = [_lib.Context(0) for _ in range(M + (1 if title is not None else 0))]
    try:
        ranker = ctxs[-1]
        Wd, bd = [_dev(m["W"][2]) for m in members], [_dev(m["W"][3]) for m in members]
        kw = {}
        if title is not None:
            kw = dict(feat=_dev(title["feat"]), OutW_T=_dev(title["OutW_T"]), Out_b=_dev(title["Out_b"]), w_title=_dev(title["w_t"]))

        def run(ls, status_want):
            rp, col = _csr(ls, B)
            n = int(col.size)
            out = torch.full((n + 3,), 7.0, dtype=torch.float32, device="cuda")
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            ranker.ensemble_candidates(ctxs[:M], [_dev(m["h"]) for m in members], [_dev(x) for x in a], Wd, bd,
                                       (_dev(rp), _dev(_some(col, np.int32))), n, out, status=status, **kw)
            got = out.cpu().numpy()
            assert (got[n:] == 7.0).all() and int(status.item()) == status_want
            rows = np.repeat(np.arange(B), np.diff(rp))
            return got[:n], rows, col.astype(np.int64)
        got, rows, col = run(lists, 0)
        ok = col >= 0
        assert (col >= nt).any() and np.array_equal(_bits(got[ok]), _bits(y[rows[ok], col[ok]]))
        assert np.isneginf(got[~ok]).all() and (~ok).sum() == 1
        bad = [np.asarray(x).copy() for x in lists]
        bad[2][5], bad[3][0], bad[3][1] = V, V + 9, -2
        got2, rows, col2 = run(bad, 1)
        out_of_range = (col2 >= V) | (col2 < -1)
        assert out_of_range.sum() == 3 and np.isnan(got2[out_of_range]).all()
        assert np.array_equal(_bits(got2[~out_of_range]), _bits(got[~out_of_range]))
    finally:
        for c in ctxs:
            c.close()


# ---- 3. one set of contexts across sizes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["M3-big-h256-last", "titled-M3-big"])
def test_one_set_of_contexts_across_sizes_equals_fresh_contexts(name):
    """257 -> 5 -> 37 rows on ONE set of contexts behind poisoned scratch; nothing is reset in between, and a steady state
    allocates nothing."""
    big = _ref(name)
    rng = np.random.default_rng(12)
    calls = []
    for n, lens in ((257, (25, 31, 0, 3)), (5, (0, 1, 140, 7)), (37, (3, 0, 60, 1))):
        q = big if n == 257 else _prefix(big, n)
        calls.append((q, [_list_of(q, r, lens[r % 4], rng) for r in range(n)]))
    one = Ctxs(big["members"], big["title"])
    try:
        _poison(one, big["members"], big["shape"], big["title"])
        got = [_rank_of(one, q, lists) for q, lists in calls]
        again = _rank_of(one, *calls[0])
        grown = _scratch(one)
        again2 = _rank_of(one, *calls[0])
        assert _scratch(one) == grown
    finally:
        one.close()
    for (q, lists), (r, s) in zip(calls, got):
        fresh = Ctxs(big["members"], big["title"])
        try:
            fr, fs = _rank_of(fresh, q, lists)
        finally:
            fresh.close()
        wr, ws = _want(q, lists)
        assert np.array_equal(r, fr) and np.array_equal(_bits(s), _bits(fs))
        assert np.array_equal(r, wr) and np.array_equal(_bits(s), _bits(ws))
    for x in (again, again2):
        assert np.array_equal(x[0], got[0][0]) and np.array_equal(_bits(x[1]), _bits(got[0][1]))


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    import torch
    p = _ref("M2-mid-h256-x40-last")
    V, nt, B = p["shape"]
    cx = Ctxs(p["members"])
    t = _tensors(cx, p)
    lists = [[1, 2, 3]] * B
    rp, col = _csr(lists, B)
    n = int(col.size)
    ans = (_dev(rp), _dev(col))
    srp, sc = _dev(p["srp"]), _dev(p["sc"])
    rank = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    score = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")

    def refused(match, ctxs=None, hs=None, srp_=srp, sc_=sc, n_seed=None, n_=n, ans_=ans, Wd=None):
        before = _scratch(cx)
        with pytest.raises(_lib.DaeError, match=match):
            cx.ranker().ensemble_rank_of(ctxs or cx.m, hs or t["hs"], t["a"], Wd or t["Wd"], t["bd"], nt, srp_, sc_, ans_, n_, rank,
                                         out_score=score, n_seed=n_seed)
        torch.cuda.synchronize()
        assert _scratch(cx) == before and bool((rank == -7).all()) and bool((score == 7.0).all()), match
    try:
        refused("listed twice", ctxs=[cx.m[1], cx.m[1]], hs=[t["hs"][1], t["hs"][1]])
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            cx.m[0].bind_stream()
        refused("another stream")
        cx.m[0].bind_stream()
        Wd0, bd0 = t["Wd"][0], t["bd"][0]
        c2 = _lib.Context(0)                                      # a bf16 image is no fp32 image
        try:
            c2.prepack_decoder(Wd0, bd0, dtype=_lib.DAE_DTYPE_BF16)
            refused("member 0 holds no image prepacked for dtype 0", ctxs=[c2, cx.m[1]])
        finally:
            c2.close()
        refused("n_seed=4 without a seed CSR", srp_=None, sc_=None, n_seed=4)
        refused("n_seed=-1", n_seed=-1)
        refused("both be given or both null", sc_=None, n_seed=0)
        refused("does not match", hs=[t["hs"][1], t["hs"][1]], Wd=[t["Wd"][1], t["Wd"][1]])
        refused("n_ans=-1", n_=-1)
        refused("null pointer", ans_=(None, ans[1]))
        mixT = torch.zeros((_nt32(nt, V), B), dtype=torch.float32, device="cuda")
        for c in cx.m:
            c.set_score_mix(mixT, t["a"][0])
            refused("dae_set_score_mix")
            c.set_score_mix()
        # n_ans == 0 returns DAE_OK and writes nothing; and the same call goes through once nothing is wrong
        cx.ranker().ensemble_rank_of(cx.m, t["hs"], t["a"], t["Wd"], t["bd"], nt, srp, sc, ans, 0, rank, out_score=score)
        torch.cuda.synchronize()
        assert bool((rank == -7).all()) and bool((score == 7.0).all())
        r, s = _rank_of(cx, p, lists)
        wr, ws = _want(p, lists)
        assert np.array_equal(r, wr) and np.array_equal(_bits(s), _bits(ws))
        # an id >= V: rank -1, a NaN score, status bit 0; an out-of-range SEED raises no status
        bad = [[5, V, 6], [V + 7, 9]] + [[11]] * (B - 2)
        r, s = _rank_of(cx, p, bad, status_want=1)
        wr, ws = _want(p, bad)
        assert np.array_equal(r, wr) and np.isnan(s[[1, 3]]).all() and np.array_equal(_bits(np.delete(s, [1, 3])), _bits(np.delete(ws, [1, 3])))
        q = dict(p, sc=np.where(np.arange(p["sc"].size) == 3, V + 5, p["sc"]).astype(np.int32))
        q["seeds"] = [list(x) for x in p["seeds"]]
        srp_h = p["srp"]
        row3 = int(np.searchsorted(srp_h, 3, side="right") - 1)
        gone = int(p["sc"][3])
        q["seeds"][row3] = [c for c in q["seeds"][row3] if c != gone]
        q["order"], q["place"] = _order_and_place(q["y"], nt, *_csr(q["seeds"], B))
        r, s = _rank_of(cx, q, [[gone, 4, 50]] * B)
        wr, ws = _want(q, [[gone, 4, 50]] * B)
        assert np.array_equal(r, wr) and np.array_equal(_bits(s), _bits(ws))
    finally:
        cx.close()


# ---- 5. the model --------------------------------------------------------------------------------------------------------------------
PV, PNT, PB, N_CHAR, L = 6000, 5000, 6, 41, 25


class Conf:
    batch = PB; n_input = PV; n_output = PV; n_tracks = PNT; hidden = 64; lr = 0.01; reg_lambda = 0.0
    char_emb = 25; strmaxlen = L; charsize = N_CHAR; char_model = 'Char_CNN'; filter_num = 40; filter_size = [3, 5]
    save = "/tmp/_ens_rank_of_unused"; initval = "NULL"; DAEval = "NULL"; title_lr = 0.002


def _weights(conf, H, seed, shuffled=False):
    """(W_enc, b_enc, W_dec, b_dec); shuffled: the decoder's track rows (and biases) permuted -- another popularity order."""
    W = make_weights(conf.n_input, H, seed=seed, bias="zipf", n_tracks=conf.n_tracks)
    if shuffled:
        perm = np.random.default_rng(seed).permutation(conf.n_tracks)
        W_dec, b_dec = W[2].copy(), W[3].copy()
        W_dec[:conf.n_tracks], b_dec[:conf.n_tracks] = W[2][perm], W[3][perm]
        W = (W[0], W[1], W_dec, b_dec)
    return W


def _dae(H, seed, conf=Conf, cls=DAE, title_model=None, shuffled=False):
    """-> (a fitted model, its weights (W_enc, b_enc, W_dec, b_dec))."""
    c = conf()
    c.hidden = H
    m = cls(c, title_model) if title_model is not None else cls(c)
    W = _weights(c, H, seed, shuffled)
    m._host_init = lambda: [W[0], W[2], W[1], W[3]]
    m.fit()
    return m, W


@pytest.fixture(scope="module")
def py_problem():
    pos, ones, seeds = make_playlists(PB, PNT, PV - PNT, seed=22)
    keep = pos[:, 0] != 4                                         # row 4: no input, a title in use
    pos, ones = pos[keep], ones[keep]
    seeds[4] = []
    rng = np.random.default_rng(23)
    titles = rng.integers(0, N_CHAR, (PB, L))
    for r in range(PB):
        titles[r, int(rng.integers(1, L + 1)):] = -1
    tm = get_model(Conf())
    tm.fit(tn.make_params(N_CHAR, 25, [3, 5], 40, PV, seed=4))
    ms = [_dae(64, 31)[0], _dae(96, 32)[0]]
    return dict(pos=pos, ones=ones, seeds=seeds, titles=titles, use=np.asarray([1, 0, 1, 1, 1, 0], np.float32), tm=tm, ms=ms)


@pytest.mark.parametrize("titled", [False, True])
@pytest.mark.parametrize("seeds_from_input", [False, True])
def test_ranks_of_a_recommended_list_are_its_positions(py_problem, titled, seeds_from_input):
    g = py_problem
    ens = DAE_ensemble(g["ms"], alphas=[0.3, 0.7], title_model=g["tm"] if titled else None)
    kw = dict(titles=g["titles"], titles_use=g["use"]) if titled else {}
    seeds = SEEDS_FROM_INPUT if seeds_from_input else g["seeds"]
    k = 500
    idx, score = ens.recommend(g["pos"], g["ones"], seeds, k=k, dtype="f32", **kw)
    assert (idx >= 0).all()
    cols = np.concatenate([idx, np.full((PB, 2), -1, idx.dtype)], axis=1)
    ranks, scores = ens.rank_of(g["pos"], g["ones"], cols, seeds, want_scores=True, **kw)
    assert ranks.dtype == np.int32 and ranks.shape == cols.shape and scores.dtype == np.float32
    assert np.array_equal(ranks[:, :k], np.tile(np.arange(k, dtype=np.int32), (PB, 1)))
    assert (ranks[:, k:] == -1).all() and np.isneginf(scores[:, k:]).all()
    assert np.array_equal(_bits(scores[:, :k]), _bits(score))
    ragged = ens.rank_of(g["pos"], g["ones"], [idx[0, ::-1], [], idx[2, :3]], seeds, **kw)
    assert len(ragged) == PB and np.array_equal(ragged[0], np.arange(k)[::-1]) and ragged[1].size == 0
    assert np.array_equal(ragged[2], [0, 1, 2]) and all(x.size == 0 for x in ragged[3:])


def test_titled_single_member_alpha_one_is_mixed_rank_of(py_problem):
    g = py_problem
    dt, _W = _dae(64, 31, cls=DAE_title, title_model=g["tm"])
    ens = DAE_ensemble([g["ms"][0]], alphas=[1.0], title_model=g["tm"])
    rng = np.random.default_rng(5)
    cols = rng.integers(0, PNT, (PB, 200))
    cols[:, 0], cols[:, 1], cols[0, 2] = -1, PNT + 5, g["seeds"][0][0]
    for seeds in (g["seeds"], SEEDS_FROM_INPUT):
        a = dt.mixed_rank_of(g["pos"], g["ones"], cols, seeds, g["titles"], g["use"], want_scores=True)
        b = ens.rank_of(g["pos"], g["ones"], cols, seeds, titles=g["titles"], titles_use=g["use"], want_scores=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


@pytest.mark.parametrize("titled", [False, True])
def test_ranks_equal_the_dense_route_ordered_on_the_host(py_problem, titled):
    g = py_problem
    per_row = np.asarray([[0.2, 0.9, 0.0, 0.5, 0.4, 0.6], [0.8, 0.1, 0.0, 0.5, 0.7, 0.3]], np.float32)     # row 2: every weight 0
    ens = DAE_ensemble(g["ms"], alphas=per_row, title_model=g["tm"] if titled else None)
    kw = dict(titles=g["titles"], titles_use=g["use"]) if titled else {}
    rng = np.random.default_rng(24)
    cols = rng.integers(0, PNT, (PB, 300))
    cols[:, 0], cols[:, 1], cols[0, 2] = -1, PNT + 5, g["seeds"][0][0]
    ranks, scores = ens.rank_of(g["pos"], g["ones"], cols, g["seeds"], want_scores=True, **kw)
    y = ens.ensemble_scores(g["pos"], g["ones"], dtype="f32", **kw)
    for r in range(PB):
        sd = np.asarray(sorted(set(g["seeds"][r])), np.int64)
        live = np.setdiff1d(np.arange(PNT), sd)
        order = live[np.lexsort((live, -_okey(y[r, live])))]
        place = np.full(PV, -1, np.int64)
        place[order] = np.arange(order.size)
        want = np.where(cols[r] >= 0, place[np.maximum(cols[r], 0)], -1)
        assert np.array_equal(ranks[r], want), r
        ok = want >= 0
        assert np.array_equal(_bits(scores[r][ok]), _bits(y[r, cols[r][ok]])) and np.isneginf(scores[r][~ok]).all()


# ---- 6. fit_alphas ---------------------------------------------------------------------------------------------------------------------
class FitConf(Conf):
    batch = 37; n_input = 3301; n_output = 3301; n_tracks = 2990


@pytest.fixture(scope="module")
def fit_problem():
    """Members A, B, C with unrelated random weights (B's and C's decoders rank the tracks by popularity orders of their own);
    every row's answers are the columns at places 0 .. 9 of A's own canonical order (seeds removed), by the oracle."""
    c = FitConf()
    V, nt, B = c.n_input, c.n_tracks, c.batch
    pos, ones, seeds = make_playlists(B, nt, V - nt, seed=9)
    keep = ~np.isin(pos[:, 0], NO_INPUT)
    pos, ones = pos[keep], ones[keep]
    rp, col, val = coo_to_csr(pos, ones, B, V)
    srp, sc = seeds_to_csr(seeds, B, nt)
    ms, sig = [], []
    for H, seed in ((64, 41), (96, 42), (64, 43)):
        m, W = _dae(H, seed, conf=FitConf, shuffled=seed != 41)
        ms.append(m)
        sig.append(oracle.decode(oracle.encode(rp, col, val, W[0], W[1]), W[2], W[3], 0, nt, apply_sigmoid=True))
    order_a, _place = _order_and_place(sig[0], nt, srp, sc)
    answers = [[int(x) for x in order_a[r][:10]] for r in range(B)]
    assert all(min(a) >= 0 for a in answers)

    def metric(alphas, n_members, name="mrr"):
        """The metric by the oracle: y of the first n_members members at these alphas, the answers' places, utils/metrics.py."""
        a = [np.full(B, x, np.float32) for x in np.asarray(alphas, np.float32)]
        _o, place = _order_and_place(_chain(sig[:n_members], a), nt, srp, sc)
        ranks = np.concatenate([place[r][answers[r]] for r in range(B)])
        return met.mean_reciprocal_rank(ranks) if name == "mrr" else float(met.recall_at(ranks, [int(name.split("@")[1])])[0])
    return dict(ms=ms, feeds=[(pos, ones, answers, seeds, B)], metric=metric)


def test_fit_alphas_prefers_the_member_the_answers_come_from(fit_problem):
    g = fit_problem
    only_a, only_b = g["metric"]([1, 0], 2), g["metric"]([0, 1], 2)
    assert only_a > 2 * only_b, (only_a, only_b)                  # the reference separates the corners
    ens = DAE_ensemble(g["ms"][:2])
    alphas, value, trace = ens.fit_alphas(g["feeds"], steps=10)
    assert np.array_equal(ens.alphas, alphas) and alphas.dtype == np.float32 and len(trace) == 11
    assert alphas[0] >= alphas[1]
    at = {tuple(np.round(a * 10).astype(int)): v for a, v in trace}
    assert value >= at[(10, 0)] and value >= at[(0, 10)] and value >= at[(5, 5)]
    assert at[(10, 0)] == only_a and at[(0, 10)] == only_b
    assert value == g["metric"](alphas, 2)
    a2, v2, _t = DAE_ensemble(g["ms"][:2]).fit_alphas(g["feeds"], metric="recall@10", steps=4)
    assert v2 == g["metric"](a2, 2, "recall@10")


def test_fit_alphas_three_members_ends_on_a_pair_move_optimum(fit_problem):
    g = fit_problem
    ens = DAE_ensemble(g["ms"])
    alphas, value, trace = ens.fit_alphas(g["feeds"], steps=4)
    pt = np.round(alphas * 4).astype(int)
    assert np.array_equal(alphas, (pt / np.float32(4)).astype(np.float32)) and pt.sum() == 4 and (pt >= 0).all()
    keys = [tuple(np.round(a * 4).astype(int)) for a, _v in trace]
    assert len(set(keys)) == len(keys)
    assert value == g["metric"](alphas, 3)
    for i in range(3):
        for j in range(3):
            if i != j and pt[j] > 0:
                q = pt.copy()
                q[i] += 1
                q[j] -= 1
                assert g["metric"](q / np.float32(4), 3) <= value, (pt, q)


# ---- 7. the drivers ------------------------------------------------------------------------------------------------------------------
def test_drivers_log_the_ensemble_ranks_and_fit_the_alphas(tmp_path):
    """main.py --dae --testmode on the golden mini dataset with [BASE] ensemble: eval_ensemble_ranks = on logs exactly one more
    line per split, whose numbers are those of `DAE_ensemble.rank_of` driven by hand; ensemble_fit = 5 logs the fitted alphas, and
    the lines behind it are those of an ensemble constructed with these alphas."""
    from spotify_recsys_challenge_2018_amd import main as cli
    from spotify_recsys_challenge_2018_amd.main_runner import main_train
    from spotify_recsys_challenge_2018_amd.models import ensemble as E
    from spotify_recsys_challenge_2018_amd.utils.data_reader import data_reader_challenge, data_reader_test
    G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    work = tmp_path / "run"
    work.mkdir()
    shutil.copytree(os.path.join(G, "data"), tmp_path / "data")
    ini = open(os.path.join(G, "config.ini")).read()
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        open(work / "config.ini", "w").write(ini)
        conf = cli.load_conf("run")
        conf.set_dae_conf()
        rd = data_reader_challenge(data_dir=conf.data_dir, filename="challenge_inorder_5to100", batch_size=5)
        V, nt = rd.num_items, rd.num_tracks
        for name, H, seed in (("w_dae", 32, 1), ("w_other", 96, 2)):
            W = make_weights(V, H, seed=seed, bias="zipf", n_tracks=nt)
            pickle.dump([W[0], W[2], W[1], W[3]], open(work / name, "wb"))
        splits = ("test-0", "test-1", "test-5", "test-25r")

        def testmode_lines(base_keys):
            open(work / "config.ini", "w").write(ini.replace("[BASE]", "[BASE]\n" + base_keys))
            n0 = len(open(work / "log.txt").read().splitlines()) if os.path.exists(work / "log.txt") else 0
            assert cli.main(["--dir", "run", "--dae", "--testmode"]) == 0
            new = open(work / "log.txt").read().splitlines()[n0:]
            return [l for l in new if l.startswith("seed num")], [l for l in new if l.startswith("ensemble:")]
        plain, said = testmode_lines("ensemble = w_other\nensemble_alpha = 0.25, 0.75")
        assert len(plain) == 4 and len(said) == 1
        assert testmode_lines("ensemble = w_other\nensemble_alpha = 0.25, 0.75\neval_ensemble_ranks = off")[0] == plain
        full, _said = testmode_lines("ensemble = w_other\nensemble_alpha = 0.25, 0.75\neval_ensemble_ranks = on")
        assert len(full) == 8 and full[:4] == plain

        def by_hand(alphas):
            class C:
                batch = conf.batch; n_input = V; n_tracks = nt; hidden = 32; lr = 0.005; reg_lambda = 0.0; save = "x"
                initval = str(work / "w_dae")
            m0 = DAE(C())
            m0.fit()
            ens = DAE_ensemble([m0, E.load_member(C(), str(work / "w_other"))], alphas=alphas)
            lines = []
            for s in splits:
                reader = data_reader_test(data_dir=conf.data_dir, filename=s, batch_size=conf.batch, test_num=conf.testsize)
                ranks = []
                while True:
                    x_positions, test_seed, test_answer, _titles, x_ones = reader.next_batch_test()
                    ranks += ens.rank_of(x_positions, x_ones, [list(a) for a in test_answer], SEEDS_FROM_INPUT, n_rows=len(test_seed))
                    if reader.test_idx == 0:
                        break
                ranks = np.concatenate(ranks)
                lines.append("seed num: %s ensemble ranks: mrr %f median %.1f %s"
                             % (s, met.mean_reciprocal_rank(ranks), met.median_rank(ranks),
                                ' '.join("recall@%d %f" % (k, v) for k, v in zip(main_train.RANK_CUTS, met.recall_at(ranks, main_train.RANK_CUTS)))))
            return ens, lines
        _ens, want = by_hand([0.25, 0.75])
        assert full[4:] == want
        # ensemble_fit: the alphas are fitted on test-5 first, then everything is an ensemble of these alphas
        fitted, said = testmode_lines("ensemble = w_other\nensemble_fit = 5\neval_ensemble_ranks = on")
        m = re.match(r"ensemble: fitted alphas ([0-9.e+-]+), ([0-9.e+-]+) \(mrr ([0-9.]+) on test-5, (\d+) points evaluated\)", said[1])
        assert m and len(said) == 2, said
        alphas = [float(m.group(1)), float(m.group(2))]
        assert abs(sum(alphas) - 1.0) < 1e-6 and int(m.group(4)) == 11
        again, _ = testmode_lines("ensemble = w_other\nensemble_alpha = %r, %r\neval_ensemble_ranks = on" % tuple(alphas))
        assert fitted == again and len(fitted) == 8
        assert fitted[4:] == by_hand(alphas)[1]
        mrr5 = float(fitted[6].split()[fitted[6].split().index("mrr") + 1])
        assert abs(mrr5 - float(m.group(3))) < 1e-6
        # --challenge fits the same alphas (in its own batches of 5) before it ranks the submission
        open(work / "config.ini", "w").write(ini.replace("[BASE]", "[BASE]\nensemble = w_other\nensemble_fit = 5")
                                             .replace("[CHALLENGE]", "[CHALLENGE]\nallow_no_title = True"))
        n0 = len(open(work / "log.txt").read().splitlines())
        assert cli.main(["--dir", "run", "--challenge"]) == 0
        new = open(work / "log.txt").read().splitlines()[n0:]
        assert [l for l in new if l.startswith("ensemble: fitted")] == [said[1]]
        assert new.index(said[1]) < next(i for i, l in enumerate(new) if l.startswith("wrote "))
    finally:
        os.chdir(cwd)
