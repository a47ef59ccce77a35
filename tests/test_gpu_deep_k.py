"""GPU (-m gpu): deep top-k, 1 024 < k <= 4 096 (DAE_MAX_K_DEEP) -- the 8 192-key instantiation of the selection kernel
(csrc/topk.hip) alone, behind the fused scoring path, behind the sharded halves and behind dae_rank_candidates, and the refusals
of the calls that keep k <= 1 024.

Expected values never come from the code under test: rankings are `oracle.topk` (the C oracle orders any k) over logits the
device wrote with dae_decode_dense in the same dtype -- the repository's identity "fused == dense + the same ranking, indices
and scores bit for bit" -- and once in this file the oracle's ranking is itself checked against a numpy lexsort on
(-key, column)."""
import pickle

import numpy as np
import pytest

import oracle
from oracle import title_numpy as tn
from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.models.DAEs import DAE, DAE_title, coo_to_csr, seeds_to_csr
from spotify_recsys_challenge_2018_amd.models.title_models import get_model
from spotify_recsys_challenge_2018_amd.sharding import HipRankStages, prepack_scoring_shard, scoring_shard
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights

pytestmark = pytest.mark.gpu
F32, BF, EXACT = _lib.DAE_DTYPE_F32, _lib.DAE_DTYPE_BF16, _lib.DAE_DTYPE_BF16_EXACT
U32 = np.uint32
K_DEEP = 4096


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _some(a, dtype):
    return a if a.size else np.zeros(1, dtype)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _same(idx, score, want_idx, want_score):
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    return np.array_equal(idx, want_idx) and np.array_equal(score.view(U32), np.asarray(want_score, np.float32).view(U32))


def _okey(z):
    u = np.asarray(z, np.float32).view(U32)
    return np.where(u >> 31, ~u, u | U32(0x80000000)).astype(np.int64)


def _lexsort_rank(z_row, cols, seeds, k):
    """numpy's own ranking of one row: key descending, column ascending, seeds and -inf dropped -> (idx [k], logit [k])."""
    keep = ~np.isin(cols, np.asarray(seeds, np.int64)) & (_okey(z_row) > 0x007FFFFF)
    c, z = cols[keep], z_row[keep]
    order = np.lexsort((c, -_okey(z)))[:k]
    idx = np.full(k, -1, np.int32); lg = np.full(k, -np.inf, np.float32)
    idx[:order.size] = c[order]; lg[:order.size] = z[order]
    return idx, lg


# ---- 1. the selection alone (dae_topk_dense) -----------------------------------------------------------------------------------
B_SEL = 5
_SEL = {}


def _sel_logits(ncols):
    """Five rows, one per kind of logits: normal | 16 distinct values (hundreds of ties straddle any rank: the column decides) |
    all equal | -inf except 1 500 entries | normal.  ld > ncols; the slack holds large values that must never be ranked."""
    if ncols not in _SEL:
        rng = np.random.default_rng(ncols)
        ld = ncols + 37
        z = np.full((B_SEL, ld), 50.0, np.float32)
        z[0, :ncols] = rng.standard_normal(ncols)
        z[1, :ncols] = (np.arange(16, dtype=np.float32) * 0.37 - 2.6)[rng.integers(0, 16, ncols)]
        z[2, :ncols] = 0.25
        z[3, :ncols] = -np.inf
        z[3, rng.permutation(ncols)[:1500]] = rng.standard_normal(1500)
        z[4, :ncols] = rng.standard_normal(ncols) * 3.0
        _SEL[ncols] = dict(z=z, dev=_dev(z), want={})
    return _SEL[ncols]


def _sel_seeds(p, ncols, kind, col_base):
    """-> per-row lists of GLOBAL seed columns, ascending and unique."""
    rng = np.random.default_rng(ncols + 7)
    if kind == "none":
        return None
    out = []
    for r in range(B_SEL):
        if kind == "best300":           # the row's 150 best columns and 150 others
            best = np.argsort(-p["z"][r, :ncols], kind="stable")[:150]
            s = np.union1d(best, rng.permutation(ncols)[:150])
        else:                           # "most": all but 1 000 columns, so that fewer than k remain
            s = np.setdiff1d(np.arange(ncols), rng.permutation(ncols)[:1000])
        out.append((np.unique(s) + col_base).tolist())
    return out


def _sel_want(p, ncols, kind, col_base, out_kind):
    """The oracle's ranking at k = 4 096, computed once per configuration and left unchanged: a shorter list is its prefix."""
    key = (kind, col_base, out_kind)
    if key not in p["want"]:
        seeds = _sel_seeds(p, ncols, kind, col_base)
        srp, sc = seeds_to_csr(seeds, B_SEL, col_base + ncols) if seeds is not None else (None, None)
        s, i = oracle.topk(p["z"], K_DEEP, srp, sc, col_base=col_base, ncols=ncols, out_kind=out_kind)
        p["want"][key] = (seeds, srp, sc, s, i)
    return p["want"][key]


@pytest.mark.parametrize("seed_kind", ["none", "best300", "most"])
@pytest.mark.parametrize("k", [1025, 2048, 4095, 4096])
@pytest.mark.parametrize("ncols", [3000, 4096, 4097, 9001, 70000])
def test_selection_alone(ctx, ncols, k, seed_kind):
    """3 000: fewer columns than k (padding); 4 096: the bound that selects the 256-thread shape for k <= 1 024 -- never for a
    deep row; 70 000: more keys than the LDS cache holds, the source is read again.  Both out_kinds, col_base 0 and 64."""
    import torch
    p = _sel_logits(ncols)
    for col_base in (0, 64):
        for out_kind in (_lib.DAE_OUT_SCORE, _lib.DAE_OUT_LOGIT):
            seeds, srp, sc, ws, wi = _sel_want(p, ncols, seed_kind, col_base, out_kind)
            s = torch.full((B_SEL, k), 7.0, device="cuda"); i = torch.full((B_SEL, k), -7, dtype=torch.int32, device="cuda")
            ctx.topk_dense(p["dev"], ncols, col_base, None if srp is None else _dev(srp), None if sc is None else _dev(_some(sc, np.int32)),
                           k, s, i, out_kind=out_kind)
            assert _same(i, s, wi[:, :k], ws[:, :k]), (ncols, k, seed_kind, col_base, out_kind)
            if seed_kind == "most" or ncols < k:
                assert (wi[:, k - 1] == -1).all()              # the case really pads


def test_oracle_ranking_is_the_lexsort_ranking():
    """Once per file: the reference of every test here against numpy's lexsort on (-key, column)."""
    ncols, col_base = 9001, 64
    p = _sel_logits(ncols)
    seeds, srp, sc, ws, wi = _sel_want(p, ncols, "best300", col_base, _lib.DAE_OUT_LOGIT)
    cols = np.arange(ncols, dtype=np.int64) + col_base
    for r in range(B_SEL):
        idx, lg = _lexsort_rank(p["z"][r, :ncols], cols, seeds[r], K_DEEP)
        assert np.array_equal(idx, wi[r]) and np.array_equal(lg.view(U32), ws[r].view(U32)), r
    assert (wi[3, 1500 - 300:] == -1).any() and (wi[1, :K_DEEP] >= 0).all()


def test_deep_list_extends_the_shallow_one(ctx):
    """The first 1 024 entries of the k = 4 096 list are the k = 1 024 list, which the existing instantiation produces."""
    import torch
    for ncols in (4096, 70000):
        p = _sel_logits(ncols)
        seeds, srp, sc, ws, wi = _sel_want(p, ncols, "best300", 0, _lib.DAE_OUT_SCORE)
        out = {}
        for k in (1024, K_DEEP):
            s = torch.empty((B_SEL, k), device="cuda"); i = torch.empty((B_SEL, k), dtype=torch.int32, device="cuda")
            ctx.topk_dense(p["dev"], ncols, 0, _dev(srp), _dev(sc), k, s, i)
            out[k] = (i, s)
        assert torch.equal(out[K_DEEP][0][:, :1024], out[1024][0]) and torch.equal(out[K_DEEP][1][:, :1024], out[1024][1])


def test_selection_without_the_seed_bitmap(ctx):
    """A ranked range too wide for the LDS seed bitmap next to the 64 KiB sort buffer (> ~600 000 columns): the bitmap-free mode.
    Row 0: k + seeds fit the sort buffer (seeds removed after the collect); row 1: they do not (every element tested)."""
    import torch
    ncols, k = 620000, K_DEEP
    rng = np.random.default_rng(5)
    z = rng.standard_normal((2, ncols)).astype(np.float32)
    best = np.argsort(-z[1])[:4000]
    seeds = [np.unique(np.concatenate([np.argsort(-z[0])[:100], rng.permutation(ncols)[:200]])).tolist(),
             np.unique(np.concatenate([best, rng.permutation(ncols)[:300]])).tolist()]
    assert len(seeds[0]) + k <= 8192 < len(seeds[1]) + k
    srp, sc = seeds_to_csr(seeds, 2, ncols)
    ws, wi = oracle.topk(z, k, srp, sc, ncols=ncols, out_kind=_lib.DAE_OUT_LOGIT)
    s = torch.empty((2, k), device="cuda"); i = torch.empty((2, k), dtype=torch.int32, device="cuda")
    ctx.topk_dense(_dev(z), ncols, 0, _dev(srp), _dev(sc), k, s, i, out_kind=_lib.DAE_OUT_LOGIT)
    assert _same(i, s, wi, ws)


# ---- 2. the fused path ---------------------------------------------------------------------------------------------------------
def _fused_problem(V, nt, B, H, seed):
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=seed, bias="zipf", n_tracks=nt)
    pos, ones, seeds = make_playlists(B, nt, V - nt, seed=seed + 1)
    rng = np.random.default_rng(seed + 2)
    # one row with 250 seeds, the most popular columns (the row's likely winners) among them
    seeds[1 % B] = np.unique(np.concatenate([np.arange(100), rng.permutation(nt)[:150]]))[:250].tolist()
    rp, col, val = coo_to_csr(pos, ones, B, V)
    srp, sc = seeds_to_csr(seeds, B, nt)
    d = dict(rp=_dev(rp), col=_dev(col), val=_dev(val), We=_dev(W_enc), be=_dev(b_enc), Wd=_dev(W_dec), bd=_dev(b_dec),
             srp=_dev(srp), sc=_dev(_some(sc, np.int32)))
    return d, srp, sc


def _fused_lists(c, d, nt, B, k, dtype):
    import torch
    s = torch.full((B, k), 7.0, device="cuda"); i = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
    c.score_topk(d["rp"], d["col"], d["val"], d["We"], d["be"], nt, d["srp"], d["sc"], k, s, i, dtype=dtype)
    return s, i, c.last_plan()


def _dense_logits(c, d, V, B, H, dtype, rows=None):
    """The device's own dense logits of `dtype` (dae_encode + dae_decode_dense), on the host."""
    import torch
    h = torch.empty((B, H), device="cuda")
    c.encode(d["rp"], d["col"], d["val"], d["We"], d["be"], h)
    z = torch.empty((B, V), device="cuda")
    c.decode_dense(h, z, apply_sigmoid=False, dtype=dtype)
    return (z if rows is None else z[torch.as_tensor(rows, device="cuda")]).cpu().numpy()


FUSED = [(33000, 30011, 37, 4096, F32, 256), (33000, 30011, 257, 1025, F32, 256),
         (33000, 6000, 128, 4096, F32, 256),       # the sample holds fewer than k elements: tau must be -inf
         (33000, 3000, 64, 4096, F32, 256),        # fewer tracks than k: padding
         (40037, 39990, 129, 2048, BF, 256), (33000, 20011, 256, 4096, BF, 256),
         (9000, 8000, 40, 4096, F32, 64),          # the generic kernels
         (40000, 33000, 40, 4096, F32, 64),        # ... on the threshold path
         (21000, 20011, 2048, 1025, F32, 256)]     # many short rows: the wave-per-row threshold kernel


@pytest.mark.parametrize("V,nt,B,k,dtype,H", FUSED)
def test_fused_equals_dense_plus_oracle_ranking(V, nt, B, k, dtype, H):
    c = _lib.Context(0)
    try:
        d, srp, sc = _fused_problem(V, nt, B, H, seed=V % 97)
        c.prepack_decoder(d["Wd"], d["bd"], dtype=dtype)
        _s, _i, plan_1024 = _fused_lists(c, d, nt, B, 1024, dtype)        # the plan of the same shape at k = 1 024: k <= 1 024 plans are the parent's
        s, i, plan = _fused_lists(c, d, nt, B, k, dtype)
        print("plan words (V, tracks, B, k, dtype, H) = %s: %s" % ((V, nt, B, k, dtype, H), plan))
        assert plan["fused"] == plan_1024["fused"], (plan, plan_1024)
        z = _dense_logits(c, d, V, B, H, dtype)
        ws, wi = oracle.topk(z, k, srp, sc, ncols=nt)
        assert _same(i, s, wi, ws), plan
        if nt < k:
            assert (wi[:, nt:] == -1).all() and (wi[0, :nt - 300] >= 0).all(), plan
    finally:
        c.close()


def test_fused_full_vocabulary():
    """The shipped shape (|vocab| 170 000, 140 000 tracks, hidden 256, 256 rows) at k = 4 096: 16 sampled rows against the host
    ranking of their dense logits."""
    V, nt, B, k, H = 170000, 140000, 256, 4096, 256
    c = _lib.Context(0)
    try:
        d, srp, sc = _fused_problem(V, nt, B, H, seed=0)
        c.prepack_decoder(d["Wd"], d["bd"], dtype=F32)
        s, i, plan = _fused_lists(c, d, nt, B, k, F32)
        assert plan["fused"] == 1, plan
        rows = np.unique(np.concatenate([[0, 1, 255], np.random.default_rng(1).permutation(B)[:16]]))[:16]
        z = _dense_logits(c, d, V, B, H, F32, rows=rows)
        srp_r = np.concatenate([[0], np.cumsum(np.diff(srp)[rows])]).astype(np.int32)
        sc_r = np.concatenate([sc[srp[r]:srp[r + 1]] for r in rows]).astype(np.int32)
        ws, wi = oracle.topk(z, k, srp_r, sc_r, ncols=nt)
        assert _same(i[_dev(rows)], s[_dev(rows)], wi, ws), plan
    finally:
        c.close()


# ---- 3. the sharded halves -----------------------------------------------------------------------------------------------------
def test_sharded_halves_merge_to_the_unsharded_lists():
    import torch
    V, nt, B, k, H, world = 33000, 30011, 64, 2048, 256, 4
    d, srp, sc = _fused_problem(V, nt, B, H, seed=12)
    feed = (d["rp"], d["col"], d["val"], d["srp"], d["sc"])
    full = _lib.Context(0)
    ctxs, keep = [full], []
    try:
        full.prepack_decoder(d["Wd"], d["bd"], 0, V, dtype=F32)
        s0, i0, _plan = _fused_lists(full, d, nt, B, k, F32)
        stages = []
        for g in range(world):
            c = _lib.Context(0)
            ctxs.append(c)
            bound, rows = prepack_scoring_shard(c, d["Wd"], d["bd"], scoring_shard(nt, V, world, g), F32)
            keep.append(rows)
            stages.append(HipRankStages(c, d["We"], d["be"], bound, F32))
        taus = torch.stack([st.local_begin(feed, k).clone() for st in stages])
        tau_max = taus.amax(0)
        lists = [tuple(t.clone() for t in st.local_finish(feed, k, tau_max)) for st in stages]
        gl, gi = torch.stack([a for a, _ in lists]), torch.stack([b for _, b in lists])
        s, i = stages[0].merge(gl, gi)
        assert torch.equal(i, i0) and torch.equal(s.view(torch.int32), s0.view(torch.int32))
        z = _dense_logits(full, d, V, B, H, F32)                          # ... and those are the oracle's
        ws, wi = oracle.topk(z, k, srp, sc, ncols=nt)
        assert _same(i0, s0, wi, ws)
    finally:
        for c in ctxs:
            c.close()


# ---- 4. dae_rank_candidates ----------------------------------------------------------------------------------------------------
def test_rank_candidates_deep(ctx):
    import torch
    V, B, k, cap = 20000, 4, 2048, 6000
    rng = np.random.default_rng(3)
    lens = [6000, 2500, 1500, 0]                                          # rows above and below k
    cands = [np.sort(rng.permutation(V)[:n]).astype(np.int32) for n in lens]
    keys = [(rng.integers(-40, 40, n) * 0.125).astype(np.float32) for n in lens]      # 80 distinct values: the column decides
    seeds = [np.unique(np.concatenate([c[np.argsort(-z)[:100]], rng.permutation(V)[:200]])).tolist() if c.size else []
             for c, z in zip(cands, keys)]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    srp, sc = seeds_to_csr(seeds, B, V)
    s = torch.full((B, k), 7.0, device="cuda"); i = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
    ctx.rank_candidates(V, (_dev(rp), _dev(np.concatenate(cands))), _dev(np.concatenate(keys)), cap, _dev(srp), _dev(sc), k, s, i,
                        out_kind=_lib.DAE_OUT_LOGIT)
    want = [_lexsort_rank(z, c.astype(np.int64), sd, k) for c, z, sd in zip(cands, keys, seeds)]
    assert _same(i, s, np.stack([w[0] for w in want]), np.stack([w[1] for w in want]))
    assert want[0][0][-1] >= 0 and want[2][0][-1] == -1


# ---- 5. refusals: nothing written ----------------------------------------------------------------------------------------------
def _refused(call, match, *outs):
    with pytest.raises(_lib.DaeError, match=match):
        call()
    import torch
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 7).all()), "a refused call wrote to its output"


def test_refusals_write_nothing(ctx):
    import torch
    V, nt, B, H = 3000, 2500, 4, 64
    d, srp, sc = _fused_problem(V, nt, B, H, seed=4)
    ctx.prepack_decoder(d["Wd"], d["bd"], dtype=F32)
    h = torch.rand((B, H), device="cuda")
    z = torch.rand((B, V), device="cuda")

    def outs(k):
        return torch.full((B, k), 7.0, device="cuda"), torch.full((B, k), 7, dtype=torch.int32, device="cuda")
    # k = 4 097 on each call that takes deep lists
    s, i = outs(4097)
    deep = r"k=4097 out of \[1,4096\]"
    _refused(lambda: ctx.topk_dense(z, nt, 0, d["srp"], d["sc"], 4097, s, i), deep, s, i)
    _refused(lambda: ctx.decode_topk(h, nt, d["srp"], d["sc"], 4097, s, i), deep, s, i)
    _refused(lambda: ctx.score_topk(d["rp"], d["col"], d["val"], d["We"], d["be"], nt, d["srp"], d["sc"], 4097, s, i), deep, s, i)
    _refused(lambda: ctx.score_topk(d["rp"], d["col"], d["val"], d["We"], d["be"], nt, d["srp"], d["sc"], 4097, s, i, dtype=BF), deep, s, i)
    tau = torch.full((B,), 7.0, device="cuda")
    _refused(lambda: ctx.score_topk_begin(d["rp"], d["col"], d["val"], d["We"], d["be"], nt, d["srp"], 4097, tau), deep, tau)
    gl = torch.rand((2, B, 4097), device="cuda"); gi = torch.zeros((2, B, 4097), dtype=torch.int32, device="cuda")
    _refused(lambda: ctx.topk_merge(gl, gi, s, i), deep, s, i)
    cand = (_dev(np.arange(B + 1, dtype=np.int32) * 10), _dev(np.arange(B * 10, dtype=np.int32)))
    _refused(lambda: ctx.rank_candidates(V, cand, torch.rand(B * 10, device="cuda"), 10, d["srp"], d["sc"], 4097, s, i), deep, s, i)
    # k = 1 025 where 1 024 stays the limit
    s, i = outs(1025)
    kept = r"k=1025 out of \[1,1024\]"
    _refused(lambda: ctx.decode_topk(h, nt, d["srp"], d["sc"], 1025, s, i, dtype=EXACT), kept, s, i)
    _refused(lambda: ctx.score_topk(d["rp"], d["col"], d["val"], d["We"], d["be"], nt, d["srp"], d["sc"], 1025, s, i, dtype=EXACT), kept, s, i)
    _refused(lambda: ctx.score_topk_begin(d["rp"], d["col"], d["val"], d["We"], d["be"], nt, d["srp"], 1025, tau, dtype=EXACT), kept, tau)
    mixT = torch.zeros((nt, B), device="cuda"); w = torch.ones(B, device="cuda")
    ctx.set_score_mix(mixT, w)
    try:
        _refused(lambda: ctx.decode_topk(h, nt, d["srp"], d["sc"], 1025, s, i), kept, s, i)
    finally:
        ctx.set_score_mix()
    rec = torch.full((B, 24), 7, dtype=torch.uint8, device="cuda")
    ans = (_dev(np.arange(B + 1, dtype=np.int32)), _dev(np.arange(B, dtype=np.int32)))
    _refused(lambda: ctx.rank_metrics(torch.zeros((B, 1025), dtype=torch.int32, device="cuda"), 1025, ans[0], ans[1], out=rec),
             kept, rec)
    with pytest.raises(_lib.DaeError, match=r"k out of \[1,1024\]"):
        _lib.Pipeline(d["We"], d["be"], d["Wd"], d["bd"], nt, k=1025)
    # ... and the limits themselves are taken
    s, i = outs(4096)
    ctx.score_topk(d["rp"], d["col"], d["val"], d["We"], d["be"], nt, d["srp"], d["sc"], 4096, s, i)
    assert int(i[0, 0]) >= 0 and int(i[0, -1]) == -1                      # 2 500 tracks: the tail is padding


# ---- 6. Python -----------------------------------------------------------------------------------------------------------------
PV, PNT, PH, PB = 6000, 5000, 64, 6


@pytest.fixture(scope="module")
def py_problem():
    W_enc, b_enc, W_dec, b_dec = make_weights(PV, PH, seed=21, bias="zipf", n_tracks=PNT)
    pos, ones, seeds = make_playlists(PB, PNT, PV - PNT, seed=22)
    return dict(W_enc=W_enc, b_enc=b_enc, W_dec=W_dec, b_dec=b_dec, pos=pos, ones=ones, seeds=seeds)


def _model(p, decode_dtype="f32"):
    class C:
        save = "/tmp/_deepk_unused"; n_input = PV; lr = 0.01; reg_lambda = 0.0; initval = "NULL"
        batch = PB; hidden = PH; n_tracks = PNT
    C.decode_dtype = decode_dtype
    m = DAE(C())
    m._host_init = lambda: [p["W_enc"], p["W_dec"], p["b_enc"], p["b_dec"]]
    m.fit()
    return m


@pytest.mark.parametrize("name,dtype", [("f32", F32), ("bf16", BF)])
def test_recommend_deep(py_problem, name, dtype):
    import torch
    p = py_problem
    m = _model(p)
    idx, score = m.recommend(p["pos"], p["ones"], p["seeds"], k=3000, dtype=name)
    m._ensure_packed(dtype)
    h = m.encode(p["pos"], p["ones"])
    z = torch.empty((PB, PV), device="cuda")
    m.ctx.decode_dense(h, z, apply_sigmoid=False, dtype=dtype)
    srp, sc = seeds_to_csr(p["seeds"], PB, PNT)
    ws, wi = oracle.topk(z.cpu().numpy(), 3000, srp, sc, ncols=PNT)
    assert np.array_equal(idx, wi) and np.array_equal(score.view(U32), ws.view(U32))
    idx500, score500 = m.recommend(p["pos"], p["ones"], p["seeds"], k=500, dtype=name)
    assert np.array_equal(idx[:, :500], idx500) and np.array_equal(score[:, :500].view(U32), score500.view(U32))


def test_recommend_exact_mode_deep_runs_fp32_and_says_so_once(py_problem, capfd):
    p = py_problem
    m = _model(p)
    want = m.recommend(p["pos"], p["ones"], p["seeds"], k=3000, dtype="f32")
    capfd.readouterr()
    got = m.recommend(p["pos"], p["ones"], p["seeds"], k=3000, dtype="exact_bf16")
    err = capfd.readouterr().err
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(U32), want[1].view(U32))
    assert err.count("\n") == 1 and "exact_bf16" in err and "1024" in err and "fp32" in err
    m.recommend(p["pos"], p["ones"], p["seeds"], k=2000, dtype="exact_bf16")
    assert capfd.readouterr().err == ""                                   # once


def test_streamed_calls_refuse_deep_k(py_problem):
    p = py_problem
    m = _model(p)
    feeds = [(p["pos"], p["ones"], p["seeds"], PB)]
    with pytest.raises(ValueError, match="1024"):
        m.recommend_iter(feeds, k=2000)
    with pytest.raises(ValueError, match="1024"):
        m.evaluate_iter([(feeds[0], [[1]] * PB)], k=2000)
    assert not m._pipes                                                   # no pipeline was created


def test_titled_recommend_refuses_deep_k_before_any_launch(tmp_path):
    N_CHAR, E, fs, F, L = 41, 25, [3, 5], 40, 25

    class Conf:
        lr = 0.01; reg_lambda = 0.0; charsize = N_CHAR; char_model = 'Char_CNN'; save = "/tmp/_deepk_unused"
        initval = "NULL"; title_lr = 0.002; batch = 8; n_input = 3000; n_output = 3000; n_tracks = 2500; hidden = 64
    c = Conf()
    c.char_emb, c.filter_size, c.filter_num, c.strmaxlen = E, list(fs), F, L
    W_enc, b_enc, W_dec, b_dec = make_weights(c.n_input, c.hidden, seed=1, bias="zipf", n_tracks=c.n_tracks)
    pk = tmp_path / "w_dae"
    with open(pk, "wb") as f:
        pickle.dump([W_enc, W_dec, b_enc, b_dec], f)
    c.DAEval = str(pk)
    mt = get_model(c)
    mt.fit(tn.make_params(N_CHAR, E, fs, F, c.n_output, seed=4))
    m = DAE_title(c, mt)
    m.fit()
    pos, ones, seeds = make_playlists(c.batch, c.n_tracks, c.n_input - c.n_tracks, seed=5)
    titles = np.random.default_rng(6).integers(0, N_CHAR, (c.batch, L))
    before = m.ctx.lib.dae_scratch_bytes(m.ctx.h)
    with pytest.raises(ValueError, match="1024"):
        m.recommend(pos, ones, seeds, k=2000, titles=titles, titles_use=np.ones(c.batch, np.float32))
    assert m.ctx.lib.dae_scratch_bytes(m.ctx.h) == before and m._csr_status is None      # nothing uploaded, nothing reserved
    # without titles in use: the plain path, which takes the deep k
    idx, score = m.recommend(pos, ones, seeds, k=2000, titles=titles, titles_use=np.zeros(c.batch, np.float32))
    want = DAE.recommend(m, pos, ones, seeds, k=2000)
    assert np.array_equal(idx, want[0]) and np.array_equal(score.view(U32), want[1].view(U32))
