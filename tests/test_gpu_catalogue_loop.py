"""GPU (-m gpu): the streamed loops inside a catalogue -- `recommend_iter` / `evaluate_iter(..., catalogue=handle)` on a pipeline in
catalogue mode (include/dae_hip.h dae_pipeline_set_catalogue; csrc/pipeline.hip, csrc/pipeline_issue.hip,
csrc/catalogue.hip) and
`rank_candidates(..., catalogue=handle)`.

The expected lists of a feed are `model.recommend(feed, catalogue=handle)` of that feed ALONE -- the call tests/test_gpu_catalogue.py
pins to the oracle -- and, for one catalogue, also the independent route of that file: `oracle.topk` over the device's dense logits
of the FULL image with the row's seeds united with the catalogue's complement (tests/test_catalogue_cpu.py `reference`).  Every
comparison is bit for bit: indices, and score bits as uint32.

The model: |vocab| 33 000, 30 011 tracks, hidden 256, zipf bias, batch 32, k = 100.  A launch of the loop holds 8 feeds = 256 rows
(`_coalesce_count`), the pipeline has 3 lanes and 8 launch slots: 133 feeds run every slot at least twice.
WHICH PLAN RUNS.  At the model's 32 rows a ranking call has 1 024 SIMD slots, more than the 938 tiles of the whole track range: no
catalogue of this vocabulary takes the threshold path there in fp32 / bf16 (score_plan.h: `fused` needs more tiles than one round of
slots); the exact mode always does, and the case asserts that for the per-batch call of the 3 000-column catalogue.  The launches
of the LOOP hold 256 rows = 512 slots: the smallest catalogue whose fp32 / bf16 launches take the threshold path (sample, tau,
filter) has 513 tiles -- `big`, 16 400 columns -- and the case asserts `fused == 1` for a ranking call of 256 rows on that image."""
import pickle
import warnings

import numpy as np
import pytest

from oracle import title_numpy as tn
from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.models.DAEs import DAE, DAE_title, SEEDS_FROM_INPUT, coo_to_csr, seeds_to_csr
from spotify_recsys_challenge_2018_amd.models.title_models import get_model
from spotify_recsys_challenge_2018_amd.utils import metrics as met
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights
from test_catalogue_cpu import random_catalogue, reference
from test_metrics_cpu import reference as metrics_reference

pytestmark = pytest.mark.gpu
F32, BF, EXACT = _lib.DAE_DTYPE_F32, _lib.DAE_DTYPE_BF16, _lib.DAE_DTYPE_BF16_EXACT
U32 = np.uint32
V, NT, H, B, K = 33000, 30011, 256, 32, 100
N_BASE = 10                                   # distinct feeds; the loops cycle over them
ROWS_HEAD = [32, 7, 32, 1]                    # the first launch coalesces feeds of these sizes


def _eq(got, want):
    return (got[0].shape == want[0].shape and np.array_equal(got[0], want[0])
            and np.array_equal(np.asarray(got[1], np.float32).view(U32), np.asarray(want[1], np.float32).view(U32)))


def _model(tmp_path, scale=1.0, seed=31):
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=seed, bias="zipf", n_tracks=NT)
    W_dec = (W_dec * scale).astype(np.float32)
    path = str(tmp_path / ("init_%s.pkl" % scale))
    with open(path, "wb") as f:
        pickle.dump([W_enc, W_dec, b_enc, b_dec], f)

    class C:
        save = str(tmp_path / "unused"); batch = B; n_input = V; hidden = H; lr = 0.005; reg_lambda = 0.0
        n_tracks = NT; initval = path
    m = DAE(C()); m.fit()
    return m


CATS = {"a3000": random_catalogue(NT, 3000, seed=3), "small40": random_catalogue(NT, 40, seed=40),
        "all": np.arange(NT, dtype=np.int32), "big": random_catalogue(NT, 16400, seed=16)}


def _base_feeds():
    """N_BASE feeds of 32 rows.  Feed 0 carries the rows a catalogue loop must get right (the seeds are the row's own tracks):
    row 0 only tracks OUTSIDE every random catalogue, row 1 only tracks inside `a3000`, row 2 empty, row 3 only tracks inside
    `small40` (10 of its 40 columns: 30 rankable, fewer than k), row 4 only tracks inside `big`."""
    feeds = [list(make_playlists(B, NT, V - NT, seed=100 + s)) for s in range(N_BASE)]
    pos, ones, _ = feeds[0]
    outside = np.setdiff1d(np.arange(NT), np.concatenate([CATS["a3000"], CATS["small40"], CATS["big"]]))
    special = {0: outside[:20], 1: CATS["a3000"][:15], 2: np.zeros(0, np.int64), 3: CATS["small40"][:10], 4: CATS["big"][5:30]}
    keep = ~np.isin(pos[:, 0], list(special))
    add = np.concatenate([np.stack([np.full(len(c), r, np.int64), np.asarray(c, np.int64)], 1) for r, c in special.items()])
    feeds[0][0] = np.concatenate([add, pos[keep]])
    feeds[0][1] = np.concatenate([np.ones(len(add), np.float32), ones[keep]])
    feeds[0][2] = [sorted(set(int(c) for c in special[r])) if r in special else s for r, s in enumerate(feeds[0][2])]
    return feeds


BASE = _base_feeds()


def _stream():
    """-> [(base feed number, explicit seed lists?, n_rows)]: the head launch, the explicit feed (the per-batch route in the middle
    of the stream), then 128 feeds = 16 full launches: every one of the 8 slots twice, every lane five times."""
    seq = [(i, False, n) for i, n in enumerate(ROWS_HEAD)] + [(4, True, 32)]
    seq += [((5 + j) % N_BASE, False, [32, 32, 19, 32][j % 4]) for j in range(128)]
    return seq


def _feed(i, explicit, n):
    pos, ones, seeds = BASE[i]
    return (pos, ones, seeds if explicit else SEEDS_FROM_INPUT, n)


def _want(m, dtype, h):
    """The expected lists of every distinct feed: `recommend` of the feed alone (all 32 rows; a shorter feed is its first rows)."""
    kw = {} if h is None else {"catalogue": h}
    want = {(i, False): m.recommend(BASE[i][0], BASE[i][1], SEEDS_FROM_INPUT, k=K, dtype=dtype, **kw) for i in range(N_BASE)}
    want[(4, True)] = m.recommend(BASE[4][0], BASE[4][1], BASE[4][2], k=K, dtype=dtype, **kw)
    return want


def _check_loop(got, want, seq, scores=True):
    assert len(got) == len(seq)
    for (gi, gs), (i, ex, n) in zip(got, seq):
        wi, ws = want[(i, ex)]
        assert gi.shape == (n, K) and np.array_equal(gi, wi[:n]), (i, ex, n)
        if scores:
            assert np.array_equal(gs.view(U32), ws[:n].view(U32)), (i, ex, n)
        else:
            assert gs is None


def _own_seeds(pos):
    P = np.asarray(pos, np.int64).reshape(-1, 2)
    return [sorted(set(P[(P[:, 0] == r) & (P[:, 1] < NT), 1].tolist())) for r in range(B)]


def _oracle_lists(m, pos, ones, cols, dtype):
    """The independent route: dense logits of the model's FULL image, seeds u complement of the catalogue, oracle.topk."""
    import torch
    dt = BF if dtype == BF else F32
    m._ensure_packed(dt)
    hid = m.encode(pos, ones)
    z = torch.empty((B, V), device="cuda")
    m.ctx.decode_dense(hid, z, apply_sigmoid=False, dtype=dt)
    srp, sc = seeds_to_csr(_own_seeds(pos), B, NT)
    ws, wi = reference(z.cpu().numpy(), K, srp, sc, cols, NT)
    return wi, ws


def _plan_at_launch_rows(m, h, dtype):
    """last_plan of a ranking call of 256 rows (a launch of the loop: 8 feeds) on the handle's image."""
    import torch
    rows = 8 * B
    pos = np.concatenate([BASE[i][0] + np.array([[i * B, 0]]) for i in range(8)])
    ones = np.concatenate([BASE[i][1] for i in range(8)])
    rp, col, val = coo_to_csr(pos, ones, rows, V)
    srp, sc = seeds_to_csr([s for i in range(8) for s in _own_seeds(BASE[i][0])], rows, NT)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rp, col, val, srp, sc)]
    s = torch.empty((rows, K), device="cuda"); i = torch.empty((rows, K), dtype=torch.int32, device="cuda")
    h._ensure(dtype)
    h.ctx.bind_stream()
    h.ctx.score_topk_catalogue(h.cat, d[0], d[1], d[2], m.weights["encoder_h"], m.biases["encoder_b"], d[3], d[4], K, s, i, dtype=dtype)
    torch.cuda.synchronize()
    return h.ctx.last_plan(), i.cpu().numpy()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    m = _model(tmp_path_factory.mktemp("catloop"))
    yield m
    m.close_pipelines()


# ---- recommend_iter(catalogue=) -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,name", [(F32, "f32"), (BF, "bf16"), (EXACT, "exact_bf16")])
@pytest.mark.parametrize("cat", ["a3000", "small40", "all", "big"])
def test_recommend_iter_in_a_catalogue_gives_the_per_feed_lists(model, cat, dtype, name):
    m, cols, seq = model, CATS[cat], _stream()
    h = m.catalogue(cols)
    try:
        want = _want(m, name, h)
        plan = h.ctx.last_plan()
        print("plan of the per-batch call (%s, n = %d, 32 rows, %s): %s" % (cat, len(cols), name, plan))
        assert plan["n_tiles"] == (len(cols) + 31) // 32
        if cat == "a3000" and dtype == EXACT:
            assert plan["fused"] == 1, plan                   # the exact mode's threshold path at the model's own batch
        if cat == "big":
            plan256, i256 = _plan_at_launch_rows(m, h, dtype)
            print("plan at a launch's 256 rows (big, n = %d, %s): %s" % (len(cols), name, plan256))
            assert plan256["fused"] == 1 and plan256["n_tiles"] == 513, plan256
            assert np.array_equal(i256[:B], want[(0, False)][0])      # ... and it ranks what the 32-row call ranks
        if dtype == EXACT:                                    # the fp32 lists, bit for bit
            w32 = _want(m, "f32", h)
            assert all(_eq(want[key], w32[key]) for key in want)
        if cat in ("a3000", "big") and dtype != EXACT:        # the independent route, on the feed with the special rows
            assert _eq(want[(0, False)], _oracle_lists(m, BASE[0][0], BASE[0][1], cols, dtype))
        wi, ws = want[(0, False)]
        assert (wi[2] >= 0).sum() == min(K, len(cols))        # the empty row: the catalogue's best
        if cat != "all":
            assert np.isin(wi[wi >= 0], cols).all()
        if cat == "a3000":
            assert (wi[1] >= 0).all() and not np.isin(wi[1], CATS["a3000"][:15]).any()
        if cat == "small40":                                  # fewer columns than k: -1 stays -1 through the map-back, -inf beside it
            assert (wi[:, 40:] == -1).all() and np.isneginf(ws[:, 40:]).all()
            assert (wi[3] >= 0).sum() == 30 and (wi[0] >= 0).sum() == 40
        feeds = [_feed(*x) for x in seq]
        for scores in (True, False):
            got = [(gi.copy(), None if gs is None else gs.copy())
                   for gi, gs in m.recommend_iter(feeds, k=K, dtype=name, want_scores=scores, catalogue=h)]
            _check_loop(got, want, seq, scores)
        pipes = [p for key, (_g, p) in m._pipes.items() if key[-1] == ("catalogue", id(h))]
        assert len(pipes) == 1 and pipes[0] in h._pipes
        st = pipes[0].stats()
        assert st["feeds"] == len(seq) - 1 and st["launches"] == 17 and st["guard_fallbacks"] == 0      # 1 + 16: feeds were coalesced
        if cat == "all":                                      # every track: the loop without a catalogue
            plain = [(gi.copy(), gs.copy()) for gi, gs in m.recommend_iter(feeds[:12], k=K, dtype=name)]
            _check_loop(plain, want, seq[:12])
    finally:
        h.close()


def test_the_guard_fires_inside_the_loop_and_the_rerun_ranks_the_catalogue(tmp_path):
    """A forged bound (dae_set_exact_margin < 1, as tests/test_gpu_exact.py forges it: decoder x 40) makes the guard fire inside
    the catalogue loop; what comes out are the fp32 CATALOGUE lists, so the re-run used the catalogue's fp32 image."""
    m = _model(tmp_path, scale=40.0)
    h = m.catalogue(CATS["a3000"])
    try:
        seq = _stream()[:40]
        feeds = [_feed(*x) for x in seq]
        want = _want(m, "f32", h)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = [(gi.copy(), gs.copy()) for gi, gs in m.recommend_iter(feeds, k=K, dtype="exact_bf16", catalogue=h)]
        _check_loop(got, want, seq)
        assert m.__dict__.get("_guard_fallbacks", 0) == 0
        m.ctx.set_exact_margin(1e-3)
        m._mark_dirty()
        with pytest.warns(UserWarning, match="bound guard"):
            got = [(gi.copy(), gs.copy()) for gi, gs in m.recommend_iter(feeds, k=K, dtype="exact_bf16", catalogue=h)]
        assert m._guard_fallbacks >= 1
        pipe = next(p for key, (_g, p) in m._pipes.items() if key[-1] == ("catalogue", id(h)))
        assert pipe.stats()["guard_fallbacks"] >= 1
        _check_loop(got, want, seq)
        full = m.recommend(BASE[0][0], BASE[0][1], SEEDS_FROM_INPUT, k=K, dtype="f32")
        assert not np.array_equal(full[0], want[(0, False)][0])       # (the full image's fp32 lists are other lists)
    finally:
        m.ctx.set_exact_margin(1.0)
        h.close()
        m.close_pipelines()


def test_loops_alternate_and_the_models_images_are_never_repacked(model):
    m = model
    ha, hb = m.catalogue(CATS["a3000"]), m.catalogue(CATS["big"])
    try:
        seq = _stream()[:20]
        feeds = [_feed(*x) for x in seq]
        w_full, w_a, w_b = _want(m, "bf16", None), _want(m, "bf16", ha), _want(m, "bf16", hb)
        assert not np.array_equal(w_a[(0, False)][0], w_b[(0, False)][0])
        packs = []
        real = m.ctx.prepack_decoder
        m.ctx.prepack_decoder = lambda *a, **kw: (packs.append(1), real(*a, **kw))[1]
        gen, dirty, pa, pb = m._weights_gen, dict(m._packed_dirty), dict(ha._packed), dict(hb._packed)
        try:
            for _ in range(2):
                for h, want in ((None, w_full), (ha, w_a), (hb, w_b), (ha, w_a)):
                    kw = {} if h is None else {"catalogue": h}
                    got = [(gi.copy(), gs.copy()) for gi, gs in m.recommend_iter(feeds, k=K, dtype="bf16", **kw)]
                    _check_loop(got, want, seq)
                assert _eq(m.recommend(BASE[1][0], BASE[1][1], SEEDS_FROM_INPUT, k=K, dtype="bf16"), w_full[(1, False)])
        finally:
            del m.ctx.prepack_decoder
        assert not packs and m._weights_gen == gen and m._packed_dirty == dirty and ha._packed == pa and hb._packed == pb
        assert len(m._pipes) == 1                             # one pipeline at a time per model
    finally:
        ha.close(); hb.close()


def test_a_weight_change_reaches_the_next_catalogue_loop(tmp_path):
    m = _model(tmp_path)
    h = m.catalogue(CATS["a3000"])
    try:
        seq = _stream()[:12]
        feeds = [_feed(*x) for x in seq]
        w0 = _want(m, "f32", h)
        _check_loop([(gi.copy(), gs.copy()) for gi, gs in m.recommend_iter(feeds, k=K, dtype="f32", catalogue=h)], w0, seq)
        m.weights["decoder_h"].mul_(-1.0)
        m.biases["decoder_b"].add_(0.25)
        m._mark_dirty()
        w1 = _want(m, "f32", h)
        assert not np.array_equal(w1[(0, False)][0], w0[(0, False)][0])
        assert _eq(w1[(0, False)], _oracle_lists(m, BASE[0][0], BASE[0][1], CATS["a3000"], F32))
        _check_loop([(gi.copy(), gs.copy()) for gi, gs in m.recommend_iter(feeds, k=K, dtype="f32", catalogue=h)], w1, seq)
    finally:
        h.close()
        m.close_pipelines()


def test_closing_the_handle_closes_its_pipelines(model):
    import gc
    m = model
    h = m.catalogue(CATS["a3000"])
    feeds = [_feed(*x) for x in _stream()[:6]]
    got = [gi.copy() for gi, _s in m.recommend_iter(feeds, k=K, dtype="bf16", want_scores=False, catalogue=h)]
    assert len(got) == 6
    gc.collect()
    key, pipe = next((key, p) for key, (_g, p) in m._pipes.items() if key[-1] == ("catalogue", id(h)))
    assert pipe.h is not None
    h.close()
    assert pipe.h is None and key not in m._pipes and h.cat is None
    with pytest.raises(ValueError, match="closed"):
        list(m.recommend_iter(feeds, k=K, dtype="bf16", catalogue=h))
    with pytest.raises(ValueError, match="closed"):
        list(m.evaluate_iter([(feeds[0], [[1]] * 32)], k=K, dtype="bf16", catalogue=h))
    with pytest.raises(ValueError, match="handle"):
        list(m.recommend_iter(feeds, k=K, catalogue=CATS["a3000"]))
    # the model is as usable as before
    assert len(list(m.recommend_iter(feeds, k=K, dtype="bf16"))) == 6


# ---- _lib.Pipeline.set_catalogue -----------------------------------------------------------------------------------------------------
def test_set_catalogue_refusals_leave_the_pipeline_usable(model, tmp_path):
    import torch
    m = model
    args = (m.weights["encoder_h"], m.biases["encoder_b"], m.weights["decoder_h"], m.biases["decoder_b"], NT)
    ctx = _lib.Context(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cat = _lib.Catalogue(ctx, dev(CATS["a3000"]), NT)
    other = _lib.Catalogue(ctx, dev(CATS["a3000"][:500]), NT - 11)            # built for another n_tracks
    pos, ones, _ = BASE[0]
    want_full = m.recommend(pos, ones, SEEDS_FROM_INPUT, k=K, dtype="f32")
    h = m.catalogue(CATS["a3000"])
    want_cat = m.recommend(pos, ones, SEEDS_FROM_INPUT, k=K, dtype="f32", catalogue=h)
    h.close()
    pipe = _lib.Pipeline(*args, dtype=F32, k=K, group_rows=64, max_nnz=1 << 16, lanes=2)
    assert hasattr(pipe, "set_catalogue")
    try:
        with pytest.raises(_lib.DaeError, match="n_tracks"):
            pipe.set_catalogue(other)
        assert pipe.submit(pos, ones, B)
        pipe.flush()
        assert _eq(pipe.poll(True, copy=True), want_full)
        with pytest.raises(_lib.DaeError, match="before the first submit"):
            pipe.set_catalogue(cat)
        assert pipe.submit(pos, ones, B)                      # still a pipeline over the whole track range
        pipe.flush()
        assert _eq(pipe.poll(True, copy=True), want_full)
    finally:
        pipe.close()
    pipe = _lib.Pipeline(*args, dtype=F32, k=K, group_rows=64, max_nnz=1 << 16, lanes=2)
    try:
        pipe.set_catalogue(cat)
        with pytest.raises(_lib.DaeError, match="before the first submit"):   # once
            pipe.set_catalogue(cat)
        assert pipe.submit(pos, ones, B)
        pipe.flush()
        assert _eq(pipe.poll(True, copy=True), want_cat)
    finally:
        pipe.close()
    # a titled pipeline of the exact mode
    tm_model = _title_model(tmp_path, hidden=128)[0]
    scorer = tm_model._title_scorer()
    tcat = _lib.Catalogue(ctx, dev(random_catalogue(2500, 700, seed=1)), 2500)
    targs = (tm_model.weights["encoder_h"], tm_model.biases["encoder_b"], tm_model.weights["decoder_h"], tm_model.biases["decoder_b"], 2500)
    pipe = _lib.Pipeline(*targs, dtype=EXACT, k=K, group_rows=16, max_nnz=1 << 14, lanes=2, title=scorer)
    try:
        with pytest.raises(_lib.DaeError, match="DAE_DTYPE_BF16_EXACT"):
            pipe.set_catalogue(tcat)
        tpos, tones, _ = make_playlists(8, 2500, 500, seed=5)
        assert pipe.submit(tpos, tones, 8)                    # usable: a plain feed over the whole track range
        pipe.flush()
        gi, _gs = pipe.poll(True, copy=True)
        assert np.array_equal(gi, tm_model.recommend(tpos, tones, SEEDS_FROM_INPUT, k=K, dtype="f32")[0])
    finally:
        pipe.close()
        tcat.close(); other.close(); cat.close(); ctx.close()


# ---- titled ------------------------------------------------------------------------------------------------------------------------
N_CHAR, T_E, T_FS, T_F, T_L = 41, 25, [3, 5], 40, 25
TB, TNT, TV = 8, 2500, 3000


def _title_model(tmp_path, hidden=64):
    class Conf:
        lr = 0.01; reg_lambda = 0.0; charsize = N_CHAR; char_model = 'Char_CNN'; save = "/tmp/_catalogue_loop_unused"
        initval = "NULL"; title_lr = 0.002; batch = TB; n_input = TV; n_output = TV; n_tracks = TNT
    c = Conf()
    c.hidden = hidden
    c.char_emb, c.filter_size, c.filter_num, c.strmaxlen = T_E, list(T_FS), T_F, T_L
    W_enc, b_enc, W_dec, b_dec = make_weights(c.n_input, c.hidden, seed=1, bias="zipf", n_tracks=c.n_tracks)
    pk = tmp_path / ("w_dae_%d" % hidden)
    with open(pk, "wb") as f:
        pickle.dump([W_enc, W_dec, b_enc, b_dec], f)
    c.DAEval = str(pk)
    mt = get_model(c)
    mt.fit(tn.make_params(N_CHAR, T_E, T_FS, T_F, c.n_output, seed=4))
    m = DAE_title(c, mt)
    m.fit()
    return m, c


def _titled_feeds(n=13):
    """Titled feeds of 8 rows; titles_use mixes 0 and 1 inside a feed, feed 3 uses no title at all (a plain launch of the titled
    pipeline), feed 5 carries explicit seed lists (the per-batch route)."""
    rng = np.random.default_rng(8)
    feeds = []
    for i in range(n):
        pos, ones, seeds = make_playlists(TB, TNT, TV - TNT, seed=60 + i)
        titles = rng.integers(0, N_CHAR, (TB, T_L))
        use = (np.arange(TB) % 3 != i % 3).astype(np.float32)
        if i == 3:
            use[:] = 0.0
        feeds.append((pos, ones, [list(s) for s in seeds] if i == 5 else SEEDS_FROM_INPUT, [TB, 3, TB, TB, 1][i % 5], titles, use))
    return feeds


def _titled_want(m, feeds, dtype, h):
    return [m.recommend(p, o, s, k=K, n_rows=n, dtype=dtype, titles=t, titles_use=u, catalogue=h) for p, o, s, n, t, u in feeds]


def test_titled_recommend_iter_in_a_catalogue(tmp_path, capfd):
    m, c = _title_model(tmp_path)
    cols = random_catalogue(TNT, 700, seed=700)
    feeds = _titled_feeds()
    h = m.catalogue(cols)
    try:
        w32 = _titled_want(m, feeds, "f32", h)
        for name in ("f32", "bf16"):
            want = w32 if name == "f32" else _titled_want(m, feeds, name, h)
            got = [(gi.copy(), gs.copy()) for gi, gs in m.recommend_iter(feeds, k=K, dtype=name, catalogue=h)]
            assert len(got) == len(feeds) and all(_eq(g, w) for g, w in zip(got, want))
            assert all(np.isin(g[0][g[0] >= 0], cols).all() for g in got)
        assert not _eq(w32[0], m.recommend(*feeds[0][:3], k=K, n_rows=TB, dtype="f32", titles=feeds[0][4], titles_use=feeds[0][5]))
        capfd.readouterr()
        for _ in range(2):                                    # the exact mode: the fp32 lists, said once
            got = [(gi.copy(), gs.copy()) for gi, gs in m.recommend_iter(feeds, k=K, dtype="exact_bf16", catalogue=h)]
            assert all(_eq(g, w) for g, w in zip(got, w32))
        err = capfd.readouterr().err
        assert err.count("\n") == 1 and "exact_bf16" in err and "catalogue" in err and "fp32" in err
    finally:
        h.close()
        m.close_pipelines()


# ---- evaluate_iter(catalogue=) --------------------------------------------------------------------------------------------------------
def _answers(rng, idx, cols, n_tracks):
    """Answer lists for the rows of `idx` (the catalogue lists the model returns): hits from anywhere in the list, tracks OUTSIDE
    the catalogue (never hit, counted), ids beyond the vocabulary, -1, duplicates; row 2 holds 300 answers."""
    outside = np.setdiff1d(np.arange(n_tracks), cols)
    out = []
    for r, row in enumerate(idx):
        cand = row[row >= 0]
        n = 300 if r == 2 else int(rng.integers(1, 60))
        take = 0 if r % 7 == 3 or not cand.size else int(rng.integers(1, min(n, cand.size) + 1))
        a = rng.choice(cand, size=take, replace=False).tolist() + rng.choice(outside, size=n - take, replace=True).tolist()
        if r % 7 == 1 and cand.size:
            a[0] = int(cand[0])
        if r % 7 == 5:
            a = a + [-1] * 3 + a[:3] + [n_tracks + 77]
        out.append([int(x) for x in rng.permutation(a)])
    return out


def _check_records(rec, idx, answers):
    assert rec.dtype == met.RECORD_DTYPE and len(rec) == len(idx) == len(answers)
    want = met.rank_records(idx, answers)
    for f in ("hits_r", "first", "m", "n_answer"):
        assert np.array_equal(rec[f], want[f]), f
    assert np.array_equal(rec["dcg"].view(np.uint64), want["dcg"].view(np.uint64))
    for r in range(len(idx)):
        assert met.finish_record(rec[r]) == metrics_reference(idx[r], answers[r])


@pytest.mark.parametrize("name", ["f32", "bf16", "exact_bf16"])
def test_evaluate_iter_in_a_catalogue(model, name):
    m, cols = model, CATS["a3000"]
    h = m.catalogue(cols)
    try:
        seq = _stream()[:30]
        feeds = [_feed(*x) for x in seq]
        want = _want(m, name, h)
        lists = [want[(i, ex)][0][:n] for i, ex, n in seq]
        rng = np.random.default_rng(5)
        answers = [_answers(rng, idx, cols, NT) for idx in lists]
        assert any(len(a) >= 300 for ans in answers for a in ans)
        got = list(m.evaluate_iter(zip(feeds, answers), k=K, dtype=name, catalogue=h))
        assert [len(g) for g in got] == [n for _i, _e, n in seq]
        for rec, idx, ans in zip(got, lists, answers):
            _check_records(rec, idx, ans)
        assert sum(int(g["hits_r"].sum()) for g in got) > 100
        pipes = [p for key, (_g, p) in m._pipes.items() if ("catalogue", id(h)) in key and "eval" in key]
        assert len(pipes) == 1 and pipes[0].eval and 0 < pipes[0].stats()["launches"] < len(feeds) - 1
    finally:
        h.close()


def test_titled_evaluate_iter_in_a_catalogue(tmp_path):
    m, c = _title_model(tmp_path)
    cols = random_catalogue(TNT, 700, seed=700)
    feeds = _titled_feeds()
    h = m.catalogue(cols)
    try:
        for name in ("f32", "bf16"):
            lists = [w[0] for w in _titled_want(m, feeds, name, h)]
            rng = np.random.default_rng(6)
            answers = [_answers(rng, idx, cols, TNT) for idx in lists]
            got = list(m.evaluate_iter(zip(feeds, answers), k=K, dtype=name, catalogue=h))
            assert [len(g) for g in got] == [f[3] for f in feeds]
            for rec, idx, ans in zip(got, lists, answers):
                _check_records(rec, idx, ans)
    finally:
        h.close()
        m.close_pipelines()


# ---- rank_candidates(catalogue=) -------------------------------------------------------------------------------------------------------
def _cand_lists(rng, n_rows, n_tracks, cols, n_input):
    """Per row a candidate list with repeats, -1 padding and artist columns; row 1's candidates all lie OUTSIDE the catalogue."""
    outside = np.setdiff1d(np.arange(n_tracks), cols)
    out = []
    for r in range(n_rows):
        a = rng.integers(0, n_tracks, size=int(rng.integers(50, 400))).tolist() + rng.choice(cols, size=60).tolist()
        a += [-1, a[0], a[1], int(n_input - 1)]
        out.append(outside[:80].tolist() if r == 1 else [int(x) for x in rng.permutation(a)])
    return out


def _by_hand(cands, cols):
    keep = set(int(c) for c in cols)
    return [sorted(set(int(x) for x in row if x in keep)) for row in cands]


def test_rank_candidates_in_a_catalogue(model):
    m, cols = model, CATS["a3000"]
    h = m.catalogue(cols)
    try:
        pos, ones, seeds = BASE[1]
        cands = _cand_lists(np.random.default_rng(1), B, NT, cols, V)
        for sd in (SEEDS_FROM_INPUT, seeds):
            got = m.rank_candidates(pos, ones, cands, sd, k=K, catalogue=h)
            want = m.rank_candidates(pos, ones, _by_hand(cands, cols), sd, k=K)
            assert _eq(got, want)
            assert (got[0][1] == -1).all() and np.isneginf(got[1][1]).all()       # nothing of row 1 lies in the catalogue
            assert (got[0][0] >= 0).any() and np.isin(got[0][got[0] >= 0], cols).all()
            assert not _eq(got, m.rank_candidates(pos, ones, cands, sd, k=K))
        arr = np.full((B, 50), -1, np.int64)
        arr[:, :40] = np.random.default_rng(2).integers(0, NT, (B, 40))
        arr[:, 40:45] = cols[:5]
        assert _eq(m.rank_candidates(pos, ones, arr[:20], seeds, k=K, n_rows=20, catalogue=h),
                   m.rank_candidates(pos, ones, _by_hand(arr[:20].tolist(), cols), seeds, k=K, n_rows=20))
    finally:
        h.close()
    with pytest.raises(ValueError, match="closed"):
        m.rank_candidates(pos, ones, cands, seeds, k=K, catalogue=h)


def test_titled_rank_candidates_in_a_catalogue(tmp_path):
    m, c = _title_model(tmp_path)
    cols = random_catalogue(TNT, 700, seed=700)
    h = m.catalogue(cols)
    try:
        pos, ones, seeds, _n, titles, use = _titled_feeds(1)[0]
        P = np.asarray(pos, np.int64).reshape(-1, 2)
        seeds = [sorted(set(P[(P[:, 0] == r) & (P[:, 1] < TNT), 1].tolist())) for r in range(TB)]
        cands = _cand_lists(np.random.default_rng(3), TB, TNT, cols, TV)
        got = m.rank_candidates(pos, ones, cands, seeds, k=K, titles=titles, titles_use=use, catalogue=h)
        want = m.rank_candidates(pos, ones, _by_hand(cands, cols), seeds, k=K, titles=titles, titles_use=use)
        assert _eq(got, want) and (got[0][1] == -1).all() and (got[0][0] >= 0).any()
        assert not _eq(got, m.rank_candidates(pos, ones, cands, seeds, k=K, titles=titles, titles_use=use))
    finally:
        h.close()
