"""GPU (-m gpu): rank_of -- the exact rank of given tracks among all rankable tracks of a row (csrc/rank_of.hip) -- against the
CPU oracle.  oracle.encode -> oracle.decode -> oracle.topk(k = n_tracks, seeds) is the whole canonical ordering of a row; an
answer's rank is its position in it.  Ranks are compared as integers, logits by their bits: no tolerance anywhere."""
import pickle

import numpy as np
import pytest

import oracle
from oracle import title_numpy as tn
from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.models.DAEs import DAE, DAE_title, SEEDS_FROM_INPUT, coo_to_csr, seeds_to_csr
from spotify_recsys_challenge_2018_amd.models.title_models import get_model
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights

pytestmark = pytest.mark.gpu
F32 = _lib.DAE_DTYPE_F32
U32 = np.uint32


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _some(a, dtype):
    return a if a.size else np.zeros(1, dtype)


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(U32), b.view(U32))


# ---- problems and their references: computed once per shape, shared, left unchanged ------------------------------------------
_WEIGHTS, _PROBLEMS = {}, {}


def _weights(V, nt, H):
    if (V, nt, H) not in _WEIGHTS:
        W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=V + H, bias="zipf", n_tracks=nt)
        b_enc = (np.random.default_rng(H + 3).standard_normal(H) * 0.1).astype(np.float32)
        _WEIGHTS[(V, nt, H)] = (W_enc, b_enc, W_dec, b_dec)
    return _WEIGHTS[(V, nt, H)]


def _order_and_place(z, nt, srp, sc):
    """The canonical ordering of every row's rankable tracks and, per (row, track), its place in it (-1: a seed)."""
    _s, order = oracle.topk(z, nt, srp, sc, ncols=nt, out_kind=_lib.DAE_OUT_LOGIT)
    B = z.shape[0]
    place = np.full((B, nt), -1, np.int32)
    for r in range(B):
        o = order[r][order[r] >= 0]
        place[r, o] = np.arange(o.size, dtype=np.int32)
    return order, place


def _finish_problem(W, V, nt, B, pos, ones, seeds, rows=None):
    W_enc, b_enc, W_dec, b_dec = W
    rp, col, val = coo_to_csr(pos, ones, B, V)
    h = oracle.encode(rp, col, val, W_enc, b_enc)
    sel = np.arange(B) if rows is None else np.asarray(rows)
    z = oracle.decode(h[sel], W_dec, b_dec, 0, nt)               # the track columns are all a rank needs
    return rp, col, val, h, sel, z


def _problem(V, nt, B, H):
    """Row 0 has no seeds, row 1 has 250 (the most popular columns among them), row 2 has the row's own top 50 columns."""
    key = (V, nt, B, H)
    if key not in _PROBLEMS:
        W = _weights(V, nt, H)
        pos, ones, seeds = make_playlists(B, nt, V - nt, seed=B + 1)
        rng = np.random.default_rng(B + 2)
        seeds[0] = []
        seeds[1] = np.unique(np.concatenate([np.arange(100), rng.permutation(nt)[:150]]))[:250].tolist()
        rp, col, val, h, _sel, z = _finish_problem(W, V, nt, B, pos, ones, seeds)
        top50 = np.lexsort((np.arange(nt), -_okey(z[2])))[:50]
        seeds[2] = sorted(int(c) for c in top50)
        srp, sc = seeds_to_csr(seeds, B, nt)
        order, place = _order_and_place(z, nt, srp, sc)
        _PROBLEMS[key] = dict(V=V, nt=nt, B=B, H=H, W=W, pos=pos, ones=ones, seeds=seeds, rp=rp, col=col, val=val, h=h, z=z,
                              srp=srp, sc=sc, order=order, place=place)
    return _PROBLEMS[key]


def _okey(z):
    u = np.asarray(z, np.float32).view(U32)
    u = np.where((u << U32(1)) == 0, U32(0), u)
    return np.where(u >> U32(31), ~u, u | U32(0x80000000)).astype(np.int64)


def _want(p, lists, rows=None):
    """(ranks, logits) of the listed answers by the reference, flattened in list order."""
    nt, V = p["nt"], p["V"]
    ranks, logits = [], []
    for r, cs in enumerate(lists):
        zr = p["z"][r if rows is None else rows[r]]
        pr = p["place"][r if rows is None else rows[r]]
        for c in np.asarray(cs, np.int64):
            ok = 0 <= c < nt
            ranks.append(int(pr[c]) if ok else -1)
            logits.append(zr[c] if ok and pr[c] >= 0 else (np.float32(-np.inf) if -1 <= c < V else np.float32(np.nan)))
    return np.asarray(ranks, np.int32), np.asarray(logits, np.float32)


def _csr(lists, B):
    lens = np.zeros(B, np.int64)
    lens[:len(lists)] = [len(x) for x in lists]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)]).astype(np.int32)
    return rp, col


def _prepacked(ctx, p):
    W_enc, b_enc, W_dec, b_dec = p["W"]
    d = dict(We=_dev(W_enc), be=_dev(b_enc), Wd=_dev(W_dec), bd=_dev(b_dec))
    ctx.prepack_decoder(d["Wd"], d["bd"], dtype=F32)
    return d


def _rank_of(ctx, p, d, lists, score_call=False, seeds=True, status_want=0):
    """One call through the C ABI -> (ranks, logits) on the host; nothing may be written past n_ans."""
    import torch
    B = p["B"]
    rp, col = _csr(lists, B)
    n = int(col.size)
    ans = (_dev(rp), _dev(_some(col, np.int32)))
    rank = torch.full((n + 3,), -7, dtype=torch.int32, device="cuda")
    logit = torch.full((n + 3,), 7.0, dtype=torch.float32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    srp, sc = (_dev(p["srp"]), _dev(_some(p["sc"], np.int32))) if seeds else (None, None)
    if score_call:
        ctx.score_rank_of(_dev(p["rp"]), _dev(_some(p["col"], np.int32)), _dev(_some(p["val"], np.float32)), d["We"], d["be"],
                          d["Wd"], d["bd"], p["nt"], srp, sc, ans, n, rank, out_logit=logit, status=status)
    else:
        ctx.decode_rank_of(_dev(p["h"]), d["Wd"], d["bd"], p["nt"], srp, sc, ans, n, rank, out_logit=logit, status=status)
    r, l = rank.cpu().numpy(), logit.cpu().numpy()
    assert (r[n:] == -7).all() and (l[n:] == 7.0).all()
    assert int(status.item()) == status_want
    return r[:n], l[:n]


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
    """Row lengths 0, 1, C, C + 1, 3 C + 5 on the first rows and on the last one; the others hold 0 or 1 answer, so the batch's
    average stays small and the plan keeps the tallest row group the batch allows."""
    B = p["B"]
    rng = np.random.default_rng(seed)
    lens = [r % 2 for r in range(B)]
    for r, L in zip(range(6), (0, 1, C, C + 1, 3 * C + 5, 2)):
        lens[r] = L
    lens[B - 1] = C + 1
    return [_list_of(p, r, L, rng) for r, L in enumerate(lens)]


SHAPES = {                      # V, tracks, B, H, rows per row group the edge lists must get
    "one_short_group": (33000, 30011, 37, 256, 64),
    "three_groups_last_of_one_row": (33000, 30011, 257, 256, 128),
    "small_vocabulary_h64": (9000, 8000, 40, 64, 64),
    "small_hidden_h64": (40000, 33000, 40, 64, 64),
    "hidden_128": (9000, 8000, 40, 128, 64),
    "few_ranked_tiles": (33000, 6000, 128, 256, 128),
}


def _stable_plan(B, H, make_lists):
    """The lists are built from the plan's capacity, which depends on their total: settle it."""
    plan = _lib.rank_of_plan(B, H, B)
    for _ in range(4):
        lists = make_lists(plan["capacity"])
        again = _lib.rank_of_plan(B, H, sum(len(x) for x in lists))
        if again == plan:
            return plan, lists
        plan = again
    raise AssertionError("the plan does not settle")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ---- 1. answer-row lengths at every shape -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_row_lengths(ctx, name):
    V, nt, B, H, rows_want = SHAPES[name]
    p = _problem(V, nt, B, H)
    d = _prepacked(ctx, p)
    plan, lists = _stable_plan(B, H, lambda C: _edge_lists(p, C, seed=B + H))
    assert plan["rows"] == rows_want, plan
    C = plan["capacity"]
    assert sorted({len(x) for x in lists} & {0, 1, C, C + 1, 3 * C + 5}) == sorted({0, 1, C, C + 1, 3 * C + 5})
    wr, wl = _want(p, lists)
    # the lists do hold rank 0, the last rank, and every kind of unrankable answer
    n_rankable = [int((p["order"][r] >= 0).sum()) for r in range(B)]
    assert 0 in wr and (n_rankable[4] - 1) in wr and -1 in wr
    r, l = _rank_of(ctx, p, d, lists)
    assert np.array_equal(r, wr), (plan, np.nonzero(r != wr)[0][:10], r[r != wr][:10], wr[r != wr][:10])
    assert _bits_equal(l, wl)


def test_many_answers_take_the_shorter_row_group(ctx):
    """257 rows with 30 answers each: the plan halves the row group (five groups of 64) so that one pass holds a row."""
    V, nt, B, H, _ = SHAPES["three_groups_last_of_one_row"]
    p = _problem(V, nt, B, H)
    d = _prepacked(ctx, p)
    rng = np.random.default_rng(3)
    lists = [_list_of(p, r, 30, rng) for r in range(B)]
    plan = _lib.rank_of_plan(B, H, 30 * B)
    assert plan["rows"] == 64 and plan["row_groups"] == 5 and plan["capacity"] >= 30, plan
    wr, wl = _want(p, lists)
    r, l = _rank_of(ctx, p, d, lists)
    assert np.array_equal(r, wr) and _bits_equal(l, wl)


# ---- 2. self-consistency without the oracle ---------------------------------------------------------------------------------------
PV, PNT, PH, PB = 6000, 5000, 64, 6


@pytest.fixture(scope="module")
def py_problem():
    W_enc, b_enc, W_dec, b_dec = make_weights(PV, PH, seed=21, bias="zipf", n_tracks=PNT)
    pos, ones, seeds = make_playlists(PB, PNT, PV - PNT, seed=22)
    return dict(W_enc=W_enc, b_enc=b_enc, W_dec=W_dec, b_dec=b_dec, pos=pos, ones=ones, seeds=seeds)


def _model(p, decode_dtype="f32", cls=DAE):
    class C:
        save = "/tmp/_rankof_unused"; n_input = PV; lr = 0.01; reg_lambda = 0.0; initval = "NULL"
        batch = PB; hidden = PH; n_tracks = PNT
    C.decode_dtype = decode_dtype
    m = cls(C())
    m._host_init = lambda: [p["W_enc"], p["W_dec"], p["b_enc"], p["b_dec"]]
    m.fit()
    return m


@pytest.mark.parametrize("name", ["f32", "exact_bf16"])
@pytest.mark.parametrize("seeds_from_input", [False, True])
def test_ranks_of_a_recommended_list_are_its_positions(py_problem, name, seeds_from_input):
    p = py_problem
    m = _model(p, decode_dtype=name)
    k = 500
    seeds = SEEDS_FROM_INPUT if seeds_from_input else p["seeds"]
    idx, score = m.recommend(p["pos"], p["ones"], seeds, k=k)
    cols = np.concatenate([idx, np.full((PB, 2), -1, idx.dtype)], axis=1)     # ... and -1 beside a -1
    ranks, logits = m.rank_of(p["pos"], p["ones"], cols, seeds, want_logits=True)
    assert ranks.dtype == np.int32 and ranks.shape == cols.shape and logits.dtype == np.float32
    assert (idx >= 0).all()
    assert np.array_equal(ranks[:, :k], np.tile(np.arange(k, dtype=np.int32), (PB, 1)))
    assert (ranks[:, k:] == -1).all() and np.isneginf(logits[:, k:]).all()
    assert _bits_equal(oracle.sigmoid(logits[:, :k]), score)
    # the ragged form, fewer lists than rows
    ragged = m.rank_of(p["pos"], p["ones"], [idx[0, ::-1], [], idx[2, :3]], seeds)
    assert len(ragged) == PB and np.array_equal(ragged[0], np.arange(k)[::-1]) and ragged[1].size == 0
    assert np.array_equal(ragged[2], [0, 1, 2]) and all(x.size == 0 for x in ragged[3:])


# ---- 3. ties --------------------------------------------------------------------------------------------------------------------
def test_identical_decoder_rows_rank_by_column():
    """Pairs of identical decoder rows and biases: inside one tile, in different tiles, one of the pair a seed, both among the
    answers.  The GEMM's value at the answer's own column equals the threshold, and so does its twin's: only the column tells
    them apart."""
    V, nt, B, H = 2000, 1500, 8, 64
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=5, bias="zipf", n_tracks=nt)
    W_dec, b_dec = W_dec.copy(), b_dec.copy()
    rng = np.random.default_rng(6)
    pairs = [(5, 9), (33, 63), (40, 700), (100, 1400), (31, 32), (0, 1499)] + \
            [tuple(x) for x in rng.permutation(np.arange(200, 1400))[:60].reshape(30, 2)]
    for a, b in pairs:
        W_dec[b] = W_dec[a]; b_dec[b] = b_dec[a]
    pos, ones, seeds = make_playlists(B, nt, V - nt, seed=7)
    seeds[0] = [5, 700]; seeds[1] = [9, 40, 100]; seeds[2] = []
    W = (W_enc, b_enc, W_dec, b_dec)
    rp, col, val, h, _sel, z = _finish_problem(W, V, nt, B, pos, ones, seeds)
    assert all(z[0, a] == z[0, b] for a, b in pairs)
    srp, sc = seeds_to_csr(seeds, B, nt)
    order, place = _order_and_place(z, nt, srp, sc)
    p = dict(V=V, nt=nt, B=B, H=H, W=W, rp=rp, col=col, val=val, h=h, z=z, srp=srp, sc=sc, order=order, place=place)
    flat = [c for ab in pairs for c in ab]
    lists = [rng.permutation(np.asarray(flat + flat[:7], np.int64)) for _ in range(B)]
    wr, wl = _want(p, lists)
    c = _lib.Context(0)
    try:
        d = _prepacked(c, p)
        r, l = _rank_of(c, p, d, lists)
    finally:
        c.close()
    assert np.array_equal(r, wr) and _bits_equal(l, wl)
    # where neither of a pair is a seed the two ranks are neighbours, the smaller column first
    got = dict(zip(lists[2].tolist(), r[sum(len(x) for x in lists[:2]):][:len(lists[2])].tolist()))
    assert all(got[max(a, b)] == got[min(a, b)] + 1 for a, b in pairs)


def test_every_logit_ties():
    """W_dec = 0, b_dec = 0: every logit of every row is +0 -- the rank of c is the number of non-seed tracks below c."""
    V, nt, B, H = 3000, 2600, 8, 64
    W_enc, b_enc, _W, _b = make_weights(V, H, seed=8, n_tracks=nt)
    W = (W_enc, b_enc, np.zeros((V, H), np.float32), np.zeros(V, np.float32))
    pos, ones, seeds = make_playlists(B, nt, V - nt, seed=9)
    seeds[0] = []
    seeds[1] = list(range(0, 500, 2))
    rp, col, val, h, _sel, z = _finish_problem(W, V, nt, B, pos, ones, seeds)
    srp, sc = seeds_to_csr(seeds, B, nt)
    order, place = _order_and_place(z, nt, srp, sc)
    p = dict(V=V, nt=nt, B=B, H=H, W=W, rp=rp, col=col, val=val, h=h, z=z, srp=srp, sc=sc, order=order, place=place)
    rng = np.random.default_rng(10)
    lists = [rng.integers(0, nt, 300) for _ in range(B)]
    lists[3] = np.arange(nt)[::-1]                                # every track, from the last
    wr, wl = _want(p, lists)
    for r_, cs in enumerate(lists[:2]):                           # the reference is the closed form
        sd = np.asarray(sorted(set(seeds[r_])), np.int64)
        closed = np.where(np.isin(cs, sd), -1, cs - np.searchsorted(sd, cs))
        assert np.array_equal(closed, wr[sum(len(x) for x in lists[:r_]):][:len(cs)])
    c = _lib.Context(0)
    try:
        d = _prepacked(c, p)
        r, l = _rank_of(c, p, d, lists)
    finally:
        c.close()
    assert np.array_equal(r, wr) and _bits_equal(l, wl)


# ---- 4. seeds -------------------------------------------------------------------------------------------------------------------
def test_seeds_leave_exactly_their_places(ctx):
    """Rows with 0, 250 and the row's own top 50 columns as seeds: against the unseeded ranks every answer drops by exactly the
    seeds that precede it."""
    V, nt, B, H, _ = SHAPES["one_short_group"]
    p = _problem(V, nt, B, H)
    d = _prepacked(ctx, p)
    assert len(p["seeds"][0]) == 0 and len(set(p["seeds"][1])) == 250 and len(p["seeds"][2]) == 50
    rng = np.random.default_rng(11)
    o2 = p["order"][2]
    lists = [rng.integers(0, nt, 40) for _ in range(B)]
    lists[2] = np.concatenate([o2[:30], p["seeds"][2][:5], rng.integers(0, nt, 20)]).astype(np.int64)
    lists[1] = np.concatenate([np.arange(90, 130), p["seeds"][1][-5:], rng.integers(0, nt, 20)]).astype(np.int64)
    wr, wl = _want(p, lists)
    r, l = _rank_of(ctx, p, d, lists)
    assert np.array_equal(r, wr) and _bits_equal(l, wl)
    r0, l0 = _rank_of(ctx, p, d, lists, seeds=False)
    rp, _col = _csr(lists, B)
    for row in (0, 1, 2):
        sd = np.asarray(p["seeds"][row], np.int64)
        key_c = lambda c: (-_okey(p["z"][row, c]), c)
        for i in range(rp[row], rp[row + 1]):
            c = int(lists[row][i - rp[row]])
            if c in set(sd.tolist()):
                assert r[i] == -1 and r0[i] >= 0 and np.isneginf(l[i]) and not np.isneginf(l0[i])
            else:
                before = sum(1 for s in sd.tolist() if key_c(s) < key_c(c))
                assert r[i] == r0[i] - before
    first = slice(rp[2], rp[2] + 30)
    assert np.array_equal(r[first], np.arange(30)) and np.array_equal(r0[first], np.arange(30) + 50)


# ---- 5. state ---------------------------------------------------------------------------------------------------------------------
def test_one_context_across_sizes_equals_fresh_contexts():
    """257 -> 37 -> 257 rows on ONE context, different answer shapes, nothing reset: the counters are zeroed by the call and the
    scratch is reused across sizes."""
    V, nt, _B, H, _ = SHAPES["one_short_group"]
    big, small = _problem(V, nt, 257, H), _problem(V, nt, 37, H)
    rng = np.random.default_rng(12)
    calls = [(big, [_list_of(big, r, 25 + r % 9, rng) for r in range(257)]),
             (small, [_list_of(small, r, (0, 1, 140, 7)[r % 4], rng) for r in range(37)]),
             (big, [_list_of(big, r, (3, 0)[r % 2], rng) for r in range(257)])]
    one = _lib.Context(0)
    try:
        d = _prepacked(one, big)
        got = [_rank_of(one, p, d, lists) for p, lists in calls]
        grown = one.lib.dae_scratch_bytes(one.h)
        again = _rank_of(one, big, d, calls[0][1])
        assert one.lib.dae_scratch_bytes(one.h) == grown          # a steady state allocates nothing
    finally:
        one.close()
    for (p, lists), (r, l) in zip(calls, got):
        fresh = _lib.Context(0)
        try:
            fr, fl = _rank_of(fresh, p, _prepacked(fresh, p), lists)
        finally:
            fresh.close()
        wr, wl = _want(p, lists)
        assert np.array_equal(r, fr) and _bits_equal(l, fl) and np.array_equal(r, wr) and _bits_equal(l, wl)
    assert np.array_equal(again[0], got[0][0]) and _bits_equal(again[1], got[0][1])


# ---- 6. the two entry points ----------------------------------------------------------------------------------------------------
def test_score_call_equals_encode_plus_decode_call(ctx):
    import torch
    V, nt, B, H, _ = SHAPES["one_short_group"]
    p = _problem(V, nt, B, H)
    d = _prepacked(ctx, p)
    rng = np.random.default_rng(13)
    lists = [_list_of(p, r, 20 + r, rng) for r in range(B)]
    h = torch.empty((B, H), device="cuda")
    ctx.encode(_dev(p["rp"]), _dev(p["col"]), _dev(p["val"]), d["We"], d["be"], h)
    assert _bits_equal(h.cpu().numpy(), p["h"])
    a = _rank_of(ctx, p, d, lists)
    b = _rank_of(ctx, p, d, lists, score_call=True)
    assert np.array_equal(a[0], b[0]) and _bits_equal(a[1], b[1])
    wr, wl = _want(p, lists)
    assert np.array_equal(b[0], wr) and _bits_equal(b[1], wl)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    import torch
    V, nt, B, H, _ = SHAPES["small_vocabulary_h64"]
    p = _problem(V, nt, B, H)
    W_enc, b_enc, W_dec, b_dec = p["W"]
    Wd, bd, h = _dev(W_dec), _dev(b_dec), _dev(p["h"])
    lists = [[1, 2, 3]] * B
    rp, col = _csr(lists, B)
    ans = (_dev(rp), _dev(col))
    n = int(col.size)
    srp, sc = _dev(p["srp"]), _dev(_some(p["sc"], np.int32))
    rank = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    logit = torch.full((n,), 7.0, device="cuda")

    def refused(c, match, **kw):
        a = dict(n_tracks=nt, srp=srp, sc=sc, n=n)
        a.update(kw)
        before = c.lib.dae_scratch_bytes(c.h)
        with pytest.raises(_lib.DaeError, match=match):
            c.decode_rank_of(h, Wd, bd, a["n_tracks"], a["srp"], a["sc"], ans, a["n"], rank, out_logit=logit)
        torch.cuda.synchronize()
        assert c.lib.dae_scratch_bytes(c.h) == before
        assert bool((rank == -7).all()) and bool((logit == 7.0).all())

    c = _lib.Context(0)
    try:
        refused(c, "none is prepacked")
        c.prepack_decoder(Wd, bd, dtype=_lib.DAE_DTYPE_BF16)
        refused(c, "none is prepacked")                           # a bf16 image is no fp32 image
        c.prepack_decoder(Wd, bd, 0, V // 2, dtype=F32)
        refused(c, "shard image")
        cat = _lib.Catalogue(c, _dev(np.arange(0, nt, 3, dtype=np.int32)), nt)
        c.prepack_decoder_catalogue(cat, Wd, bd, dtype=F32)
        refused(c, "catalogue image")
        c.prepack_decoder(Wd, bd, dtype=F32)
        refused(c, "n_ans=-1", n=-1)
        refused(c, "both be given or both null", sc=None)
        refused(c, "both be given or both null", srp=None)
        refused(c, "n_tracks", n_tracks=V + 1)
        refused(c, "n_tracks", n_tracks=0)
        cat.close()
        # an id >= V: rank -1, status bit 0, a NaN logit, the neighbours unharmed
        d = dict(Wd=Wd, bd=bd)
        bad = [[5, V, 6], [V + 7, 9], [-2, 10]] + [[11]] * (B - 3)
        r, l = _rank_of(c, p, d, bad, status_want=1)
        wr, wl = _want(p, bad)
        assert np.array_equal(r, wr) and r[1] == -1 and r[3] == -1 and r[5] == -1
        assert np.isnan(l[[1, 3, 5]]).all() and _bits_equal(np.delete(l, [1, 3, 5]), np.delete(wl, [1, 3, 5]))
    finally:
        c.close()


def test_python_refusals(py_problem, tmp_path):
    p = py_problem
    m = _model(p)
    with pytest.raises(ValueError, match="out of range"):
        m.rank_of(p["pos"], p["ones"], [[1, PV]], p["seeds"])
    with pytest.raises(ValueError, match="out of range"):
        m.rank_of(p["pos"], p["ones"], np.asarray([[1, -2]]), p["seeds"])
    m.shard_scoring(0, 2)
    with pytest.raises(_lib.DaeError, match="scoring shard"):
        m.rank_of(p["pos"], p["ones"], [[1, 2]], p["seeds"])

    class Conf:
        lr = 0.01; reg_lambda = 0.0; charsize = 41; char_model = 'Char_CNN'; save = "/tmp/_rankof_unused"
        initval = "NULL"; title_lr = 0.002; batch = PB; n_input = PV; n_output = PV; n_tracks = PNT; hidden = PH
        char_emb = 25; filter_size = [3, 5]; filter_num = 40; strmaxlen = 25
    c = Conf()
    pk = tmp_path / "w_dae"
    with open(pk, "wb") as f:
        pickle.dump([p["W_enc"], p["W_dec"], p["b_enc"], p["b_dec"]], f)
    c.DAEval = str(pk)
    mt = get_model(c)
    mt.fit(tn.make_params(41, 25, [3, 5], 40, c.n_output, seed=4))
    t = DAE_title(c, mt)
    t.fit()
    titles = np.zeros((PB, 25), np.int32)
    with pytest.raises(ValueError, match="title mix"):
        t.rank_of(p["pos"], p["ones"], [[1, 2]], p["seeds"], titles=titles, titles_use=np.ones(PB, np.float32))
    # without titles in use it ranks the plain DAE logits, as the untitled model does
    cols = np.arange(0, 400, 7).reshape(1, -1)
    assert np.array_equal(t.rank_of(p["pos"], p["ones"], cols, p["seeds"], titles=titles, titles_use=np.zeros(PB, np.float32)),
                          _model(p).rank_of(p["pos"], p["ones"], cols, p["seeds"]))


# ---- 8. the shipped shape, once ---------------------------------------------------------------------------------------------------
def test_shipped_shape():
    """|vocab| 170 000, 140 000 tracks, 256 rows, hidden 256, 100 answers per row: 16 sampled rows against the oracle."""
    V, nt, B, H = 170000, 140000, 256, 256
    W = _weights(V, nt, H)
    pos, ones, seeds = make_playlists(B, nt, V - nt, seed=31)
    rows = np.unique(np.concatenate([[0, 1, 255], np.random.default_rng(1).permutation(B)[:16]]))[:16]
    rp, col, val, h, _sel, z = _finish_problem(W, V, nt, B, pos, ones, seeds, rows=rows)
    srp, sc = seeds_to_csr(seeds, B, nt)
    srp_r = np.concatenate([[0], np.cumsum(np.diff(srp)[rows])]).astype(np.int32)
    sc_r = np.concatenate([sc[srp[r]:srp[r + 1]] for r in rows]).astype(np.int32)
    order, place = _order_and_place(z, nt, srp_r, _some(sc_r, np.int32))
    p = dict(V=V, nt=nt, B=B, H=H, W=W, rp=rp, col=col, val=val, h=h, z=z, srp=srp, sc=sc, order=order, place=place,
             seeds=seeds)
    rng = np.random.default_rng(32)
    lists = [rng.integers(0, nt, 100) for _ in range(B)]
    for i, r in enumerate(rows):
        lists[r][:6] = [order[i][0], order[i][499], order[i][500], order[i][120000], seeds[r][0], -1]
    wr, wl = _want(p, [lists[r] for r in rows], rows=np.arange(rows.size))
    c = _lib.Context(0)
    try:
        d = _prepacked(c, p)
        r, l = _rank_of(c, p, d, lists, score_call=True)
    finally:
        c.close()
    pick = np.concatenate([np.arange(100 * r, 100 * r + 100) for r in rows])
    assert np.array_equal(r[pick], wr) and _bits_equal(l[pick], wl)
    assert {0, 499, 500, 120000} <= set(wr.tolist())


# ---- 9. the driver ----------------------------------------------------------------------------------------------------------------
def test_driver_logs_one_rank_line_per_split_with_eval_ranks_on(tmp_path):
    """main.py --dae --testmode on the golden mini dataset: without the key (and with `off`) the log is what it was; with
    [BASE] eval_ranks = on one more line per split follows the existing ones; --title refuses the key by name."""
    import os
    import random
    import shutil
    from spotify_recsys_challenge_2018_amd import main as cli
    G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    work = tmp_path / "run"
    work.mkdir()
    shutil.copy(os.path.join(G, "config.ini"), work / "config.ini")
    shutil.copytree(os.path.join(G, "data"), tmp_path / "data")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        random.seed(0); np.random.seed(0)
        assert cli.main(["--dir", "run", "--pretrain"]) == 0
        assert cli.main(["--dir", "run", "--dae"]) == 0
        splits = ("test-0", "test-1", "test-5", "test-25r")
        ini = open(work / "config.ini").read()

        def testmode_lines(base_key):
            open(work / "config.ini", "w").write(ini.replace("[BASE]", "[BASE]\n" + base_key))
            n0 = len(open(work / "log.txt").read().splitlines())
            assert cli.main(["--dir", "run", "--dae", "--testmode"]) == 0
            return [l for l in open(work / "log.txt").read().splitlines()[n0:] if l.startswith("seed num")]
        plain = testmode_lines("")
        assert len(plain) == 4 and testmode_lines("eval_ranks = off") == plain
        full = testmode_lines("eval_ranks = on")
        assert len(full) == 8 and full[:4] == plain
        for l, s in zip(full[4:], splits):
            assert l.startswith("seed num: %s ranks: mrr " % s), l
            w = l.split()
            mrr, med = float(w[w.index("mrr") + 1]), float(w[w.index("median") + 1])
            rec = [float(w[w.index("recall@%d" % k) + 1]) for k in (500, 1000, 5000, 10000)]
            assert 0.0 < mrr <= 1.0 and med >= 0.0 and rec == sorted(rec) and 0.0 <= rec[0] and rec[-1] <= 1.0
        with pytest.raises(ValueError, match="eval_ranks"):
            cli.main(["--dir", "run", "--title", "--testmode"])
    finally:
        os.chdir(cwd)
