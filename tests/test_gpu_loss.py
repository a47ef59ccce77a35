"""GPU (-m gpu): the loss without a step -- dae_decode_loss_rows / dae_score_loss (csrc/loss_rows.hip, decode_f32_kernel's
EPI_ROWLOSS), model.loss, Session.run(model.cost) and [BASE] eval_loss.

The cost and every row's loss are checked against the rounding-aware float64 reference of the training step
(oracle/dae_numpy.py grads_f32 / grads_bf16 with the fp32 head, on the GPU's own hidden rows), under the intervals the
reference derives -- no tolerance of this file's own:

  cost     inside dn.cost_interval(ref, bounds);
  row r    inside [sum_c L_lo[r, c] - w_r, sum_c L_hi[r, c] + w_r],  w_r = (V + 2) U32 sum_c max(|L_lo|, |L_hi|)[r, c]:
           cost_interval's summation term restricted to a row (V fp32 terms in any order; the partials' double sums and
           the final rounding are inside the + 2).
"""
import functools
import os
import pickle
import random
import shutil

import numpy as np
import pytest

from oracle import dae_numpy as dn
from spotify_recsys_challenge_2018_amd import _lib
from test_gpu_train_bf16_ref import SEED, _dev, make_case, run_step
from test_train_saturated_reference_cpu import planted_case

pytestmark = pytest.mark.gpu
F32, BF16 = _lib.DAE_DTYPE_F32, _lib.DAE_DTYPE_BF16
DTYPES = [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16")]
ERR_ARG, ERR_STATE = -1, -4


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _tensors(c):
    csr = [_dev(a if a.size else np.zeros(1, a.dtype)) for a in c["csr"]]
    return csr[:3], csr[3:], [_dev(a) for a in c["W"]]


def _prepack(ctx, c, W, dtype):
    ctx.prepack_decoder(W[0] if c["tied"] else W[2], W[3], 0, c["V"], dtype)


def score_loss(ctx, c, dtype, want_rows=True, want_cost=True, prepack=True, tensors=None):
    """dae_score_loss of case c on ctx in `dtype` -> (cost or None, rows or None) as host values."""
    import torch
    x, y, W = tensors or _tensors(c)
    ctx.set_train_dtype(dtype)
    if prepack:
        _prepack(ctx, c, W, dtype)
    rows = torch.full((c["B"],), float("nan"), device="cuda") if want_rows else None
    cost = torch.full((1,), float("nan"), device="cuda") if want_cost else None
    ctx.score_loss(x, y, W[0], W[1], None if c["tied"] else W[2], W[3], c["n_batch"], c["tied"], ikp=c["ikp"], kp=c["kp"],
                   seed=SEED, reg_lambda=c["lam"], row_loss=rows, cost_out=cost)
    torch.cuda.synchronize()
    return (float(cost.item()) if want_cost else None), (rows.cpu().numpy() if want_rows else None)


def gpu_hidden(ctx, c):
    """The GPU's own hidden rows of the case (the step's encode: same masks for the same seed)."""
    import torch
    x, _y, W = _tensors(c)
    h = torch.empty((c["B"], c["H"]), device="cuda")
    ctx.encode(x[0], x[1], x[2], W[0], W[1], h, ikp=c["ikp"], kp=c["kp"], seed=SEED)
    torch.cuda.synchronize()
    return h.cpu().numpy()


def reference(c, dtype, h):
    """(ref, bounds) of the case in `dtype` with the fp32 head, on the hidden rows h."""
    W_enc, b_enc, W_dec, b_dec = c["W"]
    kw = dict(n_batch=c["n_batch"], tied=c["tied"], reg_lambda=c["lam"], input_keep_mask=c["im"], ikp=c["ikp"],
              hidden_keep_mask=c["hm"], kp=c["kp"], h=h)
    Wd = W_enc if c["tied"] else W_dec
    if dtype == F32:
        ref = dn.grads_f32(c["x"], c["y"], W_enc, b_enc, Wd, b_dec, **kw)
        return ref, dn.f32_bounds(ref)
    ref = dn.grads_bf16(c["x"], c["y"], W_enc, b_enc, Wd, b_dec, head="fp32", **kw)
    return ref, dn.bf16_bounds(ref)


def row_intervals(bounds, V):
    w = (V + 2) * dn.U32 * np.maximum(np.abs(bounds["L_lo"]), np.abs(bounds["L_hi"])).sum(axis=1)
    return bounds["L_lo"].sum(axis=1) - w, bounds["L_hi"].sum(axis=1) + w


def check_against_reference(cost, rows, c, ref, bounds, what=""):
    lo, hi = dn.cost_interval(ref, bounds)
    print("%s cost %.9g in [%.9g, %.9g]" % (what, cost, lo, hi))
    assert np.isfinite(cost) and lo <= cost <= hi, (what, cost, lo, hi)
    rlo, rhi = row_intervals(bounds, c["V"])
    assert rows.shape == (c["B"],) and np.isfinite(rows).all(), what
    half = np.maximum(0.5 * (rhi - rlo), 1e-300)
    off = np.abs(rows - 0.5 * (rhi + rlo)) / half
    print("%s rows: worst |row - mid| / half-width %.4f" % (what, float(off.max())))
    bad = np.flatnonzero((rows < rlo) | (rows > rhi))
    assert bad.size == 0, (what, [(int(r), float(rows[r]), float(rlo[r]), float(rhi[r])) for r in bad[:8]])


def run_and_check(c, dtype, what=""):
    ctx = _lib.Context(0)
    try:
        h = gpu_hidden(ctx, c)
        cost, rows = score_loss(ctx, c, dtype)
    finally:
        ctx.close()
    ref, bounds = reference(c, dtype, h)
    check_against_reference(cost, rows, c, ref, bounds, what)
    return cost, rows, ref, bounds


# ---- against the rounding-aware reference ------------------------------------------------------------------------------------------
SHAPES = [
    # V, nt, H, B, options
    (31, 20, 256, 3, dict()),                                        # less than a tile, less than a wave's rows
    (33, 20, 256, 256, dict()),                                      # the second tile holds one column
    (900, 700, 32, 10, dict(lam=0.01)),
    (1500, 1200, 64, 64, dict(tied=True)),
    (3000, 2400, 128, 37, dict()),
    (3000, 2500, 96, 130, dict()),                                   # two row groups, the second nearly empty
    (2100, 2000, 256, 250, dict(tied=True, lam=0.02, ikp=0.75, kp=0.8)),
    (640, 500, 64, 4096, dict()),                                    # many row groups
    (20000, 16000, 256, 288, dict()),                                # more tiles than workgroups, more than one row group
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V,nt,H,B,opt", SHAPES, ids=["%dx%dx%dx%d" % s[:4] for s in SHAPES])
def test_cost_and_rows_inside_the_reference_intervals(V, nt, H, B, opt, dtype):
    run_and_check(make_case(V, nt, H, B, **opt), dtype)


# ---- the positives ------------------------------------------------------------------------------------------------------------------
PV, PNT, PH, PB = 3000, 2400, 64, 8          # V % 32 == 24: column V - 1 sits in a partial last tile
ROW_EMPTY, ROW_LONG, ROW_WEIGHTS, ROW_LAST, ROW_ARTISTS = 0, 1, 2, 3, 4


def _positives_case(all_empty=False):
    base = make_case(PV, PNT, PH, PB)
    x, y = base["x"].copy(), base["y"].copy()
    rng = np.random.default_rng(11)
    y[ROW_EMPTY] = 0.0
    y[ROW_LONG] = 0.0
    y[ROW_LONG, rng.choice(PV, 1300, replace=False)] = 1.0
    y[ROW_WEIGHTS] = 0.0
    cols = rng.choice(PV, 30, replace=False)
    y[ROW_WEIGHTS, cols[0::3]] = 0.15
    y[ROW_WEIGHTS, cols[1::3]] = 0.5
    y[ROW_WEIGHTS, cols[2::3]] = 1.0
    y[ROW_LAST] = 0.0
    y[ROW_LAST, PV - 1] = 1.0
    y[ROW_ARTISTS] = 0.0
    y[ROW_ARTISTS, rng.choice(np.arange(PNT, PV), 12, replace=False)] = 1.0
    if all_empty:
        y[:] = 0.0
    return make_case(PV, PNT, PH, PB, feed=(x, y))


@functools.lru_cache(maxsize=None)
def _positives(dtype, all_empty):
    c = _positives_case(all_empty)
    cost, rows, ref, bounds = run_and_check(c, dtype, "positives")
    rows.setflags(write=False)
    return c, cost, rows, bounds


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row,n_targets", [(ROW_LONG, 1300), (ROW_WEIGHTS, 30), (ROW_LAST, 1), (ROW_ARTISTS, 12)],
                         ids=["1300-targets", "weights", "column-V-1", "artists-only"])
def test_rows_of_positives(row, n_targets, dtype):
    """A row of 1 300 targets, weights 0.15 / 0.5 / 1.0, the one target in column V - 1 of a partial tile, artist targets
    only: inside the row's interval (checked for every row of the case), and not what the row costs without its targets."""
    c, _cost, rows, bounds = _positives(dtype, False)
    assert int((c["y"][row] != 0).sum()) == n_targets
    rlo, rhi = row_intervals(bounds, c["V"])
    assert rlo[row] <= rows[row] <= rhi[row]
    _c0, _cost0, rows0, _b0 = _positives(dtype, True)
    assert rows[row] != rows0[row]


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_target_rows(dtype):
    """All rows empty: the negatives alone, inside the intervals.  An empty row of a batch with targets: the same bits."""
    _c, _cost, rows, _bounds = _positives(dtype, False)
    _c0, cost0, rows0, _b0 = _positives(dtype, True)
    assert rows[ROW_EMPTY].tobytes() == rows0[ROW_EMPTY].tobytes()
    assert (rows0 > 0).all() and cost0 > 0


# ---- one saturated case ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_saturated_logits(dtype):
    """Planted columns as in tests/test_gpu_train_saturated.py (logits to 20 as negatives and as targets): the fp32 head's
    intervals hold; the float64 head's value is printed beside them."""
    c = planted_case(2003, 1600, 256, 65, dict())
    cost, _rows, ref, _bounds = run_and_check(c, dtype, "saturated")
    assert float(ref["_aux"]["z"].max()) > 13.0
    W_enc, b_enc, W_dec, b_dec = c["W"]
    r64 = dn.grads(c["x"], c["y"], W_enc, b_enc, W_dec, b_dec, n_batch=c["n_batch"], tied=False)
    print("float64 head: cost %.9g, the call's off it by %.3g relative" % (r64["cost"], abs(cost - r64["cost"]) / r64["cost"]))


# ---- against the step ------------------------------------------------------------------------------------------------------------------
STEP_CASES = [(2100, 2000, 256, 250, dict(tied=True, lam=0.02, ikp=0.75, kp=0.8)), (3000, 2400, 128, 37, dict(lam=0.01, kp=0.8))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V,nt,H,B,opt", STEP_CASES, ids=["tied-256", "untied-128"])
def test_cost_against_the_step(V, nt, H, B, opt, dtype):
    c = make_case(V, nt, H, B, **opt)
    ctx = _lib.Context(0)
    try:
        h = gpu_hidden(ctx, c)
        cost, rows = score_loss(ctx, c, dtype)
        step = run_step(ctx, c, dtype)
    finally:
        ctx.close()
    ref, bounds = reference(c, dtype, h)
    lo, hi = dn.cost_interval(ref, bounds)
    print("loss %.9g, step %.9g in [%.9g, %.9g]" % (cost, step["cost"], lo, hi))
    assert lo <= cost <= hi and lo <= step["cost"] <= hi
    # the cost from the rows, on the host in float64
    W_enc, b_enc, W_dec, b_dec = c["W"]
    l2 = 0.5 * sum(float((np.asarray(t, np.float64) ** 2).sum()) for t in ((W_enc, b_dec, b_enc) + (() if c["tied"] else (W_dec,))))
    host = rows.astype(np.float64).sum() / c["n_batch"] + np.float64(np.float32(c["lam"])) * l2
    assert abs(cost - host) <= np.spacing(np.float32(abs(host))), (cost, host)


# ---- what the call leaves alone -------------------------------------------------------------------------------------------------------
def test_calls_repeat_their_bits_and_leave_the_context_alone():
    import torch
    a = make_case(3000, 2400, 128, 37, lam=0.01, ikp=0.75, kp=0.8)
    b = make_case(20000, 16000, 256, 288)
    ctx = _lib.Context(0)
    try:
        for dtype in (F32, BF16):
            ta = _tensors(a)
            before = [t.clone() for t in ta[2]]
            first = score_loss(ctx, a, dtype, tensors=ta)
            again = score_loss(ctx, a, dtype, tensors=ta, prepack=False)
            assert first[0] == again[0] and first[1].tobytes() == again[1].tobytes()
            score_loss(ctx, b, dtype)                              # another shape: scratch regrown, another image
            third = score_loss(ctx, a, dtype, tensors=ta)
            assert first[0] == third[0] and first[1].tobytes() == third[1].tobytes()
            for t0, t1 in zip(before, ta[2]):
                assert torch.equal(t0, t1)
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_ranking_before_and_after_returns_the_same_lists(dtype):
    import torch
    c = make_case(3000, 2400, 128, 37)
    x, y, W = _tensors(c)
    k = 50
    ctx = _lib.Context(0)
    try:
        _prepack(ctx, c, W, dtype)
        srp, sc = ctx.seeds_from_csr(x[0], x[1], 2400)

        def rank():
            score = torch.empty((c["B"], k), device="cuda")
            idx = torch.empty((c["B"], k), dtype=torch.int32, device="cuda")
            ctx.score_topk(x[0], x[1], x[2], W[0], W[1], 2400, srp, sc, k, score, idx, dtype=dtype)
            torch.cuda.synchronize()
            return score.cpu().numpy(), idx.cpu().numpy()
        s0, i0 = rank()
        score_loss(ctx, c, dtype, prepack=False, tensors=(x, y, W))
        s1, i1 = rank()
        assert (i0 == i1).all() and s0.tobytes() == s1.tobytes()
    finally:
        ctx.close()


def test_armed_decoder_adam_survives_the_loss():
    """An armed decoder Adam pending: the next step's outputs equal those of a twin context that never called the loss.
    The rows' inputs share no column: the step's encoder scatter adds with float atomics, so two rows on one column give
    gW_enc bits that differ between any two runs of the step itself."""
    import torch
    base = make_case(2000, 1600, 128, 37, kp=0.8)
    x = np.zeros_like(base["x"])
    for r in range(37):
        x[r, 40 * r:40 * r + 3 + r % 5] = 1.0
    c = make_case(2000, 1600, 128, 37, kp=0.8, feed=(x, base["y"]))
    P = _lib._ptr

    def run(with_loss):
        x, y, W = _tensors(c)
        m, v = torch.zeros_like(W[2]), torch.zeros_like(W[2])
        out = dict(gWe=torch.zeros_like(W[0]), gbe=torch.zeros_like(W[1]), gbd=torch.zeros_like(W[3]), cost=torch.zeros(1, device="cuda"))
        ctx = _lib.Context(0)
        try:
            _prepack(ctx, c, W, F32)
            ctx.check(ctx.lib.dae_arm_decoder_adam(ctx.h, P(m), P(v), 0.005, 0.9, 0.999, 1e-8, 1))
            if with_loss:
                keep = [t.clone() for t in W + [m, v]]
                score_loss(ctx, c, F32, prepack=False, tensors=(x, y, W))
                assert all(torch.equal(a, b) for a, b in zip(keep, W + [m, v]))
            ctx.check(ctx.lib.dae_train_forward_backward(
                ctx.h, P(x[0]), P(x[1]), P(x[2]), P(y[0]), P(y[1]), P(y[2]), P(W[0]), P(W[1]), P(W[2]), P(W[3]),
                c["V"], c["H"], c["B"], c["n_batch"], 0, float(c["ikp"]), float(c["kp"]), SEED, 0.0,
                P(out["gWe"]), P(out["gbe"]), None, P(out["gbd"]), P(out["cost"])))
            torch.cuda.synchronize()
        finally:
            ctx.close()
        return [t.cpu().numpy() for t in (W[2], m, v, out["gWe"], out["gbe"], out["gbd"], out["cost"])]
    plain, lossy = run(False), run(True)
    assert np.abs(plain[1]).max() > 0 and np.abs(plain[3]).max() > 0      # the armed update really ran; gW_enc is there
    for name, p, q in zip(("W_dec", "m", "v", "gW_enc", "gb_enc", "gb_dec", "cost"), plain, lossy):
        assert p.tobytes() == q.tobytes(), name


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
def test_arguments():
    import torch
    c = make_case(900, 700, 32, 10)
    x, y, W = _tensors(c)
    P = _lib._ptr
    rows, cost = torch.zeros(c["B"], device="cuda"), torch.zeros(1, device="cuda")
    ctx = _lib.Context(0)

    def call(B=c["B"], H=c["H"], V=c["V"], r=rows, co=cost, Wt=W):
        return ctx.lib.dae_score_loss(ctx.h, P(x[0]), P(x[1]), P(x[2]), P(y[0]), P(y[1]), P(y[2]), P(Wt[0]), P(Wt[1]), P(Wt[2]),
                                      P(Wt[3]), V, H, B, c["n_batch"], 0, 1.0, 1.0, SEED, 0.0, P(r), P(co))
    try:
        assert call() == ERR_STATE                                 # no image yet
        ctx.prepack_decoder(W[2], W[3], 0, c["V"], BF16)
        assert call() == ERR_STATE                                 # an image of the other dtype
        ctx.prepack_decoder(W[2], W[3], 0, 512, F32)
        assert call() == ERR_STATE                                 # an image that does not cover [0, V)
        assert b"[0, 900)" in ctx.lib.dae_last_error(ctx.h)
        ctx.prepack_decoder(W[2], W[3], 0, c["V"], F32)
        assert call() == 0
        assert call(r=None, co=None) == ERR_ARG
        assert call(B=0) == ERR_ARG
        big = [torch.zeros((40, 1056), device="cuda"), torch.zeros(1056, device="cuda"), torch.zeros((40, 1056), device="cuda"),
               torch.zeros(40, device="cuda")]
        assert call(H=48) == ERR_ARG and call(H=1056, V=40, Wt=big) == ERR_ARG
        h = torch.zeros((c["B"], c["H"]), device="cuda")

        def rows_call(B=c["B"], H=c["H"], dtype=F32):
            return ctx.lib.dae_decode_loss_rows(ctx.h, P(h), B, H, dtype, P(y[0]), P(y[1]), P(y[2]), P(W[2]), P(W[3]), c["V"], P(rows))
        assert rows_call() == 0
        assert rows_call(B=0) == ERR_ARG and rows_call(H=48) == ERR_ARG and rows_call(H=1056) == ERR_ARG
        assert rows_call(dtype=BF16) == 0                          # (the bf16 image of the whole vocabulary is still there)
        assert rows_call(dtype=_lib.DAE_DTYPE_BF16_EXACT) == ERR_ARG
        torch.cuda.synchronize()
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_either_output_may_be_null_and_the_rows_call_agrees(dtype):
    import torch
    c = make_case(3000, 2400, 128, 37, lam=0.01)
    ctx = _lib.Context(0)
    try:
        cost, rows = score_loss(ctx, c, dtype)
        cost_only, none = score_loss(ctx, c, dtype, want_rows=False)
        none2, rows_only = score_loss(ctx, c, dtype, want_cost=False)
        assert none is None and none2 is None and cost_only == cost and rows_only.tobytes() == rows.tobytes()
        # dae_decode_loss_rows on the same hidden rows: the same row losses
        x, y, W = _tensors(c)
        h = torch.empty((c["B"], c["H"]), device="cuda")
        ctx.encode(x[0], x[1], x[2], W[0], W[1], h)
        out = torch.empty(c["B"], device="cuda")
        ctx.decode_loss_rows(h, y, W[2], W[3], out, dtype=dtype)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == rows.tobytes()
    finally:
        ctx.close()


# ---- model ---------------------------------------------------------------------------------------------------------------------------
class _Conf:
    def __init__(self, **kw):
        self.save, self.initval = "unused", "NULL"
        self.batch, self.n_input, self.hidden, self.lr, self.reg_lambda = 16, 900, 128, 0.005, 0.0
        self.n_tracks = 700
        self.__dict__.update(kw)


def _feed(model, seed=3):
    from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists
    pos, ones, _ = make_playlists(model.n_batch, model.n_tracks, model.n_input - model.n_tracks, seed=seed, seed_counts=(3, 9, 20))
    xm = pos[:, 1] < model.n_tracks
    return pos[xm], ones[xm], pos, np.ones(len(pos), np.float32)


def _model(cls=None, **kw):
    from spotify_recsys_challenge_2018_amd.models.DAEs import DAE
    m = (cls or DAE)(_Conf(**kw))
    m.fit()
    return m


def _c_call(params, feed, n_batch, tied, dtype=F32, ikp=1.0, kp=1.0, seed=0, lam=0.0):
    """dae_score_loss on host parameter arrays in a fresh context -> (cost, rows)."""
    import torch
    from spotify_recsys_challenge_2018_amd.models.DAEs import coo_to_csr
    V = params[0].shape[0]
    x = [_dev(a if a.size else np.zeros(1, a.dtype)) for a in coo_to_csr(feed[0], feed[1], n_batch, V)]
    y = [_dev(a if a.size else np.zeros(1, a.dtype)) for a in coo_to_csr(feed[2], feed[3], n_batch, V)]
    W = [_dev(np.ascontiguousarray(p, np.float32)) for p in params]
    rows, cost = torch.empty(n_batch, device="cuda"), torch.empty(1, device="cuda")
    ctx = _lib.Context(0)
    try:
        ctx.set_train_dtype(dtype)
        ctx.prepack_decoder(W[0] if tied else W[1], W[3], 0, V, dtype)
        ctx.score_loss(x, y, W[0], W[2], None if tied else W[1], W[3], n_batch, tied, ikp=ikp, kp=kp, seed=seed, reg_lambda=lam,
                       row_loss=rows, cost_out=cost)
        torch.cuda.synchronize()
    finally:
        ctx.close()
    return float(cost.item()), rows.cpu().numpy()


def test_model_loss_equals_the_c_call_and_session_run():
    from spotify_recsys_challenge_2018_amd.models.DAEs import DAE_tied, Session
    m = _model(DAE_tied, reg_lambda=0.01)
    feed = _feed(m)
    cost, rows = m.loss(*feed, keep_prob=0.8, input_keep_prob=0.75, seed=77, per_row=True)
    c_cost, c_rows = _c_call(m.get_params(), feed, m.n_batch, True, ikp=0.75, kp=0.8, seed=77, lam=0.01)
    assert cost == c_cost and rows.tobytes() == c_rows.tobytes() and rows.dtype == np.float32 and rows.shape == (m.n_batch,)
    assert m.loss(*feed, keep_prob=0.8, input_keep_prob=0.75, seed=77) == cost
    with pytest.raises(ValueError, match="seed"):
        m.loss(*feed, keep_prob=0.8)
    sess = Session(m)
    fd = {m.x_positions: feed[0], m.x_ones: feed[1], m.y_positions: feed[2], m.y_ones: feed[3]}
    plain = m.loss(*feed)
    assert sess.run(m.cost, feed_dict=fd) == plain and sess.run([m.cost], feed_dict=fd) == [plain]
    fd.update({m.keep_prob: 0.8, m.input_keep_prob: 0.75})
    dropped = sess.run(m.cost, feed_dict=fd)                       # the feed's keep probabilities, a seed of the session's own
    assert np.isfinite(dropped) and dropped != plain


def test_model_loss_after_steps_of_the_rows_adam_equals_the_c_call_on_the_parameters():
    m = _model()                                                   # untied, lambda 0: rows Adam, the fused decoder Adam
    for s in range(3):
        f = _feed(m, seed=10 + s)
        m.train_step(*f, 0.8, 0.75)
    assert m._lazy is not None
    feed = _feed(m, seed=20)
    cost, rows = m.loss(*feed, per_row=True)
    c_cost, c_rows = _c_call(m.get_params(), feed, m.n_batch, False)
    assert cost == c_cost and rows.tobytes() == c_rows.tobytes()


def _disjoint_feed(model, step):
    """A training feed whose rows share no input column (40 track columns to a row): the step's encoder scatter adds with
    float atomics, so only such a feed trains the same bits twice, with or without anything in between."""
    rng = np.random.default_rng(step)
    x = [(r, 40 * r + int(c)) for r in range(model.n_batch) for c in rng.choice(40, 3 + (r + step) % 5, replace=False)]
    y = x + [(r, model.n_tracks + int(c)) for r in range(model.n_batch) for c in rng.choice(model.n_input - model.n_tracks, 2, replace=False)]
    return np.array(x, np.int64), np.ones(len(x), np.float32), np.array(sorted(y), np.int64), np.ones(len(y), np.float32)


def test_loss_between_steps_never_changes_a_training_run():
    from spotify_recsys_challenge_2018_amd.models.DAEs import Session
    plain, probed = _model(), _model()
    sess = Session(probed)
    costs = [[], []]
    for s in range(5):
        f = _disjoint_feed(plain, s)
        costs[0].append(plain.train_step(*f, 0.8, 0.75))
        costs[1].append(probed.train_step(*f, 0.8, 0.75))
        held = _feed(probed, seed=40 + s)
        probed.loss(*held)
        probed.loss(*held, keep_prob=0.8, seed=5)
        sess.run(probed.cost, feed_dict={probed.x_positions: held[0], probed.x_ones: held[1], probed.y_positions: held[2],
                                         probed.y_ones: held[3], probed.keep_prob: 0.8})
    assert costs[0] == costs[1]
    for p, q in zip(plain.get_params(), probed.get_params()):
        assert p.tobytes() == q.tobytes()


def test_driver_logs_the_heldout_loss_of_every_split(tmp_path):
    """main.py on the golden data with [BASE] eval_loss = on: a training run (--pretrain) logs one more line per split behind
    the existing ones, every epoch; --dae --testmode logs them behind the lines of the same run without the key, which stay
    as they are, and leaves the saved parameters byte for byte.  (Two training runs of the driver are not compared: rows of
    the real data share input columns, and the step's encoder scatter adds them with float atomics, so two identical runs
    differ in last bits with or without the key -- that a call between steps changes nothing is
    test_loss_between_steps_never_changes_a_training_run's.)"""
    from spotify_recsys_challenge_2018_amd import main as cli
    G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    work = tmp_path / "run"
    work.mkdir()
    shutil.copytree(os.path.join(G, "data"), tmp_path / "data")
    ini = open(os.path.join(G, "config.ini")).read()
    splits = ("test-0", "test-1", "test-5", "test-25r")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        def run(key, *args):
            open(work / "config.ini", "w").write(ini.replace("[BASE]", "[BASE]\n" + key))
            n0 = len(open(work / "log.txt").read().splitlines()) if os.path.exists(work / "log.txt") else 0
            random.seed(0); np.random.seed(0)
            assert cli.main(["--dir", "run", *args]) == 0
            return [l for l in open(work / "log.txt").read().splitlines()[n0:] if l.startswith("seed num")]

        def check_loss_lines(lines):
            assert len(lines) == 4
            for l, s in zip(lines, splits):
                assert l.startswith("seed num: %s heldout loss: " % s), l
                assert 0.0 < float(l.split()[-1]) < 1e6
        full = run("eval_loss = on", "--pretrain")
        assert len(full) == 16                                      # two epochs of four existing lines and four new ones
        for e in range(2):
            assert all(" rprecision: " in l for l in full[8 * e:8 * e + 4])
            check_loss_lines(full[8 * e + 4:8 * e + 8])
        assert run("", "--dae") and os.path.exists(work / "w_dae")
        saved = open(work / "w_dae", "rb").read()
        plain = run("", "--dae", "--testmode")
        keyed = run("eval_loss = on", "--dae", "--testmode")
        assert len(plain) == 4 and keyed[:4] == plain and run("eval_loss = off", "--dae", "--testmode") == plain
        check_loss_lines(keyed[4:])
        assert open(work / "w_dae", "rb").read() == saved
        assert len(pickle.load(open(work / "w_dae", "rb"))) == 4
    finally:
        os.chdir(cwd)
