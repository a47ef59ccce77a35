"""GPU (-m gpu): the held-out loss under the title mix (dae_mix_loss_rows = dae_decode_mix_term + decode_f32_kernel's EPI_MIXROWLOSS +
mix_loss_finish_kernel, DAE_title.mixed_loss, [BASE] eval_mixed_loss).

The reference is rounding-aware and built from the GPU's own dense route: z = the title context's decode_dense(feat) (logits),
dae = the DAE context's decode_dense(h, sigmoid), (w_t, w_p) = dae_mix_weights; hd = oracle/title_numpy.py fp32_loss_head(z, dae,
y_dense, ...) and hd0 the same with y = 0.  With U = 2^-24, n_t a row's target count and
    M_r = sum_v max(|hd0.L_lo|, |hd0.L_hi|) + sum_targets (max|hd0.L| + max|hd.L|),
every row must lie in [sum_v hd.L_lo - w_r, sum_v hd.L_hi + w_r], w_r = (V + 2 n_t + 2) U M_r: the summation term of the saturated
step test, (n + 2) U sum|L|, over the terms this path really adds (V negatives, then per target one term out and one in).  The
cost must lie in the rows' intervals summed and divided by n_batch, and equal float32(sum of the rows in float64 / n_batch) to
one fp32 ulp.

fp32_loss_head asserts w_t + w_p <= 1 in float64.  The fp32 quotients u / d and x / d of most row sums x round to a pair that
exceeds 1 by a few 2^-26 (1/3 and 2/3 both round up), so the feeds here give rows with a title in use an input of a length
whose two fp32 weights do satisfy it (`_good_lengths`: 1, 3, 5, 7, 9, 13, ...; any length without a title, where w_p = 1) -- the
inputs are chosen for the reference, never the bound for the result."""
import copy
import os
import pickle

import numpy as np
import pytest

from oracle import title_numpy as tn
from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.models.DAEs import DAE_title, coo_to_csr
from spotify_recsys_challenge_2018_amd.models.title_models import get_model
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_weights
from test_train_saturated_reference_cpu import LOGITS, TITLE_W

pytestmark = pytest.mark.gpu
F32 = _lib.DAE_DTYPE_F32
U = 2.0 ** -24
V, NT = 2003, 1600                      # an edge tile (2003 = 62 x 32 + 19) and artist columns
N_CHAR, L = 41, 25
BS = (1, 33, 96, 150, 256, 300)         # partial row groups at 64-row groups; 300 = two panels


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _good_lengths(limit=120):
    """Row sums x whose fp32 mixing weights 1 / (1 + x) and x / (1 + x) add up to at most 1 in float64 (the oracle's premise)."""
    f = np.float32
    out = []
    for n in range(1, limit):
        d = f(1) + f(n) + f(1e-10)
        if float(f(f(1) / d)) + float(f(f(n) / d)) <= 1.0:
            out.append(n)
    return out


GOOD = _good_lengths()


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def _intervals(z, dae, y_dense, w_t, w_p, n_batch):
    """-> dict(lo, hi [B]: the rows' intervals, w_r included; cost_lo, cost_hi; zero: elements with q = 0 admissible)."""
    z, dae = np.asarray(z, np.float32), np.asarray(dae, np.float32)
    hd = tn.fp32_loss_head(z, dae, y_dense, w_t, w_p, n_batch)
    hd0 = tn.fp32_loss_head(z, dae, np.zeros_like(y_dense), w_t, w_p, n_batch)
    a0 = np.maximum(np.abs(hd0["L_lo"]), np.abs(hd0["L_hi"]))
    a1 = np.maximum(np.abs(hd["L_lo"]), np.abs(hd["L_hi"]))
    tgt = y_dense != 0
    n_t = tgt.sum(axis=1)
    M = a0.sum(axis=1) + ((a0 + a1) * tgt).sum(axis=1)
    w = (z.shape[1] + 2 * n_t + 2) * U * M
    lo, hi = hd["L_lo"].sum(axis=1) - w, hd["L_hi"].sum(axis=1) + w
    return dict(lo=lo, hi=hi, cost_lo=lo.sum() / n_batch, cost_hi=hi.sum() / n_batch, zero=hd["zero"], hd=hd, hd0=hd0)


def _check(rows, cost, iv, n_batch, what=""):
    rows = np.asarray(rows, np.float64)
    assert np.isfinite(rows).all() and np.isfinite(cost), what
    inside = (iv["lo"] <= rows) & (rows <= iv["hi"])
    width = iv["hi"] - iv["lo"]
    print("%s rows %d, outside %d, widest interval %.3g of a row loss %.6g; cost %.9g in [%.9g, %.9g]"
          % (what, rows.size, (~inside).sum(), width.max(), rows[np.argmax(width)], cost, iv["cost_lo"], iv["cost_hi"]))
    assert inside.all(), [(int(r), rows[r], iv["lo"][r], iv["hi"][r]) for r in np.flatnonzero(~inside)[:6]]
    assert iv["cost_lo"] <= cost <= iv["cost_hi"]
    want = np.float32(rows.sum() / n_batch)
    assert abs(float(np.float32(cost)) - float(want)) <= float(np.spacing(np.abs(want))), (cost, want)


def _y_dense(ypos, yval, B):
    y = np.zeros((B, V), np.float64)
    if len(ypos):
        y[ypos[:, 0], ypos[:, 1]] = yval
    return y


# ---- feeds -------------------------------------------------------------------------------------------------------------------------
def _feed(B, seed, all_untitled=False):
    """x: row r has a title in use and an input of a GOOD length, but rows r % 4 == 3 (no title: any length), row 1 (a title, no
    input: w_playlist = 0) and row 2 (neither: yp = 0).  y: the input's columns and some more, and row 0 targets at column 0,
    V - 1 and an artist column with fractional values, row 4 none, row 5 one, row 6 three hundred."""
    rng = np.random.default_rng(seed)
    use = np.ones(B, np.float32)
    use[3::4] = 0
    if B > 2:
        use[2] = 0
    if all_untitled:
        use[:] = 0
    xpos, ypos, yval = [], [], []
    for r in range(B):
        n = int(rng.integers(1, 90)) if use[r] == 0 else GOOD[int(rng.integers(0, 24))]
        if B > 2 and r in (1, 2):
            n = 0
        cols = np.sort(np.concatenate([rng.choice(NT, n - n // 3, replace=False), NT + rng.choice(V - NT, n // 3, replace=False)]))
        xpos += [(r, int(c)) for c in cols]
        t = np.union1d(cols, rng.choice(V, int(rng.integers(0, 30)), replace=False))
        v = np.ones(t.size, np.float32)
        if r == 0:
            t = np.union1d(t, [0, V - 1, NT + 5])
            v = np.ones(t.size, np.float32)
            v[[0, -1]] = (0.25, 0.625)
            v[np.searchsorted(t, NT + 5)] = 0.5
        if B > 6 and r == 4:
            t, v = t[:0], v[:0]
        if B > 6 and r == 5:
            t, v = t[:1], v[:1]
        if B > 6 and r == 6:
            t = np.sort(rng.choice(V, 300, replace=False))
            v = np.ones(300, np.float32)
        ypos += [(r, int(c)) for c in t]
        yval += v.tolist()
    titles = rng.integers(0, N_CHAR, (B, L))
    for r in range(B):
        titles[r, int(rng.integers(1, L + 1)):] = -1
        if use[r] == 0:
            titles[r] = -1
    as_pos = lambda p: np.asarray(p, np.int64).reshape(-1, 2)
    xpos = as_pos(xpos)
    return dict(B=B, xpos=xpos, xones=np.ones(len(xpos), np.float32), ypos=as_pos(ypos), yval=np.asarray(yval, np.float32),
                titles=titles, use=use)


# ---- models ------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("mixed_loss")


def _model(workdir, H, fnum, B, fresh=False, sizes=(3, 5), n_char=N_CHAR):
    """DAE_title over V columns: DAE hidden H, a title scorer of len(sizes) * fnum features (ld_feat = that rounded up to 64)."""
    key = (H, fnum, B, tuple(sizes), n_char)
    if key in _MODELS and not fresh:
        return _MODELS[key]

    class Conf:
        lr = 0.01; reg_lambda = 0.0; char_model = 'Char_CNN'; save = "/tmp/_mixedloss_unused"; initval = "NULL"; title_lr = 0.002
        n_input = V; n_output = V; n_tracks = NT; char_emb = 25; strmaxlen = L; decode_dtype = "f32"
    c = Conf()
    c.batch, c.hidden, c.filter_size, c.filter_num, c.charsize = B, H, list(sizes), fnum, n_char
    pk = os.path.join(str(workdir), "w_dae_%d" % H)
    if not os.path.exists(pk):
        W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=H, bias="zipf", n_tracks=NT)
        with open(pk, "wb") as f:
            pickle.dump([W_enc, W_dec, b_enc, b_dec], f)
    c.DAEval = pk
    mt = get_model(c)
    mt.fit(tn.make_params(n_char, 25, list(sizes), fnum, V, seed=4))
    m = DAE_title(c, mt)
    m.fit()
    if not fresh:
        _MODELS[key] = m
    return m


def _dense_route(m, f, kp=1.0, ikp=1.0, tkp=1.0, seed=0):
    """The GPU's own dense route of the feed -> (z, dae, w_t, w_p) on the host, and the device tensors (h, feat, w_t, w_p)."""
    import torch
    tm, B = m.title_model, f["B"]
    assert B == m.n_batch
    h = m.encode(f["xpos"], f["xones"], kp, ikp, seed)
    m._ensure_packed(F32)
    dae = torch.empty((B, V), dtype=torch.float32, device=h.device)
    m.ctx.decode_dense(h, dae, apply_sigmoid=True)
    tm._ensure_packed(F32, features_table=tkp == 1.0)
    feat = tm.features(f["titles"], B, tkp, seed)
    z = torch.empty((B, V), dtype=torch.float32, device=h.device)
    tm.ctx.decode_dense(feat, z, apply_sigmoid=False)
    csr = m._upload_csr(f["xpos"], f["xones"])
    w_t, w_p = m._mix_weights(csr, f["use"], ikp, seed)
    return (z.cpu().numpy(), dae.cpu().numpy(), w_t.cpu().numpy(), w_p.cpu().numpy()), (h, feat, w_t, w_p)


def _reference(m, f, **kw):
    (z, dae, w_t, w_p), dev = _dense_route(m, f, **kw)
    return _intervals(z, dae, _y_dense(f["ypos"], f["yval"], f["B"]), w_t, w_p, m.n_batch), (w_t, w_p), dev


def _loss(m, f, **kw):
    return m.mixed_loss(f["xpos"], f["xones"], f["ypos"], f["yval"], f["titles"], f["use"], per_row=True, **kw)


# ---- 1. the reference at the issue's shapes, 2. positives, 3. mix corners -------------------------------------------------------
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("H,fnum", [(256, 200), (256, 25), (128, 200), (128, 25)])       # ld_feat 448 and 64
def test_rows_and_cost_lie_in_the_reference_intervals(workdir, H, fnum, B):
    m = _model(workdir, H, fnum, B)
    assert m.title_model.ld == (448 if fnum == 200 else 64)
    f = _feed(B, seed=B + H + fnum)
    iv, (w_t, w_p), _dev_t = _reference(m, f)
    if B > 2:
        assert w_p[1] == 0 and w_t[1] == 1 and w_p[2] == 0 and w_t[2] == 0 and w_t[3] == 0 and w_p[3] == 1     # the corners
    cost, rows = _loss(m, f)
    assert rows.dtype == np.float32 and rows.shape == (B,)
    _check(rows, cost, iv, B, "H=%d ld=%d B=%d:" % (H, m.title_model.ld, B))
    assert m.mixed_loss(f["xpos"], f["xones"], f["ypos"], f["yval"], f["titles"], f["use"]) == cost
    # the positives count: no row with targets is what the row costs without them; the row without targets is
    cost0, rows0 = m.mixed_loss(f["xpos"], f["xones"], np.zeros((0, 2), np.int64), np.zeros(0, np.float32), f["titles"], f["use"],
                                per_row=True)
    n_t = np.bincount(f["ypos"][:, 0], minlength=B)
    assert (_bits(rows)[n_t == 0] == _bits(rows0)[n_t == 0]).all()          # an empty row: the same bits alone and beside targets
    assert (rows[n_t > 0] != rows0[n_t > 0]).all()
    if B > 6:
        assert n_t[4] == 0 and n_t[5] == 1 and n_t[6] == 300
        assert rows0[2] == 0.0 and (n_t[2] == 0 or rows[2] > 0)             # yp = 0: every negative costs -0.55 ln(1 + 1e-10) = 0


def test_a_whole_batch_without_titles_and_fewer_rows_than_the_batch(workdir):
    B = 96
    m = _model(workdir, 256, 200, B)
    f = _feed(B, seed=5, all_untitled=True)
    iv, (w_t, _w_p), _d = _reference(m, f)
    assert (w_t == 0).all()
    cost, rows = _loss(m, f)
    _check(rows, cost, iv, B, "no titles:")
    # n_rows: the first 40 rows alone -- the same rows, bit for bit; the cost still over n_batch
    keep_x, keep_y = f["xpos"][:, 0] < 40, f["ypos"][:, 0] < 40
    c40, r40 = m.mixed_loss(f["xpos"][keep_x], f["xones"][keep_x], f["ypos"][keep_y], f["yval"][keep_y], f["titles"][:40], f["use"][:40],
                            n_rows=40, per_row=True)
    assert r40.shape == (40,) and (_bits(r40) == _bits(rows[:40])).all()
    assert abs(c40 - np.float32(r40.astype(np.float64).sum() / B)) <= np.spacing(np.float32(c40))


# ---- 4. saturation -------------------------------------------------------------------------------------------------------------------
class Pair:
    """The title scorer's context and the DAE's, on one stream."""

    def __init__(self):
        self.t, self.d = _lib.Context(0), _lib.Context(0)

    def close(self):
        self.t.close()
        self.d.close()


def _abi(pair, t, B, n_batch, csr, rows=True, cost=True, r0=0):
    """dae_mix_loss_rows on the device tensors t = dict(h, Wd, bd, feat, Wt, bt, w_t, w_p) -> (rows, cost) on the host."""
    import torch
    out_r = torch.full((B + 2,), 7.0, dtype=torch.float32, device="cuda") if rows else None
    out_c = torch.full((3,), 7.0, dtype=torch.float32, device="cuda") if cost else None
    pair.t.mix_loss_rows(pair.d, t["h"][r0:r0 + B], t["Wd"], t["bd"], t["feat"][r0:r0 + B], t["Wt"], t["bt"], t["w_t"][r0:r0 + B],
                         t["w_p"][r0:r0 + B], n_batch, csr, row_loss=out_r, cost_out=out_c)
    r = out_r.cpu().numpy() if rows else None
    c = out_c.cpu().numpy() if cost else None
    assert r is None or (r[B:] == 7.0).all()              # nothing is written past the outputs
    assert c is None or (c[1:] == 7.0).all()
    return (r[:B] if rows else None), (float(c[0]) if cost else None)


def _saturated_case():
    """After title_case() of the saturated step test, through both GEMMs: Output_W^T = 0 and Output_b[v] = LOGITS[v % 27] put the
    title logit of column v at a planted value in every row; h[r] = the unit vector r // 6 and W_dec[v][k] = LOGITS[(v + k) % 27],
    b_dec = 0 put the DAE's logit at LOGITS[(v + r // 6) % 27] exactly; row r mixes with TITLE_W[r % 6] (sums <= 1, some = 1).
    Targets 0 and 1 alternate, so both meet yp = 1 and yp = 0."""
    B, Vs, H, Fd = 36, 200, 32, 64
    lg = np.asarray(LOGITS, np.float32)
    v, k = np.arange(Vs)[:, None], np.arange(H)[None, :]
    Wd = lg[(v + k) % len(lg)].astype(np.float32)
    h = np.zeros((B, H), np.float32)
    h[np.arange(B), np.arange(B) // len(TITLE_W)] = 1.0
    w = np.asarray(TITLE_W, np.float32)[np.arange(B) % len(TITLE_W)]
    y = ((np.arange(B)[:, None] + np.arange(Vs)[None, :]) % 2).astype(np.float32)
    rng = np.random.default_rng(3)
    t = dict(h=h, Wd=Wd, bd=np.zeros(Vs, np.float32), feat=np.abs(rng.standard_normal((B, Fd))).astype(np.float32),
             Wt=np.zeros((Vs, Fd), np.float32), bt=lg[np.arange(Vs) % len(lg)].copy(), w_t=w[:, 0].copy(), w_p=w[:, 1].copy())
    return B, Vs, t, y


def test_saturated_mixed_scores():
    import torch
    B, Vs, t, y = _saturated_case()
    pair = Pair()
    try:
        d = {k: _dev(a) for k, a in t.items()}
        pair.d.prepack_decoder(d["Wd"], d["bd"], dtype=F32)
        pair.t.prepack_decoder(d["Wt"], d["bt"], dtype=F32)
        z, dae = torch.empty((B, Vs), device="cuda"), torch.empty((B, Vs), device="cuda")
        pair.t.decode_dense(d["feat"], z, apply_sigmoid=False)
        pair.d.decode_dense(d["h"], dae, apply_sigmoid=True)
        z, dae = z.cpu().numpy(), dae.cpu().numpy()
        lg = np.asarray(LOGITS, np.float32)
        assert np.array_equal(z, np.tile(lg[np.arange(Vs) % len(lg)], (B, 1)))          # the planted logits arrive exactly
        nb = 40
        hd = tn.fp32_loss_head(z, dae, y.astype(np.float64), t["w_t"], t["w_p"], nb)
        hd0 = tn.fp32_loss_head(z, dae, np.zeros((B, Vs)), t["w_t"], t["w_p"], nb)
        a0 = np.maximum(np.abs(hd0["L_lo"]), np.abs(hd0["L_hi"]))
        a1 = np.maximum(np.abs(hd["L_lo"]), np.abs(hd["L_hi"]))
        tgt = y != 0
        w = (Vs + 2 * tgt.sum(axis=1) + 2) * U * (a0.sum(axis=1) + ((a0 + a1) * tgt).sum(axis=1))
        iv = dict(lo=hd["L_lo"].sum(axis=1) - w, hi=hd["L_hi"].sum(axis=1) + w)
        iv["cost_lo"], iv["cost_hi"] = iv["lo"].sum() / nb, iv["hi"].sum() / nb
        rp, col, val = coo_to_csr(np.argwhere(tgt), y[tgt], B, Vs)
        rows, cost = _abi(pair, d, B, nb, (_dev(rp), _dev(col), _dev(val)))
    finally:
        pair.close()
    print("saturated: %d elements, %d with q = 0 admissible, %d of them targets" % (y.size, hd["zero"].sum(), (hd["zero"] & tgt).sum()))
    assert hd["zero"].sum() >= 50 and (hd["zero"] & tgt).any() and (hd["zero"] & ~tgt).any()
    _check(rows, cost, iv, nb, "saturated:")


# ---- 5. against the step -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dropout", [False, True])
def test_against_the_training_step(workdir, dropout):
    """mixed_loss first, then train_step on the same batch: both costs lie inside the cost interval of that seed's dense route.
    Under input dropout a row's weights are not ours to choose, so the titled rows hold one input entry (kept: x_count = 1.0f,
    weights 1/2 and 1/2; dropped: w_title = 1) or none; the rows without a title hold any number."""
    B = 96
    m = _model(workdir, 256, 200, B, fresh=True)
    f = _feed(B, seed=11)
    if dropout:
        titled = np.flatnonzero(f["use"] == 1)
        first = np.zeros(len(f["xpos"]), bool)
        first[np.unique(f["xpos"][:, 0], return_index=True)[1]] = True
        keep = ~np.isin(f["xpos"][:, 0], titled) | first
        f["xpos"], f["xones"] = f["xpos"][keep], f["xones"][keep]
    kw = dict(keep_prob=0.8, input_keep_prob=0.75, title_keep_prob=0.9) if dropout else {}
    seed = int(copy.deepcopy(m._rng).randint(0, 2 ** 31 - 1))               # what the step will draw
    ref_kw = dict(kp=0.8, ikp=0.75, tkp=0.9, seed=seed) if dropout else dict(seed=seed)
    iv, (w_t, w_p), _d = _reference(m, f, **ref_kw)
    assert (w_t.astype(np.float64) + w_p.astype(np.float64) <= 1.0).all()
    state = copy.deepcopy(m._rng.get_state())
    cost, rows = _loss(m, f, seed=seed, **kw)
    after = m._rng.get_state()
    assert np.array_equal(state[1], after[1]) and state[2] == after[2]      # nothing drawn from the model's dropout stream
    _check(rows, cost, iv, B, "dropout %s:" % dropout)
    step = m.train_step(f["xpos"], f["xones"], f["ypos"], f["yval"], kw.get("keep_prob", 1.0), kw.get("input_keep_prob", 1.0),
                        titles=f["titles"], titles_use=f["use"], title_keep_prob=kw.get("title_keep_prob", 1.0))
    print("dropout %s: mixed_loss %.9g, the step %.9g, difference %.3g; interval [%.9g, %.9g]"
          % (dropout, cost, step, cost - step, iv["cost_lo"], iv["cost_hi"]))
    assert iv["cost_lo"] <= step <= iv["cost_hi"]
    if dropout:
        with pytest.raises(ValueError, match="seed"):
            _loss(m, f, title_keep_prob=0.9)


def test_weight_pairs_above_one_and_both_sigmoids_saturated(workdir):
    """The rows the interval reference cannot take: a title in use and an input whose fp32 weights 1 / (1 + x) and x / (1 + x)
    add up to 1 + a few 2^-26 in float64 (x = 2, 4, 6, 8, 10, ...: most lengths), on columns where BOTH scorers' sigmoids are 1.0f
    (planted biases of 30), so that yp = fl(fl(w_t) + fl(w_p)) -- which fp32 rounds to exactly 1, never above -- with targets 0
    and 1 there.  Asserted without the oracle: every row and the cost are finite, the cost is float32(sum of the rows / n_batch),
    and it equals the title step's cost on the same batch to the summation term: both add the same fp32 element terms, all
    non-negative, in different orders, each order within (n + 2) U of the exact sum of at most n = V + 2 n_t terms per row."""
    import torch
    B = 96
    m = _model(workdir, 256, 200, B, fresh=True)
    tm = m.title_model
    hot = [0, 7, 640, NT + 5, V - 1]
    tm.p["Output_b"][hot] = 30.0
    m.biases["decoder_b"][hot] = 30.0
    m._mark_dirty()
    tm._packed_dirty = True
    f = _feed(B, seed=29)
    bad = [n for n in range(2, 90) if n not in GOOD]
    rng = np.random.default_rng(31)
    xpos = []
    for r in range(B):
        n = bad[int(rng.integers(0, len(bad)))] if f["use"][r] == 1 else 5
        xpos += [(r, int(c)) for c in np.sort(rng.choice(V, n, replace=False))]
    f["xpos"] = np.asarray(xpos, np.int64)
    f["xones"] = np.ones(len(xpos), np.float32)
    ypos = [(r, c) for r in range(B) for c in (hot[::2] if r % 2 else hot[1::2])]          # targets 1 on some hot columns, 0 on the others
    f["ypos"], f["yval"] = np.asarray(ypos, np.int64), np.ones(len(ypos), np.float32)
    (z, dae, w_t, w_p), _d = _dense_route(m, f)
    titled = f["use"] == 1
    assert (w_t.astype(np.float64) + w_p.astype(np.float64) > 1.0)[titled].all()            # the pairs the oracle's premise excludes
    assert (dae[:, hot] == 1.0).all() and (z[:, hot] > 20).all()
    cost, rows = _loss(m, f)
    assert np.isfinite(rows).all() and np.isfinite(cost) and (rows > 0).all()
    want = np.float32(rows.astype(np.float64).sum() / B)
    assert abs(np.float32(cost) - want) <= np.spacing(want)
    step = m.train_step(f["xpos"], f["xones"], f["ypos"], f["yval"], 1.0, 1.0, titles=f["titles"], titles_use=f["use"])
    tol = 2 * (V + 2 * len(hot) + 2) * U * cost
    print("weights above one: cost %.9g, the step %.9g, difference %.3g (allowed %.3g); largest row %.6g"
          % (cost, step, cost - step, tol, rows.max()))
    assert np.isfinite(step) and abs(cost - step) <= tol


# ---- 6. what it leaves alone ---------------------------------------------------------------------------------------------------------
def _snapshot(m):
    tm = m.title_model
    out = {"p_" + k: v.clone() for k, v in tm.p.items()}
    if tm._adam is not None:
        for k, (a, b) in tm._adam.items():
            out["m_" + k], out["v_" + k] = a.clone(), b.clone()
    for k in ("encoder_h", "decoder_h"):
        out["w_" + k] = m.weights[k].clone()
    return out


def _same(a, b):
    import torch
    return a.keys() == b.keys() and all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def test_it_changes_nothing(workdir):
    B = 33
    m = _model(workdir, 128, 25, B, fresh=True)
    f = _feed(B, seed=17)
    m.train_step(f["xpos"], f["xones"], f["ypos"], f["yval"], 1.0, 1.0, titles=f["titles"], titles_use=f["use"])    # Adam moments exist
    seeds = [sorted(set(f["xpos"][f["xpos"][:, 0] == r, 1].tolist()) & set(range(NT))) for r in range(B)]
    rec0 = m.recommend(f["xpos"], f["xones"], seeds, k=50, titles=f["titles"], titles_use=f["use"])
    # The packed images themselves have no getter in the C interface.  What reads every word of them is a dense decode of all V
    # columns: z of the title image and the DAE's scores, over hidden / feature rows with no zero entry pattern of their own,
    # compared bit for bit before and after (an altered weight or bias word of a tile changes a whole column of it).
    (z0, d0, _wt, _wp), _dev0 = _dense_route(m, f)
    before = _snapshot(m)
    a = _loss(m, f)
    b = _loss(m, f)
    assert a[0] == b[0] and (_bits(a[1]) == _bits(b[1])).all()              # two calls: the same bits
    assert _same(before, _snapshot(m))                                      # parameters, moments, the frozen DAE
    rec1 = m.recommend(f["xpos"], f["xones"], seeds, k=50, titles=f["titles"], titles_use=f["use"])
    assert np.array_equal(rec0[0], rec1[0]) and (_bits(rec0[1]) == _bits(rec1[1])).all()      # the lists and scores as they were
    (z1, d1, _wt, _wp), _dev1 = _dense_route(m, f)
    assert (_bits(z0) == _bits(z1)).all() and (_bits(d0) == _bits(d1)).all()                    # both images: every column, every row
    assert (_bits(_loss(m, f)[1]) == _bits(a[1])).all()                     # ... and behind a ranking call


def test_training_runs_end_with_the_same_bytes_with_calls_in_between(workdir):
    """Three --title training runs of four steps from the same start; the third calls mixed_loss between the steps.  The title
    step adds its embedding gradients with float atomics, so the runs use a scorer whose sums hold at most two terms each, which
    no order changes: one filter (one window per title reaches the embedding gradient) and titles that share no character."""
    B, steps = 4, 4

    def run(calls):
        m = _model(workdir, 128, 1, B, fresh=True, sizes=(3,), n_char=64)
        f = _feed(B, seed=23)
        f["titles"] = np.full((B, L), -1, np.int64)
        for r in range(B):
            f["titles"][r, :5] = np.arange(5) + 5 * r + 1
        for i in range(steps):
            if calls:
                _loss(m, f)
                _loss(m, f, keep_prob=0.8, input_keep_prob=0.75, title_keep_prob=0.9, seed=i)
            m.train_step(f["xpos"], f["xones"], f["ypos"], f["yval"], 0.8, 0.75, titles=f["titles"], titles_use=f["use"], title_keep_prob=0.9)
        return _snapshot(m)
    plain, again, called = run(False), run(False), run(True)
    assert _same(plain, again), "two identical training runs differ: the comparison below would say nothing"
    assert _same(plain, called)


# ---- 7. the C call and its arguments -------------------------------------------------------------------------------------------------
def test_the_c_call_equals_the_model_and_refuses_bad_arguments(workdir):
    import torch
    B = 300
    m = _model(workdir, 128, 25, B)
    f = _feed(B, seed=B + 128 + 25)
    cost, rows = _loss(m, f)
    _z, (h, feat, w_t, w_p) = _dense_route(m, f)
    tm = m.title_model
    t = dict(h=h, Wd=m.weights["decoder_h"], bd=m.biases["decoder_b"], feat=feat, Wt=tm.p["Output_WT"], bt=tm.p["Output_b"], w_t=w_t, w_p=w_p)
    rp, col, val = coo_to_csr(f["ypos"], f["yval"], B, V)
    csr = (_dev(rp), _dev(col), _dev(val))
    pair = Pair()
    try:
        with pytest.raises(_lib.DaeError, match="prepacked"):             # DAE_ERR_STATE: no image yet
            _abi(pair, t, B, B, csr)
        pair.t.prepack_decoder(t["Wt"], t["bt"], dtype=F32)
        with pytest.raises(_lib.DaeError, match="DAE's context"):          # ... nor on the DAE's context
            _abi(pair, t, B, B, csr)
        pair.d.prepack_decoder(t["Wd"], t["bd"], dtype=F32)
        r1, c1 = _abi(pair, t, B, B, csr)
        assert (_bits(r1) == _bits(rows)).all() and c1 == cost
        r2, none = _abi(pair, t, B, B, csr, cost=False)
        none2, c2 = _abi(pair, t, B, B, csr, rows=False)
        assert none is None and none2 is None and (_bits(r2) == _bits(rows)).all() and c2 == cost
        # a smaller batch on the same contexts (the scratch stays), rows 256.. as a batch of their own: the second panel's bits
        sub = (_dev(rp[256:] - rp[256]), _dev(col[rp[256]:]), _dev(val[rp[256]:]))
        r3, _c = _abi(pair, t, B - 256, B, sub, r0=256)
        assert (_bits(r3) == _bits(rows[256:])).all()
        # a target outside [0, V) is left out, never read
        bad_col = col.copy()
        bad_col[0], bad_col[-1] = -1, V
        r4, _c = _abi(pair, t, B, B, (csr[0], _dev(bad_col), csr[2]))
        assert np.isfinite(r4).all() and (_bits(r4[1:-1]) == _bits(rows[1:-1])).all() and r4[0] != rows[0]
        # dae_set_score_mix's state stays as the call found it
        mixT = torch.zeros((V, B), device="cuda")
        pair.t.check(pair.t.lib.dae_set_score_mix(pair.t.h, _lib._ptr(mixT), B, V, _lib._ptr(w_t)))
        r5, _c = _abi(pair, t, B, B, csr)
        assert (_bits(r5) == _bits(rows)).all()
        with pytest.raises(_lib.DaeError, match="clear dae_set_score_mix"):     # (still set: the calls that set it themselves say so)
            pair.t.mix_rank_of(pair.d, h, t["Wd"], t["bd"], feat, t["Wt"], t["bt"], w_t, w_p, NT, None, None, (csr[0], csr[1]), 0,
                               torch.zeros(1, dtype=torch.int32, device="cuda"))
        pair.t.check(pair.t.lib.dae_set_score_mix(pair.t.h, None, 0, 0, None))
        lib, P = pair.t.lib, _lib._ptr
        spare = torch.zeros(B, device="cuda")

        def call(**kw):
            a = dict(tc=pair.t.h, dc=pair.d.h, h=P(h), ld_h=128, H=128, Wd=P(t["Wd"]), bd=P(t["bd"]), feat=P(feat), ld_feat=64, Wt=P(t["Wt"]),
                     bt=P(t["bt"]), wt=P(w_t), wp=P(w_p), B=B, V=V, nb=B, rp=P(csr[0]), col=P(csr[1]), val=P(csr[2]),
                     rows=P(spare), cost=None)
            a.update(kw)
            return lib.dae_mix_loss_rows(*a.values())
        ARG, STATE = -1, -4                                                     # include/dae_hip.h DAE_ERR_ARG, DAE_ERR_STATE
        assert call() == 0
        for kw in (dict(rows=None), dict(B=0), dict(B=4097), dict(H=100), dict(H=1056, ld_h=1056), dict(ld_feat=62), dict(ld_feat=1028),
                   dict(ld_h=256), dict(nb=0), dict(dc=pair.t.h), dict(dc=None), dict(wt=None), dict(V=0)):
            rc = call(**kw)
            assert rc == ARG, (kw, rc)
        assert call(V=V - 1) == STATE and call(H=64, ld_h=64) == ARG            # no image over those columns / of that K
    finally:
        pair.close()


def test_python_refusals(workdir):
    m = _model(workdir, 128, 25, 33, fresh=True)
    f = _feed(33, seed=3)
    args = (f["xpos"], f["xones"], f["ypos"], f["yval"])
    with pytest.raises(ValueError, match="titles are required"):
        m.mixed_loss(*args, None, f["use"])
    with pytest.raises(ValueError, match="n_rows"):
        m.mixed_loss(*args, f["titles"], f["use"], n_rows=34)
    with pytest.raises(_lib.DaeError, match="titles in use"):                   # `loss` keeps refusing titles
        m.loss(*args, titles=f["titles"], titles_use=f["use"])
    m.shard_scoring(0, 2)
    with pytest.raises(_lib.DaeError, match="scoring shard"):
        m.mixed_loss(*args, f["titles"], f["use"])


# ---- 8. the driver -------------------------------------------------------------------------------------------------------------------
def test_driver_logs_one_mixed_loss_line_per_split_with_eval_mixed_loss_on(tmp_path):
    """main.py --title on the golden mini dataset: a training run with [BASE] eval_mixed_loss = on logs one more line per split
    behind the existing ones at every evaluation; --testmode with the key `on` one more line per split, and without the key (and
    with `off`) the log is what it was; --dae refuses the key by name."""
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
        ini = open(work / "config.ini").read()
        splits = ("test-0", "test-1", "test-5", "test-25r")

        def lines(base_key, *argv):
            open(work / "config.ini", "w").write(ini.replace("[BASE]", "[BASE]\n" + base_key))
            n0 = len(open(work / "log.txt").read().splitlines()) if os.path.exists(work / "log.txt") else 0
            assert cli.main(["--dir", "run"] + list(argv)) == 0
            return [l for l in open(work / "log.txt").read().splitlines()[n0:] if l.startswith("seed num")]
        lines("", "--pretrain")
        lines("", "--dae")
        trained = lines("eval_mixed_loss = on", "--title")                   # a training run: the line at every evaluation
        mine = [l for l in trained if " mixed heldout loss: " in l]
        assert len(mine) >= 4 and len(mine) * 2 == len(trained)
        plain = lines("", "--title", "--testmode")
        assert len(plain) == 4 and lines("eval_mixed_loss = off", "--title", "--testmode") == plain
        full = lines("eval_mixed_loss = on", "--title", "--testmode")
        assert len(full) == 8 and full[:4] == plain
        for l, s in zip(full[4:], splits):
            assert l.startswith("seed num: %s mixed heldout loss: " % s), l
            assert 0.0 < float(l.split()[-1]) < 1e6
        with pytest.raises(ValueError, match="eval_mixed_loss.*--title"):
            cli.main(["--dir", "run", "--dae", "--testmode"])
    finally:
        os.chdir(cwd)
