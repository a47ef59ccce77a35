"""GPU (-m gpu): the title scorer across the shapes its config keys allow ([TITLE] char_emb, filter_num, filter_size,
strmaxlen; reference main.py:69-75), against oracle/title_numpy.py.

dae_launch_title_features (csrc/title.hip) picks one of five kernels by shape.  The cases of SHAPES reach each one:

  case        E    sizes            F    L   forward kernels                        why
  wave24      25   3, 5             40   25  table; wave<24, 8>                     fs E odd (75, 125); p_max = 23
  wave32      25   1, 4             40   25  table; wave<32, 8>                     fs E = 25 odd; fs 1 -> p_max = 25
  mfma_oddE   51   2, 4             70   25  table; mfma<8>                         every fs E even with E odd
  emb128      128  1, 25            32   25  table; mfma<8>                         E = T_MAX_EMB; P = 25 and P = 1
  eight       16   1 .. 8           7    25  table; mfma<8>                         8 sizes, one partial filter block
  ld1024      50   3, 5, 7, 9       256  25  table; mfma<8>                         1024 features: the fp32 prepack's limit
  f448        50   3, 5, 7, 9       112  25  table; mfma<8>                         448 real features, no zero column
  len40       50   3, 5             64   40  title_features_kernel (both)           p_max = 38 > 32
  len64       24   2, 3             32   64  title_features_kernel (both)           p_max = 63: the table refuses

("table" = inference, title_features_table_kernel; the other kernel is what training and dropout run.)  Titles carry
padding, ids >= charsize and negative ids other than -1: all embed to zero and take no gradient."""
import copy
import pickle

import numpy as np
import pytest

import oracle
from oracle import dae_numpy as dn
from oracle import title_numpy as tn
from spotify_recsys_challenge_2018_amd.models.DAEs import DAE, DAE_title, SEEDS_FROM_INPUT, coo_to_csr, seeds_to_csr
from spotify_recsys_challenge_2018_amd.models.title_models import get_model
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights

pytestmark = pytest.mark.gpu
U = tn.U32
N_CHAR = 41

SHAPES = {                    # E, filter sizes, F, strmaxlen
    "wave24": (25, [3, 5], 40, 25),
    "wave32": (25, [1, 4], 40, 25),
    "mfma_oddE": (51, [2, 4], 70, 25),
    "emb128": (128, [1, 25], 32, 25),
    "eight": (16, [1, 2, 3, 4, 5, 6, 7, 8], 7, 25),
    "ld1024": (50, [3, 5, 7, 9], 256, 25),
    "f448": (50, [3, 5, 7, 9], 112, 25),
    "len40": (50, [3, 5], 64, 40),
    "len64": (24, [2, 3], 32, 64),
}


def _conf(E, fs, F, L, batch=24, n_input=1500, n_tracks=1200, hidden=64):
    class Conf:
        lr = 0.01; reg_lambda = 0.0; charsize = N_CHAR; char_model = 'Char_CNN'; save = "/tmp/_title_unused"
        initval = "NULL"; title_lr = 0.002
    c = Conf()
    c.char_emb, c.filter_size, c.filter_num, c.strmaxlen = E, list(fs), F, L
    c.batch, c.n_input, c.n_output, c.n_tracks, c.hidden = batch, n_input, n_input, n_tracks, hidden
    return c


def _titles(B, L, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, N_CHAR, (B, L))
    for r in range(B):
        t[r, int(rng.integers(0, L + 1)):] = -1         # right-padded like change_title2ixs
    t[0, :] = -1                                         # an empty title
    t[1, :] = np.arange(L) % N_CHAR                      # a full-length one: every window live
    t[2, 0], t[2, 3] = N_CHAR, 10 ** 6                   # ids >= charsize
    t[3, 1], t[3, 2] = -2, -(2 ** 31)                    # negative ids other than -1
    return t


def _uniform(seed, stream, rows, cols):
    l = oracle.lib()
    return np.array([[l.orc_uniform(seed, stream, int(r), int(c)) for c in cols] for r in rows], np.float32)


def _dae_title(tmp_path, conf, seed=4):
    W_enc, b_enc, W_dec, b_dec = make_weights(conf.n_input, conf.hidden, seed=1, bias="zipf", n_tracks=conf.n_tracks)
    b_enc = (np.random.default_rng(2).standard_normal(conf.hidden) * 0.1).astype(np.float32)
    pk = tmp_path / "w_dae"
    with open(pk, "wb") as f:
        pickle.dump([W_enc, W_dec, b_enc, b_dec], f)
    conf.DAEval = str(pk)
    mt = get_model(conf)
    host = tn.make_params(N_CHAR, conf.char_emb, conf.filter_size, conf.filter_num, conf.n_output, seed=seed)
    mt.fit(host)
    m = DAE_title(conf, mt)
    m.fit()
    return m, host, (W_enc, b_enc, W_dec, b_dec)


def _table_bounds(titles, host, fs, E):
    """feature_bounds of title_features_table_kernel: E roundings per table entry, then fs + 1 additions."""
    return np.concatenate([tn.feature_bounds(titles, {**host, "Conv_W0": host["Conv_W%d" % i], "Conv_b0": host["Conv_b%d" % i]},
                                             [f], extra_terms=E + f - f * E) for i, f in enumerate(fs)], axis=1)


def _sig_err(s, z, zerr):
    """fp32 sigmoid of a logit known within zerr: as in title_grad_bounds (exp's argument error, 1 ulp exp, add, rcp)."""
    return s * (1 - s) * (4 * U * (np.abs(z) + 1) + 1.01 * zerr) + 3 * U * s


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_features_per_shape(name):
    """Chain kernels (kept for backward; with dropout): the fmaf chain of features_f32_chain bit for bit, argmax
    included, dropout masks from orc_uniform stream 2.  Inference: the table path within its derived bound of the chain
    and of float64 -- or, where the launcher refuses the table (p_max > 32), the chain's bits."""
    E, fs, F, L = SHAPES[name]
    conf = _conf(E, fs, F, L)
    m = get_model(conf)
    host = tn.make_params(N_CHAR, E, fs, F, conf.n_output, seed=7)
    m.fit(host)
    B, nf = 24, len(fs) * F
    titles = _titles(B, L, seed=len(name))
    chain, carg = tn.features_f32_chain(titles, host, fs)
    feat, _d, arg, raw = (a.cpu().numpy() for a in m.features(titles, B, keep_for_backward=True))
    assert feat.shape == (B, m.ld) and not feat[:, nf:].any()
    assert np.array_equal(raw.view(np.uint32), chain.view(np.uint32))
    assert np.array_equal(arg, carg)
    assert np.array_equal(feat[:, :nf].view(np.uint32), chain.view(np.uint32))
    kp, seed = 0.8, 31
    fd, _d, argd, rawd = (a.cpu().numpy() for a in m.features(titles, B, keep_prob=kp, seed=seed, keep_for_backward=True))
    mask = np.floor(np.float32(kp) + _uniform(seed, 2, range(B), range(nf)))
    assert np.array_equal(rawd.view(np.uint32), chain.view(np.uint32)) and np.array_equal(argd, carg)
    assert np.array_equal(fd[:, :nf].view(np.uint32), ((chain / np.float32(kp)) * mask).view(np.uint32))
    assert not fd[:, nf:].any()
    tab = m.features(titles, B).cpu().numpy()
    assert not tab[:, nf:].any()
    tab = tab[:, :nf]
    if L - min(fs) + 1 > 32:
        assert np.array_equal(tab.view(np.uint32), chain.view(np.uint32))
    else:
        f64 = tn.features(titles, host, fs)
        b_chain = tn.feature_bounds(titles, host, fs)
        b_tab = _table_bounds(titles, host, fs, E)
        assert np.all(np.abs(tab - f64) <= b_tab)
        assert np.all(np.abs(tab - chain) <= b_tab + b_chain)


def _mixed_bound(m, host, dae_w, pos, ones, titles, use, conf):
    """float64 mixed scores and their bound: table features -> fp32 decoder GEMM -> sigmoid; the DAE from oracle.encode's
    bit-exact h; the fp32 mixing weights (row sums of ones: exact, the same four operations)."""
    W_enc, b_enc, W_dec, b_dec = dae_w
    B, fs = conf.batch, conf.filter_size
    E = conf.char_emb
    f64 = tn.features(titles, host, fs)
    ef = np.maximum(_table_bounds(titles, host, fs, E), tn.feature_bounds(titles, host, fs))     # (table or chain)
    Wo, bo = host["Output_W"].astype(np.float64), host["Output_b"].astype(np.float64)
    z = f64 @ Wo + bo
    ez = (f64.shape[1] + 2) * U * (np.abs(f64) @ np.abs(Wo) + np.abs(bo)) + ef @ np.abs(Wo)
    st = 1 / (1 + np.exp(-z))
    rp, c, v = coo_to_csr(pos, ones, B, conf.n_input)
    h = oracle.encode(rp, c, v, W_enc, b_enc)
    zd = h.astype(np.float64) @ W_dec.astype(np.float64).T + b_dec
    dae = 1 / (1 + np.exp(-zd))
    w_t, w_p = tn.mix_weights(m._row_sums(pos, ones), 1.0, use)
    y = tn.mix(st, dae, w_t, w_p)
    bound = w_t * _sig_err(st, z, ez) + w_p * _sig_err(dae, zd, tn.dae_logit_bounds(h, W_dec, b_dec)) + 3 * U * np.abs(y)
    return y, bound


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_scoring_per_shape(tmp_path, name):
    """mixed_scores within its bound of float64; recommend's lists equal oracle.topk on the GPU's own mixed matrix.
    One odd-E shape and the 1024-feature one also stream through recommend_iter (the native titled pipeline)."""
    E, fs, F, L = SHAPES[name]
    conf = _conf(E, fs, F, L)
    m, host, dae_w = _dae_title(tmp_path, conf)
    B = conf.batch
    pos, ones, seeds = make_playlists(B, conf.n_tracks, conf.n_input - conf.n_tracks, seed=5)
    titles = _titles(B, L, seed=6)
    use = (np.arange(B) % 3 != 0).astype(np.float32)
    y = m.mixed_scores(pos, ones, titles, use).cpu().numpy()
    y64, bound = _mixed_bound(m, host, dae_w, pos, ones, titles, use, conf)
    assert np.all(np.abs(y - y64) <= bound), float(np.max(np.abs(y - y64) / bound))
    idx, score = m.recommend(pos, ones, seeds, k=100, titles=titles, titles_use=use)
    srp, sc = seeds_to_csr(seeds, B, conf.n_tracks)
    s_ref, i_ref = oracle.topk(np.ascontiguousarray(y[:, :conf.n_tracks]), 100, srp, sc, out_kind=1)
    assert np.array_equal(idx, i_ref) and np.array_equal(score.view(np.uint32), s_ref.view(np.uint32))
    if name in ("wave24", "ld1024"):
        feeds, want = [], []
        for i in range(4):
            p_, o_, _s = make_playlists(B, conf.n_tracks, conf.n_input - conf.n_tracks, seed=40 + i)
            t_ = _titles(B, L, seed=50 + i)
            u_ = (np.arange(B) % 3 != i % 3).astype(np.float32)
            s_ = [sorted(set(int(c) for r, c in p_ if r == row and c < conf.n_tracks)) for row in range(B)]
            n = [B, 7, B, 19][i]
            feeds.append((p_, o_, SEEDS_FROM_INPUT, n, t_, u_))
            want.append(m.recommend(p_, o_, s_, k=100, n_rows=n, titles=t_, titles_use=u_))
        got = list(m.recommend_iter(feeds, k=100))
        assert any(p[1].title_len == L for p in m.__dict__.get("_pipes", {}).values())       # the native titled pipeline
        for (gi, gs), (wi, ws) in zip(got, want):
            assert np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32))


def _spy_backward(mt, captured):
    """Wrap the title model's backward: record the forward values the step differentiates (its title logits, DAE scores and
    mixing weights) and the dfeat its conv backward reads -- dae_title_loss_backward run once more on the same inputs into
    scratch outputs (deterministic kernels: the same bits) -- then run the step itself."""
    import torch
    from spotify_recsys_challenge_2018_amd import _lib
    orig = mt.backward_and_step

    def spy(feat, d_titles, arg, raw, z_title, dae_score, y_csr, w_t, w_p, n_batch, keep_prob, seed, cost_out):
        B, V = z_title.shape
        P = _lib._ptr
        dfeat = torch.empty((B, mt.ld), dtype=torch.float32, device=feat.device)
        gw, gb = torch.empty_like(mt.p["Output_WT"]), torch.empty_like(mt.p["Output_b"])
        c = torch.empty(1, dtype=torch.float32, device=feat.device)
        mt.ctx.check(mt.ctx.lib.dae_title_loss_backward(
            mt.ctx.h, P(z_title), int(z_title.stride(0)), P(dae_score), int(dae_score.stride(0)),
            P(y_csr[0]), P(y_csr[1]), P(y_csr[2]), P(w_t), P(w_p), B, V, int(n_batch),
            P(feat), mt.ld, P(mt.p["Output_WT"]), P(gw), P(gb), P(dfeat), P(c)))
        captured.update(z=z_title.cpu().numpy(), dae=dae_score.cpu().numpy(), w_t=w_t.cpu().numpy(),
                        w_p=w_p.cpu().numpy(), dfeat=dfeat.cpu().numpy())
        return orig(feat, d_titles, arg, raw, z_title, dae_score, y_csr, w_t, w_p, n_batch, keep_prob, seed, cost_out)
    mt.backward_and_step = spy


def _train_and_check(tmp_path, conf, ikp, kp, tkp, steps, stats, label):
    """`steps` training steps.  Each one: the forward values the step differentiates (title logits, DAE scores, mixing
    weights) within their bounds of float64; the cost, Output_W / Output_b gradients and dfeat against grads() run ON those
    values, within title_grad_bounds (dfeat with grad_h's own two-level sum); the conv and embedding gradients against
    conv_grads_from_dfeat on the step's own dfeat, so that title_gate / wgrad / egrad are bounded by their own rounding
    alone; every bound rejects half the gradient (none is vacuous); Adam's moments bit for bit at this model's step and
    title_lr, its parameters within 1 ulp; the padding columns zero; an inference call after it reading the new variables."""
    import torch
    m, host, (W_enc, b_enc, W_dec, b_dec) = _dae_title(tmp_path, conf)
    mt = m.title_model
    captured = {}
    _spy_backward(mt, captured)
    B, V, L, fs, F = conf.batch, conf.n_input, conf.strmaxlen, conf.filter_size, conf.filter_num
    nf = len(fs) * F
    pos, _o, _s = make_playlists(B, conf.n_tracks, V - conf.n_tracks, seed=5, seed_counts=(3, 9, 20))
    yo = np.ones(len(pos), np.float32)
    titles = _titles(B, L, seed=6)
    xr, xc, xv = coo_to_csr(pos, yo, B, V)
    x = dn.sparse_to_dense(pos, yo, B, V)
    cur = host
    for t in range(1, steps + 1):
        seed = int(copy.deepcopy(m._rng).randint(0, 2 ** 31 - 1))         # the draw train_step will make
        mom = {n: tuple(a.cpu().numpy() for a in mt._adam[n]) for n in mt._tvars} if getattr(mt, "_adam", None) else None
        before = {n: mt.p[n].cpu().numpy() for n in ("char_embedding", "conv_w", "conv_b", "Output_WT", "Output_b")}
        cost = m.train_step(pos, yo, pos, yo, kp, ikp, titles=titles, title_keep_prob=tkp)
        assert mt._step == t                                                 # this model's own counter
        g = {k: v.cpu().numpy() for k, v in mt._grads.items()}
        # ---- the forward the step differentiates, against float64 with the same draws --------------------------------
        chain, carg = tn.features_f32_chain(titles, cur, fs)
        im = None
        if ikp < 1.0:
            im = np.ones((B, V), np.float32)
            for r in range(B):
                cols = xc[xr[r]:xr[r + 1]]
                im[r, cols] = np.floor(np.float32(ikp) + _uniform(seed, 0, [r], cols)[0])
        h = oracle.encode(xr, xc, xv, W_enc, b_enc, ikp, kp, seed)                      # the encode kernel's bits
        zd = h.astype(np.float64) @ W_dec.astype(np.float64).T + b_dec
        dae64 = 1 / (1 + np.exp(-zd))
        assert np.all(np.abs(captured["dae"] - dae64) <= _sig_err(dae64, zd, tn.dae_logit_bounds(h, W_dec, b_dec)))
        s = (x.astype(np.float64) / ikp * (im if im is not None else 1.0)).sum(axis=1)
        w_t, w_p = tn.mix_weights(s, ikp, np.ones(B))
        w_rel = (np.diff(xr).max() + 8) * U
        assert np.all(np.abs(captured["w_t"] - w_t[:, 0]) <= w_rel * w_t[:, 0])
        assert np.all(np.abs(captured["w_p"] - w_p[:, 0]) <= w_rel * w_p[:, 0])
        tm_mask = np.floor(np.float32(tkp) + _uniform(seed, 2, range(B), range(nf))) if tkp < 1.0 else None
        _c64, _g64, info64 = tn.grads(titles, cur, fs, dae64, x > 0, w_t, w_p, B, keep_mask=tm_mask, keep_prob=tkp,
                                      argmax=carg, gate=chain > 0)
        assert np.all(np.abs(captured["z"] - info64["z"]) <= tn.title_logit_bounds(info64))
        # ---- the backward, on those values ------------------------------------------------------------------------
        ref_cost, ref, info = tn.grads(titles, cur, fs, captured["dae"], x > 0, captured["w_t"], captured["w_p"], B,
                                       keep_mask=tm_mask, keep_prob=tkp, argmax=carg, gate=chain > 0, z=captured["z"])
        bounds = tn.title_grad_bounds(info, dae_zerr=None, dfeat_split=tn.grad_h_split(V, mt.ld, B))
        assert abs(cost - ref_cost) <= bounds["cost"], (cost, ref_cost, bounds["cost"])
        assert not captured["dfeat"][:, nf:].any()
        ref["dfeat"] = info["_aux"]["dfeat"]
        rc, bc = tn.conv_grads_from_dfeat(info, captured["dfeat"])
        ref.update(rc)
        bounds.update(bc)
        got = {"Output_W": g["Output_WT"][:, :nf].T, "Output_b": g["Output_b"], "char_embedding": g["char_embedding"],
               "dfeat": captured["dfeat"][:, :nf]}
        off = 0
        for i, f in enumerate(fs):
            got["Conv_W%d" % i] = g["conv_w"][off:off + f * conf.char_emb * F]
            got["Conv_b%d" % i] = g["conv_b"][i * F:(i + 1) * F]
            off += f * conf.char_emb * F
        assert not g["Output_WT"][:, nf:].any() and not mt.p["Output_WT"][:, nf:].any().item()
        r = tn.grad_check(got, ref, bounds)
        for k, q in r.items():
            key = k.rstrip("0123456789")
            stats[key] = max(stats.get(key, 0.0), q)
        assert max(r.values()) <= 1.0, (label, t, r)
        for k in ref:                                     # no bound is vacuous: half of any gradient leaves it
            assert tn.grad_check({k: 0.5 * ref[k]}, {k: ref[k]}, bounds)[k] > 1.0, (label, t, k)
        # ---- Adam: TF1's fp32 sequence on the GPU's own gradients, step t of this model, lr = title_lr -------------------
        for n in mt._tvars:
            m0, v0 = mom[n] if mom else (np.zeros_like(before[n]), np.zeros_like(before[n]))
            p2, m2, v2 = dn.adam_tf(before[n], m0, v0, g[n], conf.title_lr, t)
            mm, vv = (a.cpu().numpy() for a in mt._adam[n])
            assert np.array_equal(mm, m2) and np.array_equal(vv, v2), (label, t, n)
            assert np.allclose(mt.p[n].cpu().numpy(), p2, rtol=3e-7, atol=1e-9), (label, t, n)
        cur = mt.get_params()
        # ---- scoring after an in-place step reads the new variables (the table was dropped and rebuilt) ------------------
        if L - min(fs) + 1 <= 32:
            inf = mt.features(titles, B).cpu().numpy()[:, :nf]
            new_chain, _ = tn.features_f32_chain(titles, cur, fs)
            b_tab = _table_bounds(titles, cur, fs, conf.char_emb)
            assert np.all(np.abs(inf - new_chain) <= b_tab + tn.feature_bounds(titles, cur, fs))
            assert np.max(np.abs(inf - chain)) > 10 * np.max(b_tab)                    # (and not the old variables')
        torch.cuda.synchronize()
    return m


STATS = {}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_training_per_shape(tmp_path, name):
    E, fs, F, L = SHAPES[name]
    conf = _conf(E, fs, F, L)
    _train_and_check(tmp_path, conf, 0.75, 0.8, 0.8, 3, STATS, name)
    print("\n%s: max error / bound so far: %s" % (name, {k: "%.3g" % v for k, v in sorted(STATS.items())}))


def test_training_shipped_config(tmp_path):
    """The shipped [TITLE] training: batch 150, input_kp 0.01, kp 0.8, title_kp 0.8 (3, 5, 7, 9 x 100, embedding 50)."""
    conf = _conf(50, [3, 5, 7, 9], 100, 25, batch=150, n_input=2300, n_tracks=2000)
    _train_and_check(tmp_path, conf, 0.01, 0.8, 0.8, 3, STATS, "shipped")
    print("\nshipped: max error / bound so far: %s" % {k: "%.3g" % v for k, v in sorted(STATS.items())})


def test_training_full_size(tmp_path):
    """One step at the reference's full size: 170 000 columns (140 000 tracks), batch 150, hidden 256, 3, 5, 7, 9 x 100."""
    conf = _conf(50, [3, 5, 7, 9], 100, 25, batch=150, n_input=170000, n_tracks=140000, hidden=256)
    _train_and_check(tmp_path, conf, 0.5, 0.8, 0.8, 1, STATS, "full")
    print("\nall cases: max error / bound: %s" % {k: "%.3g" % v for k, v in sorted(STATS.items())})


# ---- limits: shapes the kernels cannot run fail before any launch, naming the config key --------------------------------

@pytest.mark.parametrize("change,key", [(dict(char_emb=129), "char_emb"), (dict(filter_size=list(range(1, 10))), "filter_size"),
                                        (dict(filter_size=[0, 3]), "filter_size"), (dict(filter_size=[3, 26]), "filter_size"),
                                        (dict(strmaxlen=65, filter_size=[3]), "strmaxlen")])
def test_unsupported_shapes_are_refused_at_construction(change, key):
    conf = _conf(50, [3, 5], 10, 25)
    for k, v in change.items():
        setattr(conf, k, v)
    with pytest.raises(ValueError, match=r"\[TITLE\] %s" % key):
        get_model(conf)


def test_unsupported_training_and_scoring_widths_are_refused(tmp_path):
    import torch
    conf = _conf(8, [2, 3], 257, 25)                         # 514 features: scores, but cannot train
    m, host, _w = _dae_title(tmp_path, conf)
    pos, ones, seeds = make_playlists(24, conf.n_tracks, conf.n_input - conf.n_tracks, seed=5)
    titles = _titles(24, 25, seed=1)
    before = m.title_model.get_params()
    with pytest.raises(ValueError, match=r"\[TITLE\] filter_num"):
        m.train_step(pos, ones, pos, ones, 1.0, 1.0, titles=titles)
    after = m.title_model.get_params()
    assert all(np.array_equal(before[k], after[k]) for k in before) and getattr(m.title_model, "_step", 0) == 0
    m.recommend(pos, ones, seeds, k=10, titles=titles, titles_use=np.ones(24))       # scoring at 576 columns runs
    conf2 = _conf(8, [2, 3, 4, 5, 6], 210, 25)               # 1050 features -> 1088 > 1024
    mt2 = get_model(conf2)
    mt2.fit(tn.make_params(N_CHAR, 8, conf2.filter_size, 210, conf2.n_output, seed=1))
    with pytest.raises(ValueError, match=r"\[TITLE\] filter_num x filter_size"):
        mt2.score(titles, 24)
    torch.cuda.synchronize()


def test_plain_dae_takes_titled_feeds(tmp_path):
    """recommend_iter on a plain DAE fed 6-item (titled) feeds returns what it returns for the same 4-item feeds: the
    plain model ignores titles (it used to pass them to DAE.recommend, which has no such arguments)."""
    conf = _conf(50, [3, 5], 10, 25)
    W_enc, b_enc, W_dec, b_dec = make_weights(conf.n_input, conf.hidden, seed=1, bias="zipf", n_tracks=conf.n_tracks)
    model = DAE(conf)
    model._host_init = lambda: [W_enc, W_dec, b_enc, b_dec]
    model.fit()
    B = conf.batch
    plain, titled = [], []
    for i in range(3):
        p_, o_, _s = make_playlists(B, conf.n_tracks, conf.n_input - conf.n_tracks, seed=60 + i)
        plain.append((p_, o_, SEEDS_FROM_INPUT, B))
        titled.append((p_, o_, SEEDS_FROM_INPUT, B, _titles(B, 25, seed=i), np.ones(B, np.float32)))
    want = list(model.recommend_iter(plain, k=50))
    got = list(model.recommend_iter(titled, k=50))
    got5 = list(model.recommend_iter([f[:5] for f in titled], k=50))
    model.device_csr = False                                  # the per-batch loop
    got_host = list(model.recommend_iter(titled, k=50))
    for res in (got, got5, got_host):
        assert len(res) == 3
        for (gi, gs), (wi, ws) in zip(res, want):
            assert np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
