"""GPU (-m gpu): vocabulary-sharded --title training.

1. dae_title_loss_backward_cols (csrc/title.hip title_loss_cols_kernel) on a column window against dae_title_loss_backward
   on the host-sliced problem, bit for bit.
2. Its argument errors: DaeError, nothing written.
3. One sharded step by hand (the shards one after another on the one GPU, the collectives as sums / copies) against
   oracle.title_numpy.grads with the same dropout masks and against the unsharded DAE_title.train_step.
4. DAE_title.shard_title_training(0, 1): both feeds, sync_params, save / load, scoring.
5. main.py --title under two gloo ranks on one device."""
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import dae_numpy as dn
from oracle import title_numpy as tn
from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.models.DAEs import coo_to_csr
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists
from test_gpu_title_shapes import _conf, _dae_title, _titles, _uniform

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")

V1, LD1 = 2003, 96
WINDOWS = [(0, 2003), (45, 1001), (1984, 2003), (32, 64)]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ---- 1. the window entry point against the dense one on the sliced problem ---------------------------------------------------

def _window_csr(B, lo, hi, seed):
    """The whole batch's y CSR (global ids, ascending and unique per row; ids run past the largest window, so something
    lies outside every window): row 0 empty; row 1 only targets outside [lo, hi); row 2 targets at lo - 1, lo, hi - 1 and
    hi; row 3 a run of consecutive ids that fills whole 32-column tiles of the window (more than 32 targets, and 32 of them
    in one tile of the row's tile row); the other rows random, values 1 or 0.5."""
    rng = np.random.default_rng(seed)
    n_ids = 2100
    rows = []
    for r in range(B):
        if r == 0:
            ids = []
        elif r == 1:
            ids = [c for c in (lo - 40, lo - 1, hi, hi + 1, hi + 33, n_ids - 1) if 0 <= c < n_ids]
        elif r == 2:
            ids = [c for c in (lo - 1, lo, hi - 1, hi) if 0 <= c < n_ids]
        elif r == 3:
            ids = [c for c in range(lo - 3, lo + 75) if 0 <= c < n_ids]
        else:
            ids = rng.choice(n_ids, size=int(rng.integers(1, 60)), replace=False)
        rows.append(np.unique(np.asarray(ids, np.int64)))
    rp = np.zeros(B + 1, np.int32)
    rp[1:] = np.cumsum([len(c) for c in rows])
    col = np.concatenate(rows).astype(np.int32)
    val = np.where(rng.random(len(col)) < 0.8, 1.0, 0.5).astype(np.float32)
    return rp, col, val


@pytest.fixture(scope="module")
def dense_inputs():
    rng = np.random.default_rng(3)
    B = 150
    zt = (rng.standard_normal((B, V1)) * 2).astype(np.float32)
    dae = rng.uniform(0.001, 0.999, (B, V1)).astype(np.float32)
    w_t = rng.uniform(0.05, 0.6, B).astype(np.float32)
    w_p = (np.float32(0.999) - w_t).astype(np.float32)
    feat = np.maximum(rng.standard_normal((B, LD1)), 0).astype(np.float32)
    feat[:, 90:] = 0
    WT = (rng.standard_normal((V1, LD1)) * 0.05).astype(np.float32)
    return zt, dae, w_t, w_p, feat, WT


@pytest.mark.parametrize("B", [37, 64, 150])
@pytest.mark.parametrize("lo,hi", WINDOWS)
def test_window_equals_dense_on_the_sliced_problem(ctx, dense_inputs, B, lo, hi):
    import torch
    zt, dae, w_t, w_p, feat, WT = (a[:B] if i < 5 else a for i, a in enumerate(dense_inputs))
    rp, col, val = _window_csr(B, lo, hi, seed=B + lo)
    assert (np.diff(rp) == 0).any() and (col == lo).any() and (col == hi - 1).any() and (col == hi).any()
    assert max(np.sum((col[rp[r]:rp[r + 1]] >= lo) & (col[rp[r]:rp[r + 1]] < hi)) for r in range(B)) > min(32, hi - lo - 1)
    V = hi - lo
    P = _lib._ptr
    ctx.bind_stream()
    # the window call: whole-batch CSR, window columns of the two matrices (row stride = the window), the window's rows
    d_z, d_d = _dev(zt[:, lo:hi]), _dev(dae[:, lo:hi])
    d_y = tuple(_dev(a) for a in (rp, col, val))
    d_wt, d_wp, d_f, d_W = _dev(w_t), _dev(w_p), _dev(feat), _dev(WT[lo:hi])
    got = dict(gW=torch.full((V, LD1), 7.0, device="cuda"), gb=torch.full((V,), 7.0, device="cuda"),
               dfeat=torch.full((B, LD1), 7.0, device="cuda"), cost=torch.full((1,), 7.0, device="cuda"))
    ctx.title_loss_backward_cols(d_z, d_d, d_y, d_wt, d_wp, lo, hi, B, d_f, d_W, got["gW"], got["gb"], got["dfeat"], got["cost"])
    # the dense call on the sliced problem: the CSR restricted to the window and shifted by -lo
    keep = (col >= lo) & (col < hi)
    rows = np.repeat(np.arange(B), np.diff(rp))
    rp_s = np.zeros(B + 1, np.int32)
    rp_s[1:] = np.cumsum(np.bincount(rows[keep], minlength=B))
    d_ys = (_dev(rp_s), _dev((col[keep] - lo).astype(np.int32)), _dev(val[keep]))
    ref = dict(gW=torch.full((V, LD1), 9.0, device="cuda"), gb=torch.full((V,), 9.0, device="cuda"),
               dfeat=torch.full((B, LD1), 9.0, device="cuda"), cost=torch.full((1,), 9.0, device="cuda"))
    ctx.check(ctx.lib.dae_title_loss_backward(
        ctx.h, P(d_z), V, P(d_d), V, P(d_ys[0]), P(d_ys[1]), P(d_ys[2]), P(d_wt), P(d_wp), B, V, B, P(d_f), LD1, P(d_W),
        P(ref["gW"]), P(ref["gb"]), P(ref["dfeat"]), P(ref["cost"])))
    torch.cuda.synchronize()
    for k in ("gW", "gb", "dfeat", "cost"):
        a, b = got[k].cpu().numpy(), ref[k].cpu().numpy()
        assert np.isfinite(b).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (k, float(np.abs(a - b).max()))
    assert got["gW"].abs().max().item() > 0 and not got["gW"][:, 90:].any().item()


# ---- 2. refusals ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("change", [dict(lo=-1), dict(lo=64, hi=64), dict(lo=64, hi=32), dict(B=0), dict(B=257), dict(ld=80)])
def test_window_argument_errors_write_nothing(ctx, change):
    import torch
    a = dict(lo=32, hi=96, B=40, ld=96)
    a.update(change)
    rows, V = 300, 96                                     # room for every case; the good values are never reached
    d_z = torch.zeros((rows, V), device="cuda"); d_d = torch.full((rows, V), 0.5, device="cuda")
    d_y = (torch.zeros(rows + 1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
           torch.ones(1, device="cuda"))
    d_w = torch.full((rows,), 0.4, device="cuda")
    d_f = torch.ones((rows, 96), device="cuda"); d_W = torch.ones((V, 96), device="cuda")
    outs = [torch.full((V, 96), -3.0, device="cuda"), torch.full((V,), -3.0, device="cuda"),
            torch.full((rows, 96), -3.0, device="cuda"), torch.full((1,), -3.0, device="cuda")]
    P = _lib._ptr
    ctx.bind_stream()
    with pytest.raises(_lib.DaeError, match="error"):
        ctx.check(ctx.lib.dae_title_loss_backward_cols(
            ctx.h, P(d_z), V, P(d_d), V, P(d_y[0]), P(d_y[1]), P(d_y[2]), P(d_w), P(d_w), a["B"], a["lo"], a["hi"], 40,
            P(d_f), a["ld"], P(d_W), P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3])))
    torch.cuda.synchronize()
    assert all(bool((o == -3.0).all().item()) for o in outs)


# ---- 3. one sharded step by hand ----------------------------------------------------------------------------------------------

V3, NT3, H3, E3, FS3, F3, L3 = 2003, 1600, 64, 16, [3, 5], 40, 25
KP, IKP, TKP = 0.8, 0.75, 0.8
_CASES = {}


def _step_case(tmp_path_factory, B):
    """Per batch size, made once: a model whose variables never move (the sharded steps run on it), the float64 gradients
    with the step's dropout masks, and the unsharded DAE_title.train_step's gradients from a second, identical model."""
    if B in _CASES:
        return _CASES[B]
    conf = _conf(E3, FS3, F3, L3, batch=B, n_input=V3, n_tracks=NT3, hidden=H3)
    m, host, (W_enc, b_enc, W_dec, b_dec) = _dae_title(tmp_path_factory.mktemp("shard%d" % B), conf)
    mu, _h, _w = _dae_title(tmp_path_factory.mktemp("plain%d" % B), conf)
    pos, _o, _s = make_playlists(B, NT3, V3 - NT3, seed=5, seed_counts=(3, 9, 20))
    yo = np.ones(len(pos), np.float32)
    titles = _titles(B, L3, seed=6)
    seed = int(np.random.RandomState(1234).randint(0, 2 ** 31 - 1))        # the draw the unsharded train_step makes
    u_cost = mu.train_step(pos, yo, pos, yo, KP, IKP, titles=titles, title_keep_prob=TKP)
    u = {k: v.cpu().numpy() for k, v in mu.title_model._grads.items()}
    # float64 with the same draws (tests/test_gpu_title.py test_title_training_step_gradients_and_adam)
    xr, xc, xv = coo_to_csr(pos, yo, B, V3)
    x = dn.sparse_to_dense(pos, yo, B, V3)
    im = np.ones((B, V3))
    for r in range(B):
        cols = xc[xr[r]:xr[r + 1]]
        im[r, cols] = np.floor(np.float32(IKP) + _uniform(seed, 0, [r], cols)[0])
    hm = np.floor(np.float32(KP) + _uniform(seed, 1, range(B), range(H3)))
    _, _, z = dn.forward(x, W_enc, b_enc, W_dec, b_dec, input_keep_mask=im, ikp=IKP, hidden_keep_mask=hm, kp=KP)
    dae = 1.0 / (1.0 + np.exp(-z.astype(np.float64)))
    w_t, w_p = tn.mix_weights((x / IKP * im).sum(axis=1), IKP, np.ones(B))
    nf = len(FS3) * F3
    tm_mask = np.floor(np.float32(TKP) + _uniform(seed, 2, range(B), range(nf)))
    chain, carg = tn.features_f32_chain(titles, host, FS3)               # the kernels' own windows and ReLU decisions
    ref_cost, ref, info = tn.grads(titles, host, FS3, dae, x > 0, w_t, w_p, B, keep_mask=tm_mask, keep_prob=TKP,
                                   argmax=carg, gate=chain > 0)
    ref["dfeat"] = info["_aux"]["dfeat"]
    _CASES[B] = dict(m=m, csr=(xr, xc, xv), titles=titles, seed=seed, u_cost=u_cost, u=u, ref_cost=ref_cost, ref=ref, nf=nf)
    return _CASES[B]


@pytest.mark.parametrize("B", [37, 150])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_one_sharded_step_against_float64_and_unsharded(tmp_path_factory, world, B):
    import torch
    from spotify_recsys_challenge_2018_amd.sharding import HipTitleStages, all_shard_bounds
    c = _step_case(tmp_path_factory, B)
    m, seed, nf = c["m"], c["seed"], c["nf"]
    mt = m.title_model
    p = mt.p
    shape = dict(L=L3, n_char=mt.char_size, E=E3, filter_sizes=FS3, F=F3, ld=mt.ld)
    st = HipTitleStages(m.ctx, mt.ctx, m.weights["encoder_h"], m.biases["encoder_b"],
                        lambda lo, hi: m._ensure_packed(cols=(lo, hi)), shape)
    x = tuple(_dev(a) for a in c["csr"])
    d_titles = mt.titles_to_device(c["titles"], B)
    use = torch.ones(B, device="cuda")
    bounds = all_shard_bounds(V3, world)
    assert bounds[0][0] == 0 and bounds[-1][1] == V3 and all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
    sh = []
    for lo, hi in bounds:                                   # the shards one after another on the one GPU
        d = dict(gW=torch.zeros((hi - lo, mt.ld), device="cuda"), gb=torch.zeros(hi - lo, device="cuda"),
                 dfeat=torch.zeros((B, mt.ld), device="cuda"), cost=torch.zeros(1, device="cuda"))
        w_t, w_p, dae = st.dae_forward(x, use, lo, hi, KP, IKP, seed)
        feat, arg, raw = st.features(d_titles, p["char_embedding"], p["conv_w"], p["conv_b"], TKP, seed)
        WT_rows, b_rows = p["Output_WT"][lo:hi].contiguous(), p["Output_b"][lo:hi].contiguous()
        zt = st.logits(feat, WT_rows, b_rows, lo, hi)
        st.loss_backward(zt, dae, x, w_t, w_p, lo, hi, B, feat, WT_rows, d["gW"], d["gb"], d["dfeat"], d["cost"])
        d.update(arg=arg, raw=raw)
        sh.append(d)
    dfeat = sh[0]["dfeat"].clone()                          # the two all-reduces, in rank order
    cost_t = sh[0]["cost"].clone()
    for d in sh[1:]:
        dfeat += d["dfeat"]
        cost_t += d["cost"]
    for d in sh:                                            # the convolution backward on every rank
        d.update(g_emb=torch.zeros_like(p["char_embedding"]), g_cw=torch.zeros_like(p["conv_w"]),
                 g_cb=torch.zeros_like(p["conv_b"]))
        assert torch.equal(d["arg"], sh[0]["arg"]) and torch.equal(d["raw"], sh[0]["raw"])
        st.conv_backward(d_titles, p["char_embedding"], p["conv_w"], d["arg"], d["raw"], dfeat, TKP, seed,
                         d["g_emb"], d["g_cw"], d["g_cb"])
    torch.cuda.synchronize()
    for d in sh[1:]:                                        # no atomics in the gate / wgrad kernels: identical replicas
        assert torch.equal(d["g_cw"], sh[0]["g_cw"]) and torch.equal(d["g_cb"], sh[0]["g_cb"])
    cost = float(cost_t.item())
    got = {"Output_WT": torch.cat([d["gW"] for d in sh]).cpu().numpy(), "Output_b": torch.cat([d["gb"] for d in sh]).cpu().numpy(),
           "conv_w": sh[0]["g_cw"].cpu().numpy(), "conv_b": sh[0]["g_cb"].cpu().numpy(),
           "char_embedding": sh[0]["g_emb"].cpu().numpy()}      # (rank 0's: the broadcast)
    dfeat = dfeat.cpu().numpy()
    ref, u = c["ref"], c["u"]
    print("\nworld %d B %d: cost %.9g float64 %.9g unsharded %.9g" % (world, B, cost, c["ref_cost"], c["u_cost"]))
    tol = dict(rtol=2e-4, atol=2e-7)
    # (i) float64 with the same dropout masks
    assert abs(cost - c["ref_cost"]) <= 1e-5 * abs(c["ref_cost"])
    assert np.allclose(got["Output_WT"][:, :nf], ref["Output_W"].T, **tol) and not got["Output_WT"][:, nf:].any()
    assert np.allclose(got["Output_b"], ref["Output_b"], **tol)
    assert np.allclose(dfeat[:, :nf], ref["dfeat"], **tol) and not dfeat[:, nf:].any()
    assert np.allclose(got["conv_b"], np.concatenate([ref["Conv_b%d" % i] for i in range(len(FS3))]), **tol)
    assert np.allclose(got["conv_w"], np.concatenate([ref["Conv_W%d" % i].reshape(-1) for i in range(len(FS3))]), **tol)
    assert np.allclose(got["char_embedding"], ref["char_embedding"], **tol)
    # (ii) the unsharded DAE_title.train_step on the same inputs
    assert abs(cost - c["u_cost"]) <= 1e-5 * abs(c["u_cost"])
    for k in got:
        assert np.allclose(got[k], u[k], **tol), k
    if world == 1:                                          # the same launches on the same values: the same bits
        assert np.float32(cost) == np.float32(c["u_cost"])
        for k in ("Output_WT", "Output_b", "conv_w", "conv_b"):      # (char_embedding: title_egrad_kernel's atomics)
            assert np.array_equal(got[k].view(np.uint32), u[k].view(np.uint32)), k


# ---- 4. through the model -----------------------------------------------------------------------------------------------------

def test_sharded_model_trains_syncs_saves_and_scores(tmp_path):
    import random
    import torch
    from spotify_recsys_challenge_2018_amd.utils import data_reader as dr
    from test_gpu_title_feed import B_T, L_T, NA_T, NT_T, _title_conf, _write_titled_train
    _write_titled_train(str(tmp_path))
    random.seed(11); np.random.seed(11)
    reader = dr.data_reader(str(tmp_path), "train", B_T)
    m, _host, _w = _dae_title(tmp_path, _title_conf())
    plain, _h, _w2 = _dae_title(tmp_path, _title_conf())
    m.shard_title_training(0, 1)
    m.attach_train_set(reader)
    V = NT_T + NA_T
    pos, ones, seeds = make_playlists(B_T, NT_T, NA_T, seed=5, seed_counts=(3, 9, 20))
    yo = np.ones(len(pos), np.float32)
    titles = _titles(B_T, L_T, seed=6)
    dae_before = [a.copy() for a in m.get_params()]
    tv_before = m.title_model.get_params()
    costs = [m.train_step(pos, yo, pos, yo, 0.8, 0.75, titles=titles, title_keep_prob=0.8) for _ in range(3)]
    for _ in range(3):
        draw = reader.next_batch_draw()
        draw[1:] = -1
        costs.append(m.train_step_draw(draw, 2, 0.8, 0.75, title_keep_prob=0.8))
    assert np.isfinite(costs).all() and m._title_sharded.step == 6
    p_cost = plain.train_step(pos, yo, pos, yo, 0.8, 0.75, titles=titles, title_keep_prob=0.8)
    print("\nfirst cost sharded %.9g plain %.9g" % (costs[0], p_cost))
    assert abs(costs[0] - p_cost) <= 2e-6 * abs(p_cost)            # the same draws: the model's own dropout stream
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(m.get_params(), dae_before))
    m.sync_params()
    assert not m._title_stale
    tv = m.title_model.get_params()
    assert all(not np.array_equal(tv[k], tv_before[k]) for k in tv)      # every variable moved, and came back from the trainer
    path = str(tmp_path / "title.pkl")
    m.title_model.save(path)
    fresh, _h3, _w3 = _dae_title(tmp_path, _title_conf())
    fresh.title_model.load(path)
    use = (np.arange(B_T) % 3 != 0).astype(np.float32)
    i1, s1 = m.recommend(pos, ones, seeds, k=100, titles=titles, titles_use=use)
    i2, s2 = fresh.recommend(pos, ones, seeds, k=100, titles=titles, titles_use=use)
    assert np.array_equal(i1, i2) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
    # a step after the sync goes on from the trainer's state, and goes stale again
    m.train_step(pos, yo, pos, yo, 0.8, 0.75, titles=titles, title_keep_prob=0.8)
    assert m._title_stale and m._title_sharded.step == 7
    torch.cuda.synchronize()


def test_sharded_model_keeps_the_256_row_limit(tmp_path):
    conf = _conf(16, [3, 5], 40, 25, batch=300, n_input=1500, n_tracks=1200)
    m, _host, _w = _dae_title(tmp_path, conf)
    m.shard_title_training(0, 1)
    pos, ones, _s = make_playlists(300, 1200, 300, seed=5)
    before = m.title_model.get_params()
    with pytest.raises(ValueError, match=r"\[TITLE\] batch = 300"):
        m.train_step(pos, ones, pos, ones, 1.0, 1.0, titles=_titles(300, 25, seed=1))
    assert m._title_sharded.step == 0 and not m._title_stale
    after = m.title_model.get_params()
    assert all(np.array_equal(before[k], after[k]) for k in before)


# ---- 5. the driver under two gloo ranks on one device -------------------------------------------------------------------------

def _title_loss(log):
    return [float(l.split(":")[1]) for l in log.splitlines() if l.startswith("training loss")]


def test_two_rank_title_cli_on_one_device(tmp_path):
    import random
    from spotify_recsys_challenge_2018_amd import main as cli
    shutil.copytree(os.path.join(G, "data"), tmp_path / "data")
    ini = open(os.path.join(G, "config.ini")).read().replace("epochs = 2", "epochs = 1")
    (tmp_path / "dae").mkdir()
    open(tmp_path / "dae" / "config.ini", "w").write(ini)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:                                                    # the frozen DAE the title step reads (tests/test_gpu_train.py)
        random.seed(0); np.random.seed(0)
        assert cli.main(["--dir", "dae", "--pretrain"]) == 0
        assert cli.main(["--dir", "dae", "--dae"]) == 0
        # the one-rank run the two-rank loss is printed next to: the host RNG streams seeded as _init_distributed seeds
        # them on every rank, so both runs draw the same batches and keep-probabilities
        (tmp_path / "one").mkdir()
        open(tmp_path / "one" / "config.ini", "w").write(ini)
        shutil.copy(tmp_path / "dae" / "w_dae", tmp_path / "one" / "w_dae")
        random.seed(0); np.random.seed(0)
        assert cli.main(["--dir", "one", "--title"]) == 0
    finally:
        os.chdir(cwd)
    V = pickle.load(open(tmp_path / "dae" / "w_dae", "rb"))[0].shape[0]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k_ in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k_, None)
    # the two ranks: one child each, under a time limit of its own
    run = tmp_path / "two"
    run.mkdir()
    open(run / "config.ini", "w").write(ini)
    shutil.copy(tmp_path / "dae" / "w_dae", run / "w_dae")
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "spotify_recsys_challenge_2018_amd.main", "--dir", "two", "--title"]
    procs = []
    for r in range(2):
        e = dict(env, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                 MASTER_PORT=str(29950 + os.getpid() % 40), DAE_DIST_BACKEND="gloo")
        procs.append(subprocess.Popen(cmd, cwd=tmp_path, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            out = b"(no end within the time limit)"
        outs.append(out.decode()[-3000:])
        if p.returncode != 0:                               # one child failed: nothing else is started, the other ends
            for q in procs:
                if q.poll() is None:
                    q.kill()
                    q.wait()
            break
    assert [p.returncode for p in procs] == [0, 0], outs
    losses = {}
    for name, world in (("one", 1), ("two", 2)):
        log = open(tmp_path / name / "log.txt").read()
        assert ("title training sharded over 2 ranks" in log) == (world == 2)
        losses[name] = _title_loss(log)
        assert len(losses[name]) == 1 and np.isfinite(losses[name][0])
        assert "rprecision" in log
        tv = pickle.load(open(tmp_path / name / "graph" / "model.ckpt.pkl", "rb"))
        assert tv["Output_W"].shape == (400, V) and tv["Output_b"].shape == (V,) and tv["char_embedding"].shape == (41, 50)
        assert all(np.isfinite(a).all() for a in tv.values())
    # two summation orders over an epoch: printed, not asserted
    print("\n--title epoch loss: one rank %.9g, two ranks %.9g" % (losses["one"][0], losses["two"][0]))
