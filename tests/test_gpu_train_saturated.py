"""GPU (-m gpu): the training step where the loss head saturates -- logits far outside the band an untrained model keeps
(|z| < 8), against the reference that evaluates the head as fp32 does (oracle/dae_numpy.py fp32_head: per element the
interval of the loss term and of dz over every admissible fp32 sigmoid, folded into bf16_bounds / f32_bounds).

a. planted columns: a zero decoder row and a chosen bias make z the same known logit in every row, so gb_dec[v] is the sum
   of that column's dz and shows single elements; each planted column's gb_dec must lie in its interval, and where q = 0
   is admissible an all-negative column must sit on one of the discrete fp32 values.
b. spread weights: decoder rows of very different norms and positive biases (a trained-like spread of logits).
c. a model the library trained itself, one more step.
d. the planted case through the vocabulary-sharded stages, shard boundaries inside a run of saturated columns.
e. the title loss (dae_title_loss_backward) at saturated mixed scores, element by element.
The cases and their input conditions are in tests/test_train_saturated_reference_cpu.py (checked there without a device);
the kernel variants named there follow train.hip train_plan's rules."""
import numpy as np
import pytest

from oracle import dae_numpy as dn
from oracle import title_numpy as tn
from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.utils.synthetic import train_clustered_model
from test_gpu_train_bf16_ref import KEYS, _csr, _dev, check_bf16, check_f32, make_case, run_sharded, run_step
from test_train_saturated_reference_cpu import PLANTED, SHARD_EDGES, SPREAD, plant_layout, planted_case, title_case

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _both_steps(c):
    ctx = _lib.Context(0)
    try:
        b16 = run_step(ctx, c, _lib.DAE_DTYPE_BF16)
        f32 = run_step(ctx, c, _lib.DAE_DTYPE_F32)
    finally:
        ctx.close()
    return b16, f32


def check_planted(got, c, ref, bounds, name):
    """Per planted column: gb_dec[v] = sum over the B rows of dz[r, v] lies in the sum of the rows' intervals (hardware
    allowance included; each end rounded to bf16 where the step stores dz so), widened by the fp32 sum's 2 (B + 2) u
    sum|dz|.  An all-negative column whose interval contains q = 0 holds the same fp32 value in every row, so gb_dec / B
    must be one of the discrete admissible values (dn.head_candidates), not merely between them."""
    B, nb = c["B"], c["n_batch"]
    dz16 = ref["_aux"]["dz16"]
    rnd = dn.bf16_round if dz16 else (lambda a: a)
    worst, n_disc, rows = 0.0, 0, []
    for col, logit, kind in plant_layout(c["V"]):
        g = float(got["gb_dec"][col])
        lo_e, hi_e = rnd(bounds["dz_lo"][:, col]), rnd(bounds["dz_hi"][:, col])
        tol = 2 * (B + 2) * U * np.maximum(np.abs(lo_e), np.abs(hi_e)).sum()
        lo, hi = lo_e.sum() - tol, hi_e.sum() + tol
        assert np.isfinite(g), (name, col, logit, kind, g)
        mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
        ratio = abs(g - mid) / half if half > 0 else (0.0 if g == mid else np.inf)
        rows.append((ratio, col, logit, kind, g, lo, hi))
        worst = max(worst, ratio)
        if kind == "neg" and bounds["zero"][:, col].all():
            cands = dn.head_candidates(ref["_aux"]["z"][0, col], 0.0, nb, z_err=float(bounds["z_err"][:, col].max()))
            fits = []
            for m, _, d in cands:
                a = 2.0 ** -18 * abs(d)
                v_lo, v_hi = float(rnd(np.float64(d - a))), float(rnd(np.float64(d + a)))
                t = 2 * (B + 2) * U * B * max(abs(v_lo), abs(v_hi))
                fits.append(B * v_lo - t <= g <= B * v_hi + t)
            n_disc += 1
            assert any(fits), (name, "column %d (z = %g): gb_dec %.9g is none of the admissible fp32 values" % (col, logit, g),
                               [(m, B * d) for m, _, d in cands])
    bad = [r for r in rows if r[0] > 1.0]
    print("%s planted columns: %d, worst (gb_dec - mid) / half-width %.4f; %d on the discrete values"
          % (name, len(rows), worst, n_disc))
    assert not bad, (name, "column, logit, kind, gb_dec, lo, hi", [r[1:] for r in sorted(bad, reverse=True)[:8]])


@pytest.mark.parametrize("i", range(len(PLANTED)))
def test_planted_columns(i):
    V, nt, H, B, opt = PLANTED[i]
    c = planted_case(V, nt, H, B, opt)
    b16, f32 = _both_steps(c)
    for name, got in (("bf16", b16), ("fp32", f32)):
        assert np.isfinite(got["cost"]) and all(np.isfinite(got[k]).all() for k in KEYS), name
    _, ref, bounds = check_bf16(b16, c, head="fp32")
    check_planted(b16, c, ref, bounds, "bf16")
    _, ref, bounds = check_f32(f32, c, head="fp32")
    check_planted(f32, c, ref, bounds, "fp32")


@pytest.mark.parametrize("i", range(len(SPREAD)))
def test_spread_weights(i):
    V, nt, H, B, opt = SPREAD[i]
    c = make_case(V, nt, H, B, **opt)
    b16, f32 = _both_steps(c)
    check_bf16(b16, c, head="fp32")
    check_f32(f32, c, head="fp32")


@pytest.mark.parametrize("world", [2, 3])
def test_planted_columns_through_the_sharded_stages(world):
    """PLANTED[0]'s shape with a full wave of rows (B = 96) through HipTrainStages: every shard boundary of 2 and of 3
    shards lies inside a run of eight saturated columns."""
    V, nt, H, B = 2003, 1600, 256, 96
    c = planted_case(V, nt, H, B, dict())
    planted = {col for col, logit, _ in plant_layout(V) if logit >= 13.9}

    def boundaries_inside_a_saturated_run(bounds):
        for lo, _ in bounds[1:]:
            assert lo in SHARD_EDGES and {lo - 2, lo - 1, lo, lo + 1} <= planted, lo
    got = run_sharded(c, world, check_rows=boundaries_inside_a_saturated_run)
    _, ref, bounds = check_bf16(got, c, h_rel=2.0 ** -20, head="fp32")
    check_planted(got, c, ref, bounds, "bf16, %d shards" % world)


def logit_shares(z):
    return {"z > 9.2": float((z > 9.2).mean()), "z > 13.8": float((z > 13.8).mean()), "z > 16.7": float((z > 16.7).mean()),
            "max": float(z.max()), "min": float(z.min())}


@pytest.mark.parametrize("train_dtype", ["bf16", "f32"])
def test_one_more_step_of_a_model_the_library_trained(train_dtype):
    """train_clustered_model for 300 steps (V = 2 600, hidden 256), then one step on a fresh training_feed batch against the
    reference with the fp32 head.  Prints the share of the batch's logits above 9.2 / 13.8 / 16.7 (from the reference's
    float64 logits; DESIGN.md records them) and asserts nothing about it."""
    nt, na, H, B = 2000, 600, 256, 96
    V = nt + na
    W_enc, b_enc, W_dec, b_dec, gen, info = train_clustered_model(nt, na, H, steps=300, batch=128, seed=3, n_clusters=16,
                                                                  train_dtype=train_dtype)
    xp, xo, yp, yo = gen.training_feed(B, np.random.default_rng(77))
    x = dn.sparse_to_dense(xp, xo, B, V)
    y = dn.sparse_to_dense(yp, yo, B, V)
    c = make_case(V, nt, H, B, weights=(W_enc, b_enc, W_dec, b_dec), feed=(x, y))
    b16, f32 = _both_steps(c)
    _, ref, _ = check_bf16(b16, c, head="fp32")
    print("trained %s, %d steps, costs %s: logit shares %s" % (train_dtype, info["steps"], info["costs"],
                                                                logit_shares(ref["_aux"]["z"])))
    check_f32(f32, c, head="fp32")


def test_title_loss_at_saturated_mixed_scores():
    """dae_title_loss_backward on title_case(): title logits, DAE scores and mixing weights that put the mixed score yp at
    the saturation points, targets 0 and 1.  Output_WT is the identity (V = ld = 64), so dfeat IS dz, element by element;
    every element, gOutput_b's column sums and the cost lie in the intervals of tn.fp32_loss_head; nothing is NaN or inf."""
    import torch
    z, dae, y, wt, wp = title_case()
    B, V = z.shape
    nb = 40
    hd = tn.fp32_loss_head(z, dae, y, wt, wp, nb)
    yr, yc, yv = _csr(y)
    P = _lib._ptr
    ctx = _lib.Context(0)
    try:
        d = [_dev(a) for a in (z, dae, yr, yc, yv, wt, wp)]
        feat = torch.ones((B, V), device="cuda")
        WT = torch.eye(V, device="cuda")
        gw, gb = torch.zeros((V, V), device="cuda"), torch.zeros(V, device="cuda")
        dfeat, cost = torch.zeros((B, V), device="cuda"), torch.zeros(1, device="cuda")
        ctx.check(ctx.lib.dae_title_loss_backward(ctx.h, P(d[0]), V, P(d[1]), V, P(d[2]), P(d[3]), P(d[4]), P(d[5]), P(d[6]),
                                                  B, V, nb, P(feat), V, P(WT), P(gw), P(gb), P(dfeat), P(cost)))
        torch.cuda.synchronize()
        dz, gb, gw, cost = dfeat.cpu().numpy().astype(np.float64), gb.cpu().numpy(), gw.cpu().numpy(), float(cost.item())
    finally:
        ctx.close()
    assert np.isfinite(dz).all() and np.isfinite(gb).all() and np.isfinite(gw).all() and np.isfinite(cost)
    inside = (hd["dz_lo"] <= dz) & (dz <= hd["dz_hi"])
    print("title: %d elements, %d with q = 0 admissible, %d outside their interval" % (dz.size, hd["zero"].sum(), (~inside).sum()))
    bad = np.argwhere(~inside)
    assert inside.all(), [(int(r), int(v), float(z[r, v]), float(dae[r, v]), float(y[r, v]), float(wt[r]), float(wp[r]), dz[r, v],
                           hd["dz_lo"][r, v], hd["dz_hi"][r, v]) for r, v in bad[:6]]
    tol = 2 * (B + 2) * U * np.maximum(np.abs(hd["dz_lo"]), np.abs(hd["dz_hi"])).sum(axis=0)
    assert ((hd["dz_lo"].sum(axis=0) - tol <= gb) & (gb <= hd["dz_hi"].sum(axis=0) + tol)).all()
    assert np.allclose(gw, gb[:, None] * np.ones((1, V)), rtol=1e-6, atol=1e-30)          # f = 1: gOutput_WT rows repeat gOutput_b
    tot = np.maximum(np.abs(hd["L_lo"]), np.abs(hd["L_hi"])).sum()
    w = (z.size + 2) * U * tot / nb
    lo, hi = hd["L_lo"].sum() / nb - w, hd["L_hi"].sum() / nb + w
    print("title cost %.9g in [%.9g, %.9g]" % (cost, lo, hi))
    assert lo <= cost <= hi
