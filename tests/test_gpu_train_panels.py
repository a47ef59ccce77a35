"""GPU (-m gpu): the training step at batches above 256 rows (csrc/train.hip: the decode side of the step walks 256-row
panels; DESIGN.md "Batches above 256 rows").  The helpers and the tolerances are those of tests/test_gpu_train_bf16_ref.py --
fp32 against dn.grads at rtol 2e-4 / atol 2e-7 and cost 1e-5 relative, bf16 against dn.grads_bf16 under dn.bf16_bounds; every
term shrinks with 1 / n_batch, so more rows do not widen the absolute error.  On top of the references: the one call against
the sum of separate calls on its panels' rows, the armed decoder Adam bit for bit at B > 256, a 256-row step against hashes
recorded from the commit before the panels (tests/golden/train_panels_256.json), the model classes at batch 288, the sharded
stages, and the argument checks."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import dae_numpy as dn
from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights
import test_gpu_train as tg
from test_gpu_train_bf16_ref import KEYS, _csr, _dev, check_bf16, check_f32, make_case, reference, run_sharded, run_step

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = [pytest.param(_lib.DAE_DTYPE_F32, id="f32"), pytest.param(_lib.DAE_DTYPE_BF16, id="bf16")]


def _run(c, dtype):
    ctx = _lib.Context(0)
    try:
        return run_step(ctx, c, dtype)
    finally:
        ctx.close()


def _check(got, c, dtype):
    if dtype == _lib.DAE_DTYPE_BF16:
        check_bf16(got, c)
    else:
        check_f32(got, c)


# ---- 1. against the float64 references -------------------------------------------------------------------------------
CASES = [
    # V, nt, H, B, options                                           what it reaches
    (2001, 1600, 256, 257, dict(ikp=0.75, kp=0.8)),                  # a full panel + a panel of ONE row (B <= 64 K5); masks of row 256
    (2000, 1600, 256, 320, dict()),                                  # the 64 / 65 line of the second panel: 64 rows ...
    (2000, 1600, 256, 321, dict(kp=0.8)),                            # ... and 65
    (3000, 2400, 256, 512, dict(ikp=0.75, kp=0.8)),                  # two FULL panels
    (1500, 1200, 128, 600, dict(tied=True, lam=0.01)),               # three panels; tied: both gradients in one buffer; lambda once
    (20000, 16000, 256, 300, dict()),                                # more tiles than workgroups
    (33, 20, 256, 300, dict(kp=0.8)),                                # two vocabulary tiles, the second of one row
    (999, 800, 96, 300, dict(ikp=0.75, kp=0.8)),                     # grad_wdec_kernel<1>: bf16 forward, fp32 backward
    (1000, 800, 64, 260, dict()),                                    # grad_wdec_kernel<2>
    (3000, 2400, 384, 290, dict(tied=True)),                         # three hidden halves
    (2001, 1600, 256, 300, dict(n_batch=512)),                       # the mean divides by n_batch, not by B
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V,nt,H,B,opt", CASES, ids=["V%d-H%d-B%d" % (s[0], s[2], s[3]) for s in CASES])
def test_step_above_256_rows_against_the_references(V, nt, H, B, opt, dtype):
    c = make_case(V, nt, H, B, **opt)
    _check(_run(c, dtype), c, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_target_row_in_a_later_panel(dtype):
    """A target row of 1 025 entries at batch row 260: the fix-up's staging window (1 024) in the second panel."""
    V, nt, H, B = 3000, 2400, 256, 300
    c0 = make_case(V, nt, H, B)
    y = c0["y"].copy()
    y[260] = 0.0
    y[260, np.random.default_rng(9).choice(V, 1025, replace=False)] = 1.0
    c = make_case(V, nt, H, B, feed=(c0["x"], y))
    assert c["csr"][3][261] - c["csr"][3][260] == 1025
    _check(_run(c, dtype), c, dtype)


# ---- 2. additivity, with no reference involved -------------------------------------------------------------------------
def _rows(c, r0, r1):
    """Rows [r0, r1) of case c as a case of their own; n_batch stays the whole batch's."""
    x, y = c["x"][r0:r1], c["y"][r0:r1]
    return dict(c, B=r1 - r0, x=x, y=y, csr=_csr(x) + _csr(y))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V,nt,H,B", [(3000, 2400, 256, 512), (1500, 1200, 128, 600)])
def test_one_call_is_the_sum_of_its_panels(V, nt, H, B, dtype):
    """No dropout, no lambda: cost and the four gradients of the one call against the float64 sum of separate calls on rows
    [0, 256), [256, 512) (and [512, 600)), each with n_batch = B.  fp32: rtol 2e-4, atol 2e-7.  bf16: within the element-wise
    bound of the whole case (dn.bf16_bounds)."""
    c = make_case(V, nt, H, B)
    assert c["ikp"] == 1.0 and c["kp"] == 1.0 and c["lam"] == 0.0 and c["n_batch"] == B
    ctx = _lib.Context(0)
    try:
        one = run_step(ctx, c, dtype)
        parts = [run_step(ctx, _rows(c, r0, min(r0 + 256, B)), dtype) for r0 in range(0, B, 256)]
    finally:
        ctx.close()
    tot = {k: sum(p[k].astype(np.float64) for p in parts) for k in KEYS}
    cost = sum(p["cost"] for p in parts)
    print("cost %.9g, parts %.9g" % (one["cost"], cost))
    assert abs(one["cost"] - cost) <= 1e-5 * abs(cost)
    if dtype == _lib.DAE_DTYPE_BF16:
        ref = reference(c)
        r = dn.bf16_check(one, dict(ref, **tot), dn.bf16_bounds(ref))
        print("one call - sum of the parts, over the bound:", r)
        assert max(r.values()) <= 1.0, r
    else:
        for k in KEYS:
            assert np.allclose(one[k], tot[k], rtol=2e-4, atol=2e-7), k


# ---- 3. the armed decoder Adam at B > 256 --------------------------------------------------------------------------------
ARMED = [
    (3000, 2400, 256, 512),      # two FULL panels: the armed FULL instances read the first panel's gradient
    (3000, 2400, 256, 300),      # the last panel of 44 rows: the non-FULL t32 instances
    (3000, 2400, 128, 260),      # one hidden half; fp32: grad_wdec_kernel<4, 8, true> armed; a last panel of 4 rows
    (40, 30, 256, 290),          # two tiles of 32 decoder rows, the second with 8
    (3000, 2400, 384, 300),      # three hidden halves
]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("V,nt,H,B", ARMED, ids=["V%d-H%d-B%d" % (s[0], s[2], s[3]) for s in ARMED])
def test_armed_decoder_adam_is_bit_identical_above_256_rows(V, nt, H, B, bf16):
    """The body of tests/test_gpu_train.py test_armed_decoder_adam_is_bit_identical: W_dec / m / v carry the bits of "write
    gW_dec, then dae_adam_step"; cost, gb_enc, gb_dec bit-equal between the two runs; gW_enc within the float atomics."""
    tg.test_armed_decoder_adam_is_bit_identical(V, nt, H, B, bf16)


# ---- 4. a 256-row step is untouched --------------------------------------------------------------------------------------
def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def outputs_256(dtype, armed):
    """Hashes of what a step at (V, nt, H, B) = (3000, 2400, 256, 256) leaves: cost, gb_dec, gb_enc and gW_dec -- armed, W_dec /
    m / v after the update in its place.  gW_enc is left out: its atomics differ between any two runs."""
    import torch
    V, nt, H, B = 3000, 2400, 256, 256
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=4, bias="zipf", n_tracks=nt)
    pos, ones, _ = make_playlists(B, nt, V - nt, seed=6, seed_counts=(3, 9, 20))
    xr, xc, xv = tg.coo_to_csr(pos[pos[:, 1] < nt], ones[pos[:, 1] < nt], B, V)
    yr, yc, yv = tg.coo_to_csr(pos, np.ones(len(pos), np.float32), B, V)
    csr = [_dev(a) for a in (xr, xc, xv, yr, yc, yv)]
    rng = np.random.default_rng(1)
    m = _dev((rng.standard_normal((V, H)) * 1e-3).astype(np.float32))
    v = _dev((rng.random((V, H)) * 1e-6).astype(np.float32))
    d = dict(We=_dev(W_enc), be=_dev(b_enc), Wd=_dev(W_dec), bd=_dev(b_dec))
    out = dict(gWe=torch.zeros((V, H), device="cuda"), gbe=torch.zeros(H, device="cuda"), gWd=torch.zeros((V, H), device="cuda"),
               gbd=torch.zeros(V, device="cuda"), cost=torch.zeros(1, device="cuda"))
    P = _lib._ptr
    ctx = _lib.Context(0)
    try:
        ctx.set_train_dtype(dtype)
        if armed:
            ctx.check(ctx.lib.dae_arm_decoder_adam(ctx.h, P(m), P(v), 0.005, 0.9, 0.999, 1e-8, 7))
        ctx.check(ctx.lib.dae_train_forward_backward(
            ctx.h, P(csr[0]), P(csr[1]), P(csr[2]), P(csr[3]), P(csr[4]), P(csr[5]),
            P(d["We"]), P(d["be"]), P(d["Wd"]), P(d["bd"]), V, H, B, B, 0, 0.75, 0.8, 99, 0.0,
            P(out["gWe"]), P(out["gbe"]), None if armed else P(out["gWd"]), P(out["gbd"]), P(out["cost"])))
        torch.cuda.synchronize()
    finally:
        ctx.close()
    res = dict(cost=_sha(out["cost"]), gb_dec=_sha(out["gbd"]), gb_enc=_sha(out["gbe"]))
    if armed:
        res.update(W_dec=_sha(d["Wd"]), m=_sha(m), v=_sha(v))
    else:
        res.update(gW_dec=_sha(out["gWd"]))
    return res


def golden_key(dtype, armed):
    return "%s-%s" % ("bf16" if dtype == _lib.DAE_DTYPE_BF16 else "f32", "armed" if armed else "unarmed")


@pytest.mark.parametrize("armed", [False, True], ids=["unarmed", "armed"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_256_row_step_is_untouched(dtype, armed):
    """The bits of a 256-row step are those recorded from the commit before the panels, on the same device."""
    with open(os.path.join(G, "train_panels_256.json")) as f:
        want = json.load(f)[golden_key(dtype, armed)]
    assert outputs_256(dtype, armed) == want


# ---- 5. model level ----------------------------------------------------------------------------------------------------
class _C288:
    save = "/tmp/_panels_unused"; batch = 288; n_input = 1500; hidden = 64; lr = 0.01; reg_lambda = 0.0
    initval = "NULL"; n_tracks = 1200


def test_model_rows_adam_follows_dense_adam_at_batch_288():
    """tests/test_gpu_train.py test_model_rows_adam_follows_dense_adam at batch 288 (two panels), 24 steps: costs within
    rtol 2e-4, parameters within rtol 1e-3 / atol 2e-6."""
    from spotify_recsys_challenge_2018_amd.models.DAEs import DAE
    batches = []
    for s in range(6):
        pos, ones, _ = make_playlists(_C288.batch, 1200, 300, seed=100 + s, seed_counts=(3, 9, 20))
        batches.append((pos[pos[:, 1] < 1200], ones[pos[:, 1] < 1200], pos, np.ones(len(pos), np.float32)))
    a = DAE(_C288()); a.fit()
    cd = _C288(); cd.encoder_adam = "dense"
    b = DAE(cd); b.fit()
    assert a.encoder_adam == "rows" and b.encoder_adam == "dense"
    ca, cb = [], []
    for i in range(24):
        x, xv, y, yv = batches[i % len(batches)]
        ca.append(a.train_step(x, xv, y, yv, 0.8, 0.75))
        cb.append(b.train_step(x, xv, y, yv, 0.8, 0.75))
    assert a._lazy is not None and b._lazy is None
    assert np.all(np.isfinite(ca)) and ca[-1] < ca[0]
    assert np.allclose(ca, cb, rtol=2e-4)
    for pa, pb in zip(a.get_params(), b.get_params()):
        assert np.allclose(pa, pb, rtol=1e-3, atol=2e-6)
    a.ctx.close(); b.ctx.close()


def _draw_costs(device_feed):
    """Four steps at batch 288 from the draws of a reader over 400 synthetic playlists, through train_step_draw on the attached
    set or through the host feed rebuilt from the same draws.  Playlist i holds the tracks 3 i .. 3 i + 2 and one of 300
    artists; x is the tracks, so no three rows of a batch share an input column and the encoder gradient's atomics leave no
    run-to-run difference but a repeated playlist's two addends, whose sum does not depend on their order."""
    import random
    from spotify_recsys_challenge_2018_amd.models.DAEs import DAE
    from test_gpu_train_feed import _reader
    pls = [[[3 * i, 3 * i + 1, 3 * i + 2], [1200 + i % 300]] for i in range(400)]
    random.seed(3); np.random.seed(3)
    reader = _reader(pls, n_tracks=1200, n_items=1500, batch=_C288.batch)
    conf = _C288(); conf.init_seed = 5
    model = DAE(conf); model.fit()
    model.attach_train_set(reader)
    costs = []
    for _ in range(4):
        draw = reader.next_batch_draw()
        if device_feed:
            costs.append(model.train_step_draw(draw, 0, 0.8, 0.75))
        else:
            costs.append(model._host_feed_step(draw, 0, 0.8, 0.75, True))
    model._train_feed["set"].close()
    model.ctx.close()
    return np.asarray(costs, np.float64)


def test_train_step_draw_at_batch_288_equals_the_host_feed():
    host, dev = _draw_costs(False), _draw_costs(True)
    print("host", host, "device", dev)
    assert np.all(np.isfinite(dev)) and np.array_equal(dev, host)


def test_title_training_refuses_a_batch_above_256_before_any_launch(tmp_path):
    from test_gpu_title_shapes import _conf, _dae_title, _titles
    conf = _conf(25, [3, 5], 40, 25, batch=300)
    m, _host, _w = _dae_title(tmp_path, conf)
    pos, ones, _ = make_playlists(300, conf.n_tracks, conf.n_input - conf.n_tracks, seed=5, seed_counts=(3, 9, 20))
    with pytest.raises(ValueError, match=r"\[TITLE\] batch = 300"):
        m.train_step(pos, ones, pos, ones, 0.8, 0.75, titles=_titles(300, 25, 6))
    assert m.title_model._adam is None                       # nothing of the step was set up, nothing launched
    m.ctx.close()


# ---- 6. the sharded stages -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_stages_above_256_rows(world, dtype):
    """h comes from an all-reduced pre-activation there (not bit-exact), so under bf16 it may round either way near a
    midpoint: h_rel as in tests/test_gpu_train_bf16_ref.py."""
    c = make_case(2003, 1600, 256, 300)
    got = run_sharded(c, world, dtype=dtype)
    if dtype == _lib.DAE_DTYPE_BF16:
        check_bf16(got, c, h_rel=2.0 ** -20)
    else:
        check_f32(got, c)


# ---- 7. argument checks ------------------------------------------------------------------------------------------------------
def test_row_count_limits():
    c = make_case(64, 40, 32, 8)
    ctx = _lib.Context(0)
    try:
        with pytest.raises(_lib.DaeError, match="4096"):
            run_step(ctx, dict(c, B=4097), _lib.DAE_DTYPE_F32)
        with pytest.raises(_lib.DaeError):
            run_step(ctx, dict(c, B=0), _lib.DAE_DTYPE_F32)
    finally:
        ctx.close()


def test_sixteen_panels():
    """B = 4096 on a vocabulary of two tiles."""
    c = make_case(64, 40, 32, 4096)
    check_f32(_run(c, _lib.DAE_DTYPE_F32), c)
