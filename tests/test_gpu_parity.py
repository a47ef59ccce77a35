"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against the CPU oracle on
the same seeded inputs.  fp32 path: BIT-EXACT hidden activations, logits, top-k indices and scores
(tolerance 0).  See DESIGN.md "canonical order"."""
import numpy as np
import pytest

import oracle
from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.models.DAEs import coo_to_csr, seeds_to_csr
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _problem(V, n_tracks, H, B, seed=0, dist="zipf", bias="zeros"):
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=seed, bias=bias, n_tracks=n_tracks)
    b_enc = (np.random.default_rng(seed + 7).standard_normal(H) * 0.1).astype(np.float32)
    pos, ones, seeds = make_playlists(B, n_tracks, V - n_tracks, seed=seed + 1, dist=dist)
    rp, col, val = coo_to_csr(pos, ones, B, V)
    srp, sc = seeds_to_csr(seeds, B, n_tracks)
    return dict(W_enc=W_enc, b_enc=b_enc, W_dec=W_dec, b_dec=b_dec, rp=rp, col=col, val=val,
                srp=srp, sc=sc, seeds=seeds, V=V, H=H, B=B, n_tracks=n_tracks)


def _gpu_encode(ctx, p, ikp=1.0, kp=1.0, seed=0):
    import torch
    h = torch.empty((p["B"], p["H"]), dtype=torch.float32, device="cuda")
    ctx.encode(_dev(p["rp"]), _dev(p["col"] if p["col"].size else np.zeros(1, np.int32)),
               _dev(p["val"] if p["val"].size else np.zeros(1, np.float32)),
               _dev(p["W_enc"]), _dev(p["b_enc"]), h, ikp=ikp, kp=kp, seed=seed)
    return h


@pytest.mark.parametrize("V,nt,H,B", [(2000, 1500, 32, 8), (3000, 2500, 256, 37), (1111, 1000, 64, 130),
                                      (5000, 4000, 128, 200), (2048, 2048, 288, 5)])
def test_encode_bit_exact(ctx, V, nt, H, B):
    p = _problem(V, nt, H, B)
    h_gpu = _gpu_encode(ctx, p).cpu().numpy()
    h_ref = oracle.encode(p["rp"], p["col"], p["val"], p["W_enc"], p["b_enc"])
    assert np.array_equal(h_gpu.view(np.uint32), h_ref.view(np.uint32))


def test_encode_dropout_bit_exact(ctx):
    p = _problem(3000, 2500, 64, 50)
    h_gpu = _gpu_encode(ctx, p, ikp=0.75, kp=0.8, seed=1234).cpu().numpy()
    h_ref = oracle.encode(p["rp"], p["col"], p["val"], p["W_enc"], p["b_enc"], ikp=0.75, kp=0.8,
                          seed=1234)
    assert np.array_equal(h_gpu.view(np.uint32), h_ref.view(np.uint32))
    assert (h_gpu == 0).mean() > 0.1          # hidden dropout really dropped units


def test_encode_empty_rows(ctx):
    """Short final batches leave all-zero rows: h = sigmoid(b_enc)."""
    p = _problem(1000, 800, 32, 6)
    p["rp"][3:] = p["rp"][3]                   # rows 3.. empty
    h_gpu = _gpu_encode(ctx, p).cpu().numpy()
    h_ref = oracle.encode(p["rp"], p["col"], p["val"], p["W_enc"], p["b_enc"])
    assert np.array_equal(h_gpu.view(np.uint32), h_ref.view(np.uint32))
    assert np.array_equal(h_gpu[4], h_gpu[5])


@pytest.mark.parametrize("V,nt,H,B", [(2000, 1500, 32, 8), (3000, 2500, 256, 37), (1111, 1000, 64, 130),
                                      (4100, 4100, 256, 256), (2048, 2048, 288, 5), (700, 650, 96, 300)])
def test_decode_dense_bit_exact(ctx, V, nt, H, B):
    import torch
    p = _problem(V, nt, H, B)
    h = oracle.encode(p["rp"], p["col"], p["val"], p["W_enc"], p["b_enc"])
    ctx.prepack_decoder(_dev(p["W_dec"]), _dev(p["b_dec"]))
    out = torch.full((B, V + 3), 7.0, dtype=torch.float32, device="cuda")   # odd ld: scalar stores
    ctx.decode_dense(_dev(h), out, apply_sigmoid=False)
    z_ref = oracle.decode(h, p["W_dec"], p["b_dec"])
    o = out.cpu().numpy()
    assert np.array_equal(o[:, :V].view(np.uint32), z_ref.view(np.uint32))
    assert (o[:, V:] == 7.0).all()             # nothing written past the columns
    out4 = torch.empty((B, (V + 3) // 4 * 4), dtype=torch.float32, device="cuda")
    ctx.decode_dense(_dev(h), out4, apply_sigmoid=True)
    y_ref = oracle.decode(h, p["W_dec"], p["b_dec"], apply_sigmoid=True)
    assert np.array_equal(out4.cpu().numpy()[:, :V].view(np.uint32), y_ref.view(np.uint32))


def test_decode_dense_column_shard(ctx):
    import torch
    p = _problem(3000, 2500, 64, 40)
    h = oracle.encode(p["rp"], p["col"], p["val"], p["W_enc"], p["b_enc"])
    ctx.prepack_decoder(_dev(p["W_dec"]), _dev(p["b_dec"]), 777, 2222)
    out = torch.empty((40, 2222 - 777), dtype=torch.float32, device="cuda")
    ctx.decode_dense(_dev(h), out, apply_sigmoid=False)
    z_ref = oracle.decode(h, p["W_dec"], p["b_dec"], 777, 2222)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), z_ref.view(np.uint32))


def _check_topk(idx_g, sc_g, idx_r, sc_r):
    assert np.array_equal(idx_g, idx_r)
    assert np.array_equal(sc_g.view(np.uint32), sc_r.view(np.uint32))


@pytest.mark.parametrize("n,k,B", [(1500, 500, 9), (140, 500, 4), (5000, 10, 33), (40000, 500, 6),
                                   (513, 512, 3), (3000, 1024, 2)])
def test_topk_dense_bit_exact(ctx, n, k, B):
    import torch
    rng = np.random.default_rng(n + k)
    z = rng.standard_normal((B, n + 5)).astype(np.float32)
    z[:, ::7] = z[:, 1:2]                       # heavy ties, some across the cut
    seeds = [list(rng.integers(0, n, size=rng.integers(0, 120))) for _ in range(B)]
    srp, sc = seeds_to_csr(seeds, B, n)
    score = torch.empty((B, k), dtype=torch.float32, device="cuda")
    idx = torch.empty((B, k), dtype=torch.int32, device="cuda")
    ctx.topk_dense(_dev(z), n, 100, _dev(srp), _dev(sc + 100 if sc.size else np.zeros(1, np.int32)),
                   k, score, idx)
    sc_r, idx_r = oracle.topk(z, k, srp, sc + 100, col_base=100, ncols=n)
    _check_topk(idx.cpu().numpy(), score.cpu().numpy(), idx_r, sc_r)


def test_topk_adversarial_value_distributions(ctx):
    """The ordering histogram of the selection kernel bins the collected keys linearly in the logit: rows whose values
    defeat one binning or the other -- straddling zero with tiny magnitudes, 60 orders of magnitude wide (the span
    overflows: bit-pattern bins), constant, two far clusters (everything in one bin), denormals, -inf padding, one huge
    outlier -- must still come out in the oracle's order, scores bit for bit (logit output)."""
    import torch
    rng = np.random.default_rng(7)
    n, k = 3000, 500
    rows = []
    rows.append((rng.standard_normal(n) * 1e-38).astype(np.float32))                          # denormal-ish, both signs
    rows.append((rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(np.float32))   # 60 decades
    rows.append(np.full(n, -2.5, np.float32))                                                   # constant
    r = np.where(rng.random(n) < 0.5, 1e4, -1e4).astype(np.float32) + rng.standard_normal(n).astype(np.float32) * 1e-3
    rows.append(r.astype(np.float32))                                                           # two clusters
    r = (rng.standard_normal(n) * 0.01).astype(np.float32); r[17] = 3.0e38; rows.append(r)      # one outlier stretches the span
    r = rng.standard_normal(n).astype(np.float32); r[rng.random(n) < 0.9] = -np.inf; rows.append(r)   # < k finite values
    r = np.concatenate([np.zeros(n // 2, np.float32), -np.zeros(n - n // 2, np.float32)]); rows.append(r)   # +0 / -0
    r = (rng.standard_normal(n) * 0.5).astype(np.float32); r[::3] = r[0]; rows.append(r)        # straddling zero, heavy ties
    z = np.stack(rows)
    B = z.shape[0]
    seeds = [list(rng.integers(0, n, size=rng.integers(0, 50))) for _ in range(B)]
    srp, sc = seeds_to_csr(seeds, B, n)
    for kk in (k, 1024, 3):
        score = torch.empty((B, kk), dtype=torch.float32, device="cuda")
        idx = torch.empty((B, kk), dtype=torch.int32, device="cuda")
        ctx.topk_dense(_dev(z), n, 0, _dev(srp), _dev(sc if sc.size else np.zeros(1, np.int32)), kk, score, idx,
                       out_kind=_lib.DAE_OUT_LOGIT)
        sc_r, idx_r = oracle.topk(z, kk, srp, sc, out_kind=1)
        _check_topk(idx.cpu().numpy(), score.cpu().numpy(), idx_r, sc_r)


def test_topk_all_equal_and_saturated(ctx):
    """All logits equal (tie order = ascending column) and sigmoid-saturated logits."""
    import torch
    B, n, k = 3, 2000, 500
    z = np.zeros((B, n), np.float32)
    z[1] = 40.0                                  # sigmoid == 1.0f for the whole row
    z[2, :] = np.linspace(30, 31, n, dtype=np.float32)
    srp, sc = seeds_to_csr([[0, 1, 2], [5], []], B, n)
    score = torch.empty((B, k), dtype=torch.float32, device="cuda")
    idx = torch.empty((B, k), dtype=torch.int32, device="cuda")
    ctx.topk_dense(_dev(z), n, 0, _dev(srp), _dev(sc), k, score, idx)
    sc_r, idx_r = oracle.topk(z, k, srp, sc)
    _check_topk(idx.cpu().numpy(), score.cpu().numpy(), idx_r, sc_r)
    assert idx.cpu().numpy()[0, 0] == 3


@pytest.mark.parametrize("V,nt,H,B,k,dist,bias", [
    (2000, 1500, 32, 8, 500, "zipf", "zeros"),          # small: unfused inside the library
    (70000, 60000, 64, 40, 500, "zipf", "zipf"),        # fused: sample + filter + select
    (50000, 41000, 256, 130, 500, "uniform", "zeros"),  # hidden=256 unrolled body, 2 row groups
    (40000, 40000, 96, 300, 100, "zipf", "zipf"),
    (33000, 30000, 256, 256, 500, "zipf", "zipf"),
])
def test_decode_topk_fused_bit_exact(ctx, V, nt, H, B, k, dist, bias):
    import torch
    p = _problem(V, nt, H, B, dist=dist, bias=bias)
    h = oracle.encode(p["rp"], p["col"], p["val"], p["W_enc"], p["b_enc"])
    ctx.prepack_decoder(_dev(p["W_dec"]), _dev(p["b_dec"]))
    score = torch.empty((B, k), dtype=torch.float32, device="cuda")
    idx = torch.empty((B, k), dtype=torch.int32, device="cuda")
    sc = p["sc"] if p["sc"].size else np.zeros(1, np.int32)
    ctx.decode_topk(_dev(h), nt, _dev(p["srp"]), _dev(sc), k, score, idx)
    plan = ctx.last_plan()
    z_ref = oracle.decode(h, p["W_dec"], p["b_dec"], 0, nt)
    sc_r, idx_r = oracle.topk(z_ref, k, p["srp"], p["sc"])
    _check_topk(idx.cpu().numpy(), score.cpu().numpy(), idx_r, sc_r)
    if V >= 30000:
        assert plan["fused"] == 1, plan
    # no seed may be recommended (main_challenge.py:31-35)
    ig = idx.cpu().numpy()
    for r in range(B):
        assert not (set(p["seeds"][r]) & set(ig[r].tolist()))


def test_decode_topk_equals_unfused(ctx):
    """dae_decode_dense + dae_topk_dense == dae_decode_topk (include/dae_hip.h contract)."""
    import torch
    V, nt, H, B, k = 60000, 52000, 128, 64, 500
    p = _problem(V, nt, H, B, bias="zipf")
    h = _gpu_encode(ctx, p)
    ctx.prepack_decoder(_dev(p["W_dec"]), _dev(p["b_dec"]))
    s1 = torch.empty((B, k), dtype=torch.float32, device="cuda"); i1 = torch.empty((B, k), dtype=torch.int32, device="cuda")
    s2 = torch.empty_like(s1); i2 = torch.empty_like(i1)
    ctx.decode_topk(h, nt, _dev(p["srp"]), _dev(p["sc"]), k, s1, i1)
    z = torch.empty((B, V), dtype=torch.float32, device="cuda")
    ctx.decode_dense(h, z, apply_sigmoid=False)
    ctx.topk_dense(z, nt, 0, _dev(p["srp"]), _dev(p["sc"]), k, s2, i2)
    assert torch.equal(i1, i2) and torch.equal(s1, s2)


def test_wide_decoder_strided_order_bit_exact(ctx):
    """A prepacked decoder of more than ORDER_MAX_TILES = 8192 tiles (262 144 columns) orders its sample with
    tile_order_strided_kernel instead of the bias sort: the fused path must still equal the oracle bit for bit."""
    import torch
    V, nt, H, B, k = 300000, 290000, 32, 6, 100
    p = _problem(V, nt, H, B, seed=5, bias="zipf")
    h = _gpu_encode(ctx, p)
    ctx.prepack_decoder(_dev(p["W_dec"]), _dev(p["b_dec"]))
    score = torch.empty((B, k), dtype=torch.float32, device="cuda")
    idx = torch.empty((B, k), dtype=torch.int32, device="cuda")
    ctx.decode_topk(h, nt, _dev(p["srp"]), _dev(p["sc"]), k, score, idx)
    torch.cuda.synchronize()
    plan = ctx.last_plan()
    assert plan["fused"] == 1 and plan["n_tiles"] > 8192, plan
    z_ref = oracle.decode(h.cpu().numpy(), p["W_dec"], p["b_dec"], 0, nt)
    sc_r, idx_r = oracle.topk(z_ref, k, p["srp"], p["sc"])
    _check_topk(idx.cpu().numpy(), score.cpu().numpy(), idx_r, sc_r)


def test_topk_dense_lean_wide_range_bit_exact(ctx):
    """A ranked range too wide for the LDS seed bitmap takes the lean top-k mode.  At 2 M columns the bitmap alone is 250 KB,
    more than a CU's 160 KB of LDS: the bitmap mode cannot take this launch (it would fail with DAE_ERR_ARG), so a pass here is
    a lean pass."""
    import torch
    n, k, B = 2_000_000, 500, 3
    rng = np.random.default_rng(17)
    z = rng.standard_normal((B, n)).astype(np.float32)
    for r in range(B):                          # 100 ties at the value of rank 480: they straddle the cut (k + the seeds)
        z[r, 7::20011] = np.partition(z[r], n - 480)[n - 480]
    seeds = [list(rng.integers(0, n, size=150)) + list(np.argsort(-z[r])[:40]) for r in range(B)]   # (some of the best)
    srp, sc = seeds_to_csr(seeds, B, n)
    score = torch.empty((B, k), dtype=torch.float32, device="cuda")
    idx = torch.empty((B, k), dtype=torch.int32, device="cuda")
    ctx.topk_dense(_dev(z), n, 0, _dev(srp), _dev(sc), k, score, idx)
    sc_r, idx_r = oracle.topk(z, k, srp, sc)
    _check_topk(idx.cpu().numpy(), score.cpu().numpy(), idx_r, sc_r)


def test_topk_dense_lean_seed_scan_bit_exact(ctx):
    """Lean mode with more seeds than the sort buffer leaves room for (k + seeds = 1 100 > 1 024): the narrowing cannot run
    seed-blind, so every element is tested against the row's seed list instead.  One row over a range too wide for the bitmap."""
    import torch
    n, k, B = 1_200_000, 500, 1
    rng = np.random.default_rng(23)
    z = rng.standard_normal((B, n)).astype(np.float32)
    z[0, 11::30011] = np.partition(z[0], n - 490)[n - 490]      # ties at the value of rank 490: they straddle the cut
    best = np.argsort(-z[0])
    seeds = [list(best[:60]) + list(best[470:530:2]) + list(rng.choice(n, size=510, replace=False))]
    srp, sc = seeds_to_csr(seeds, B, n)
    assert srp[1] - srp[0] >= 600 - 90 and k + (srp[1] - srp[0]) > 1024      # (duplicates collapse: still past the sort buffer)
    score = torch.empty((B, k), dtype=torch.float32, device="cuda")
    idx = torch.empty((B, k), dtype=torch.int32, device="cuda")
    ctx.topk_dense(_dev(z), n, 0, _dev(srp), _dev(sc), k, score, idx)
    sc_r, idx_r = oracle.topk(z, k, srp, sc)
    _check_topk(idx.cpu().numpy(), score.cpu().numpy(), idx_r, sc_r)


def test_score_topk_many_short_rows_bit_exact(ctx):
    """1 024 rows over 6 000 ranked columns: the fused path (188 ranked tiles > the 128 SIMD slots of a row group's workgroups),
    whose final selection over the candidate lists runs with 256 threads per row at this many rows."""
    import torch
    V, nt, H, B, k = 6400, 6000, 32, 1024, 100
    p = _problem(V, nt, H, B, bias="zipf")
    ctx.prepack_decoder(_dev(p["W_dec"]), _dev(p["b_dec"]))
    score = torch.empty((B, k), dtype=torch.float32, device="cuda")
    idx = torch.empty((B, k), dtype=torch.int32, device="cuda")
    sc = p["sc"] if p["sc"].size else np.zeros(1, np.int32)
    ctx.score_topk(_dev(p["rp"]), _dev(p["col"]), _dev(p["val"]), _dev(p["W_enc"]), _dev(p["b_enc"]),
                   nt, _dev(p["srp"]), _dev(sc), k, score, idx)
    assert ctx.last_plan()["fused"] == 1, ctx.last_plan()
    s_ref, i_ref = oracle.score_batch(p["rp"], p["col"], p["val"], p["W_enc"], p["b_enc"], p["W_dec"],
                                      p["b_dec"], nt, nt, p["srp"], p["sc"], k)
    _check_topk(idx.cpu().numpy(), score.cpu().numpy(), i_ref, s_ref)


def test_shard_merge_bit_exact(ctx):
    """Column-sharded decode + K4 merge == unsharded, run on one GPU."""
    import torch
    V, nt, H, B, k, G = 64000, 50000, 64, 48, 500, 4
    p = _problem(V, nt, H, B, bias="zipf")
    h = _gpu_encode(ctx, p)
    srp, sc = _dev(p["srp"]), _dev(p["sc"])
    bounds = np.linspace(0, nt, G + 1).astype(int)
    cl = torch.empty((G, B, k), dtype=torch.float32, device="cuda")
    ci = torch.empty((G, B, k), dtype=torch.int32, device="cuda")
    for g in range(G):
        ctx.prepack_decoder(_dev(p["W_dec"]), _dev(p["b_dec"]), int(bounds[g]), int(bounds[g + 1]))
        ctx.decode_topk(h, nt, srp, sc, k, cl[g], ci[g], out_kind=_lib.DAE_OUT_LOGIT)
    s = torch.empty((B, k), dtype=torch.float32, device="cuda"); i = torch.empty((B, k), dtype=torch.int32, device="cuda")
    ctx.topk_merge(cl, ci, s, i)
    ctx.prepack_decoder(_dev(p["W_dec"]), _dev(p["b_dec"]))
    s0 = torch.empty_like(s); i0 = torch.empty_like(i)
    ctx.decode_topk(h, nt, srp, sc, k, s0, i0)
    assert torch.equal(i, i0) and torch.equal(s, s0)
    sm, im = oracle.topk_merge(cl.cpu().numpy(), ci.cpu().numpy())
    _check_topk(i.cpu().numpy(), s.cpu().numpy(), im, sm)


def test_errors_are_loud(ctx):
    import torch
    h = torch.zeros((4, 30), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.DaeError):
        ctx.encode(_dev(np.zeros(5, np.int32)), _dev(np.zeros(1, np.int32)), _dev(np.zeros(1, np.float32)),
                   torch.zeros((10, 30), device="cuda"), torch.zeros(30, device="cuda"), h)   # H % 4
    c2 = _lib.Context(0)
    with pytest.raises(_lib.DaeError):
        c2.decode_dense(torch.zeros((4, 32), device="cuda"), torch.zeros((4, 8), device="cuda"))  # no prepack
    c2.close()


@pytest.mark.parametrize("V,nt,H,B,k", [(50000, 41000, 256, 130, 500), (33000, 30000, 72, 77, 500),
                                        (2000, 1500, 32, 8, 100)])
def test_score_topk_fused_call_bit_exact(ctx, V, nt, H, B, k):
    """dae_score_topk == oracle (and == dae_encode + dae_decode_topk); H=72 exercises k padding."""
    import torch
    p = _problem(V, nt, H, B, bias="zipf")
    ctx.prepack_decoder(_dev(p["W_dec"]), _dev(p["b_dec"]))
    score = torch.empty((B, k), dtype=torch.float32, device="cuda")
    idx = torch.empty((B, k), dtype=torch.int32, device="cuda")
    sc = p["sc"] if p["sc"].size else np.zeros(1, np.int32)
    for _ in range(2):       # second call reuses the zero-padded image
        ctx.score_topk(_dev(p["rp"]), _dev(p["col"]), _dev(p["val"]), _dev(p["W_enc"]), _dev(p["b_enc"]),
                       nt, _dev(p["srp"]), _dev(sc), k, score, idx)
    s_ref, i_ref = oracle.score_batch(p["rp"], p["col"], p["val"], p["W_enc"], p["b_enc"], p["W_dec"],
                                      p["b_dec"], nt, nt, p["srp"], p["sc"], k)
    _check_topk(idx.cpu().numpy(), score.cpu().numpy(), i_ref, s_ref)


@pytest.mark.parametrize("V,nt,H,B,k", [(40, 20, 32, 1, 1), (31, 31, 32, 3, 500), (64, 64, 64, 2, 64),
                                        (5000, 5000, 512, 40, 500), (3000, 2000, 1024, 9, 1024)])
def test_edge_shapes_bit_exact(ctx, V, nt, H, B, k):
    """Tiny vocabularies (< one tile), k larger than the vocabulary, batch 1, hidden 512 / 1024."""
    import torch
    p = _problem(V, nt, H, B, bias="zipf")
    ctx.prepack_decoder(_dev(p["W_dec"]), _dev(p["b_dec"]))
    score = torch.empty((B, k), dtype=torch.float32, device="cuda")
    idx = torch.empty((B, k), dtype=torch.int32, device="cuda")
    sc = p["sc"] if p["sc"].size else np.zeros(1, np.int32)
    keep = [_dev(a) for a in (p["rp"], p["col"] if p["col"].size else np.zeros(1, np.int32),
                              p["val"] if p["val"].size else np.zeros(1, np.float32), p["W_enc"], p["b_enc"],
                              p["srp"], sc)]
    ctx.score_topk(keep[0], keep[1], keep[2], keep[3], keep[4], nt, keep[5], keep[6], k, score, idx)
    s_ref, i_ref = oracle.score_batch(p["rp"], p["col"], p["val"], p["W_enc"], p["b_enc"], p["W_dec"],
                                      p["b_dec"], nt, nt, p["srp"], p["sc"], k)
    _check_topk(idx.cpu().numpy(), score.cpu().numpy(), i_ref, s_ref)


def test_all_tracks_are_seeds_and_no_seeds(ctx):
    """Every track of the vocabulary is a seed -> nothing to recommend (all -1); and NULL seeds."""
    import torch
    V, nt, H, B, k = 300, 200, 32, 4, 50
    p = _problem(V, nt, H, B)
    seeds = [list(range(nt))] * 2 + [[], [5]]
    srp, sc = seeds_to_csr(seeds, B, nt)
    ctx.prepack_decoder(_dev(p["W_dec"]), _dev(p["b_dec"]))
    score = torch.empty((B, k), dtype=torch.float32, device="cuda")
    idx = torch.empty((B, k), dtype=torch.int32, device="cuda")
    keep = [_dev(a) for a in (p["rp"], p["col"], p["val"], p["W_enc"], p["b_enc"], srp, sc)]
    ctx.score_topk(keep[0], keep[1], keep[2], keep[3], keep[4], nt, keep[5], keep[6], k, score, idx)
    s_ref, i_ref = oracle.score_batch(p["rp"], p["col"], p["val"], p["W_enc"], p["b_enc"], p["W_dec"],
                                      p["b_dec"], nt, nt, srp, sc, k)
    _check_topk(idx.cpu().numpy(), score.cpu().numpy(), i_ref, s_ref)
    assert (idx.cpu().numpy()[:2] == -1).all() and np.isneginf(score.cpu().numpy()[:2]).all()
    h = torch.empty((B, H), device="cuda")
    ctx.encode(keep[0], keep[1], keep[2], keep[3], keep[4], h)
    ctx.decode_topk(h, nt, None, None, k, score, idx)                     # no seed lists at all
    z = oracle.decode(h.cpu().numpy(), p["W_dec"], p["b_dec"], 0, nt)
    s0, i0 = oracle.topk(z, k)
    _check_topk(idx.cpu().numpy(), score.cpu().numpy(), i0, s0)


def test_topk_dense_over_a_range_too_wide_for_the_seed_bitmap():
    """1.5 M ranked columns do not fit the LDS seed bitmap: the selection must fall back to its bitmap-free
    mode (seed-blind narrowing + removal) instead of failing, with the same answer as the oracle."""
    import torch
    ctx = _lib.Context(0)
    n, B, k = 1500000, 3, 500
    rng = np.random.default_rng(0)
    z = rng.standard_normal((B, n)).astype(np.float32)
    seeds = [list(map(int, np.argsort(-z[0])[:40])), [], [5, 7]]
    from spotify_recsys_challenge_2018_amd.models.DAEs import seeds_to_csr
    srp, sc = seeds_to_csr(seeds, B, n)
    d_z = torch.from_numpy(z).cuda()
    s = torch.empty((B, k), device="cuda"); i = torch.empty((B, k), dtype=torch.int32, device="cuda")
    ctx.topk_dense(d_z, n, 0, torch.from_numpy(srp).cuda(), torch.from_numpy(sc).cuda(), k, s, i, out_kind=_lib.DAE_OUT_LOGIT)
    s_ref, i_ref = oracle.topk(z, k, srp, sc, out_kind=1)
    assert np.array_equal(i.cpu().numpy(), i_ref) and np.array_equal(s.cpu().numpy().view(np.uint32), s_ref.view(np.uint32))
    ctx.close()


def test_batch_larger_than_a_row_slab_equals_row_wise_calls():
    """9 000 playlists in ONE call (the library walks them in slabs of 4096 rows) == the oracle on every row."""
    import torch
    ctx = _lib.Context(0)
    V, nt, H, B, k = 3000, 2500, 64, 9000, 50
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=2, bias="zipf", n_tracks=nt)
    pos, ones, seeds = make_playlists(B, nt, V - nt, seed=3)
    rp, col, val = coo_to_csr(pos, ones, B, V)
    srp, sc = seeds_to_csr(seeds, B, nt)
    d = [_dev(a) for a in (rp, col, val, W_enc, b_enc, W_dec, b_dec, srp, sc)]
    ctx.prepack_decoder(d[5], d[6])
    s = torch.empty((B, k), device="cuda"); i = torch.empty((B, k), dtype=torch.int32, device="cuda")
    ctx.score_topk(d[0], d[1], d[2], d[3], d[4], nt, d[7], d[8], k, s, i)
    s_ref, i_ref = oracle.score_batch(rp, col, val, W_enc, b_enc, W_dec, b_dec, V, nt, srp, sc, k)
    assert np.array_equal(i.cpu().numpy(), i_ref) and np.array_equal(s.cpu().numpy().view(np.uint32), s_ref.view(np.uint32))
    h = torch.empty((B, H), device="cuda")
    ctx.encode(d[0], d[1], d[2], d[3], d[4], h)
    s2 = torch.empty_like(s); i2 = torch.empty_like(i)
    ctx.decode_topk(h, nt, d[7], d[8], k, s2, i2)
    assert torch.equal(i2, i) and torch.equal(s2, s)
    ctx.close()


def test_scoring_step_is_capturable_in_a_hip_graph():
    """After one warm-up call (scratch allocated, kernel attributes set) a scoring step issues no allocation and
    no synchronisation, so it can be captured into a HIP graph and replayed with identical results."""
    import torch
    ctx = _lib.Context(0)
    V, nt, H, B, k = 40000, 33000, 256, 96, 500
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=0, bias="zipf", n_tracks=nt)
    pos, ones, seeds = make_playlists(B, nt, V - nt, seed=1)
    rp, col, val = coo_to_csr(pos, ones, B, V)
    srp, sc = seeds_to_csr(seeds, B, nt)
    d = [_dev(a) for a in (rp, col, val, W_enc, b_enc, W_dec, b_dec, srp, sc)]
    ctx.prepack_decoder(d[5], d[6])
    s = torch.empty((B, k), device="cuda"); i = torch.empty((B, k), dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx.bind_stream()
        for _ in range(2):
            ctx.score_topk(d[0], d[1], d[2], d[3], d[4], nt, d[7], d[8], k, s, i)
        torch.cuda.synchronize()
        ref_s, ref_i = s.clone(), i.clone()
        g = torch.cuda.CUDAGraph()
        g.capture_begin()
        ctx.score_topk(d[0], d[1], d[2], d[3], d[4], nt, d[7], d[8], k, s, i)
        g.capture_end()
    torch.cuda.synchronize()
    for _ in range(3):
        s.zero_(); i.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(i, ref_i) and torch.equal(s, ref_s)
    s_ref, i_ref = oracle.score_batch(rp, col, val, W_enc, b_enc, W_dec, b_dec, V, nt, srp, sc, k)
    assert np.array_equal(ref_i.cpu().numpy(), i_ref)
    del g
    ctx.close()


def test_decode_gate_alternates_two_contexts_without_changing_results():
    """dae_set_decode_gate: two contexts on two streams, each waiting for the other's dominant launch and announcing its
    own.  Many alternating steps must neither deadlock nor change a bit of the output; removing the gate works too."""
    import ctypes
    import torch
    V, nt, H, B, k = 40000, 33000, 256, 96, 500
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=0, bias="zipf", n_tracks=nt)
    pos, ones, seeds = make_playlists(B, nt, V - nt, seed=1)
    rp, col, val = coo_to_csr(pos, ones, B, V)
    srp, sc = seeds_to_csr(seeds, B, nt)
    d = [_dev(a) for a in (rp, col, val, W_enc, b_enc, W_dec, b_dec, srp, sc)]
    ctxs = [_lib.Context(0), _lib.Context(0)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [(torch.empty((B, k), device="cuda"), torch.empty((B, k), dtype=torch.int32, device="cuda")) for _ in ctxs]
    evs = []
    for c, st in zip(ctxs, streams):
        with torch.cuda.stream(st):
            c.bind_stream()
            c.prepack_decoder(d[5], d[6])
        ev = torch.cuda.Event(); ev.record(st); evs.append(ev)
    torch.cuda.synchronize()
    for i, c in enumerate(ctxs):
        c.check(c.lib.dae_set_decode_gate(c.h, ctypes.c_void_p(evs[1 - i].cuda_event), ctypes.c_void_p(evs[i].cuda_event)))
    for step in range(40):
        j = step % 2
        with torch.cuda.stream(streams[j]):
            ctxs[j].score_topk(d[0], d[1], d[2], d[3], d[4], nt, d[7], d[8], k, outs[j][0], outs[j][1])
    torch.cuda.synchronize()
    s_ref, i_ref = oracle.score_batch(rp, col, val, W_enc, b_enc, W_dec, b_dec, V, nt, srp, sc, k)
    for s, i in outs:
        assert np.array_equal(i.cpu().numpy(), i_ref)
        assert np.array_equal(s.cpu().numpy().view(np.uint32), s_ref.view(np.uint32))
    for c in ctxs:
        c.check(c.lib.dae_set_decode_gate(c.h, None, None))
    with torch.cuda.stream(streams[0]):
        ctxs[0].score_topk(d[0], d[1], d[2], d[3], d[4], nt, d[7], d[8], k, outs[0][0], outs[0][1])
    torch.cuda.synchronize()
    assert np.array_equal(outs[0][1].cpu().numpy(), i_ref)
    for c in ctxs:
        c.close()
