"""GPU (-m gpu): the kernel shapes dae_set_overlap_hint selects, against the oracle.

bench.py sets the hint on every context of its headline and exact-bf16 rows and dae_pipeline_create on every lane, so it
decides the kernels the published numbers and the drivers' loop run:
  1. the threshold sample of a bf16 / exact-bf16 call at hidden 256 with 128-row groups leaves the generic group-maxima kernel
     for decode_bf16_h256_wavemax_kernel on a grid of its own (8 or 16 workgroups per row group), gmax_per_wave 3 or -- waves w
     and w + 4 exchanging their maxima through LDS, the "pair" branch -- 4 (score_plan.h, the gA block);
  2. the exact mode's refine launch takes 256 threads instead of 512 (refine.hip);
  3. the bf16 candidate-list selection takes topk_kernel<PairSrc, 256> below 1 024 rows (score.hip prefer_small, topk.hip).
(2) and (3) have no cases of their own: every exact case here of fewer than 768 rows runs the slim refine shape and every bf16
case of fewer than 1 024 rows the 256-thread pair-list selection.  (The exact title mix's sample grid, mix_plan.h, is not
covered here: tests/test_gpu_title_exact_shapes.py runs it.)

Every case runs on a directly driven context with set_overlap_hint(4) and without, and checks
  the lists     bf16: oracle.topk over the device's own dense bf16 logits (dae_decode_dense on a context WITHOUT the hint),
                indices and score bits; exact bf16: the fp32 path's lists without the hint, bit for bit (themselves the
                oracle's over the dense fp32 logits), every launch audited, guard and audit silent -- a directly driven context
                has no fp32 fallback, so silent words mean the lists are the exact kernels' own; fp32: hint on == hint off;
  the threshold dae_score_topk_begin returns under the hint: tau <= the row's k-th largest ranked non-seed logit (dense bf16
                logits in bf16 mode, dense fp32 logits in exact mode, whose sample runs on b - eps), which is -inf where fewer
                than k such columns exist; finite wherever the row's rank k + n_seeds fits the maxima the sample leaves (every
                group of these shapes holds a whole ranked tile); and dae_score_topk_finish on that tau gives the same lists;
  the plan      last_plan() carries neither gA nor gmax_per_wave, so every case has a row in tests/golden/score_plans.txt
                (09_hint_<case>_{on,off}; tests/test_score_plan_cpu.py pins the planner to it): the row's inputs are this
                case's shape, its gA.nb_rg / wave_groups / gmax_per_wave / use_band words are the ones written down in CASES
                and the device's last_plan() equals its last eight words.  A planner change that moves a shape off its branch
                fails here or in the CPU test instead of leaving the case on another kernel.
Cases a - h are the shapes of the planner's branches on the repository's usual synthetic model (Xavier weights, Zipf bias).  On
that model every row's winners sit in the first tiles of the bias order and all rows hold nearly the same maxima, so two things
cannot show there: what waves 4 - 7 hand to waves 0 - 3 in the pair branch, and which row block a maximum is stored for.
Cases p and q use a model whose 32-row blocks rank different column sets first (P_P, P_Q below).
A threshold that is too LOW changes no list (it only lets more candidates through), and the tile order that defines the groups
is not visible through the ABI: tightness is not asserted (profiles/overlap_hint_tests_notes.md records the candidate counts)."""
import functools
import os

import numpy as np
import pytest

import oracle
from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.models.DAEs import coo_to_csr, seeds_to_csr
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights

pytestmark = pytest.mark.gpu
F32, BF, EX = _lib.DAE_DTYPE_F32, _lib.DAE_DTYPE_BF16, _lib.DAE_DTYPE_BF16_EXACT
U32 = np.uint32
H = 256
HOT_BIAS = 30.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_plans.txt")

# problem = (V, col_lo, n_tracks, B, hot, long_row, boost); the image is [col_lo, V)
#   hot:      the unranked columns of the last ranked tile and 300 artist columns behind them get b_dec = +30 -- should the
#             per-wave kernel's mask_from_col / ncols tests go wrong they enter a maximum and the threshold goes UP.  (Case a: the
#             partial last tile is made popular enough to be a sample tile, see _problem; case f ends on a whole tile.)
#   long_row: row 2 carries ~1 600 seeds, so that k + seeds > ld_g under the hint: its threshold is -inf and every ranked
#             column of the row goes through the 256-thread selection (bf16 only: the exact cases keep seeds <= 250)
P_A, P_A_LONG = (24000, 0, 20011, 129, True, False, None), (24000, 0, 20011, 129, True, True, None)
P_B = (20000, 0, 8192, 256, False, False, None)
P_C = (24000, 0, 20000, 256, False, False, None)
P_D = (40000, 0, 36000, 512, False, False, None)
P_E = (52000, 0, 49152, 900, False, False, None)
P_F = (48000, 20000, 40000, 256, True, False, None)
# boost = (first tile, tiles per set): ROW BLOCKS THAT RANK DIFFERENTLY.  Under the Zipf prior every row's winners sit in the first
# tiles of the bias order, which the per-wave kernel's waves 0 - 3 decode first: what waves 4 - 7 hand over in the pair branch
# never reaches a threshold, and all rows of a launch hold nearly the same maxima, so a mixed-up exchange or a store to another
# row block changes nothing.  Here the rows of 32-row block rb of a group (the kernel's row blocks) rank the columns of set rb
# first, by +8 on their logits (_problem), and the sets' biases fall with rb: maxima taken from another block raise the
# threshold of some block above its k-th logit.  (64, 16): set rb = tiles 64 + 16 rb .. + 15, the FIRST tiles of wave 4 + rb --
# every winner reaches its row through the exchange; (0, 32): set rb = the first tiles of waves 2 rb and 2 rb + 1.
P_P = (24000, 0, 20000, 256, False, False, (64, 16))
P_Q = (24000, 0, 20000, 256, False, False, (0, 32))
BOOST = 8.0

# plan = (gA.nb_rg, wave_groups, gmax_per_wave, use_band, ld_g or None where nothing is claimed)
GENERIC = (128, 0, 0, 0, None)
CASES = {
    # 313 sample tiles on 16 x 8 wave slots: pairs; the last ranked tile holds 11 ranked columns
    "a_bf16": dict(p=P_A_LONG, k=500, dtype=BF, off=(128, 0, 0, 0, 4096), on=(16, 1, 4, 0, 2048)),
    "a_exact": dict(p=P_A, k=500, dtype=EX, off=(128, 0, 0, 0, 4096), on=(16, 1, 4, 0, 2048)),
    # 128 sample tiles on 64 wave slots: every wave exactly two tiles
    "b_bf16": dict(p=P_B, k=100, dtype=BF, off=GENERIC, on=(8, 1, 4, 0, 1024)),
    "b_exact": dict(p=P_B, k=100, dtype=EX, off=GENERIC, on=(8, 1, 4, 0, 1024)),
    # k across the bounds of the pair branch (4 nbA 32 >= 4 k: k <= 512) and of the own sample grid (8 nbA 32 >= 4 k: k <= 640)
    "c512_bf16": dict(p=P_C, k=512, dtype=BF, off=GENERIC, on=(16, 1, 4, 0, 2048)),
    "c513_bf16": dict(p=P_C, k=513, dtype=BF, off=GENERIC, on=(16, 1, 3, 0, 4096)),
    "c640_bf16": dict(p=P_C, k=640, dtype=BF, off=GENERIC, on=(16, 1, 3, 0, 4096)),
    "c641_bf16": dict(p=P_C, k=641, dtype=BF, off=GENERIC, on=GENERIC),
    # four row groups, about 4 tiles per wave slot
    "d_exact": dict(p=P_D, k=500, dtype=EX, off=(64, 0, 0, 0, None), on=(8, 1, 3, 0, 2048)),
    # eight row groups (the last one of 4 rows), about 8 tiles per wave slot; without the hint the band-dealt list
    "e_bf16": dict(p=P_E, k=500, dtype=BF, off=(32, 0, 0, 1, None), on=(8, 1, 3, 0, None)),
    # a column shard: col_lo != 0, 20 000 ranked of 28 000 columns
    "f_bf16": dict(p=P_F, k=500, dtype=BF, off=GENERIC, on=(16, 1, 4, 0, None)),
    # winners that sit in the tiles of waves 4 - 7, other ones per row block: the pair exchange (k + seeds <= the 512 columns of
    # a set) and, q, the per-wave store without it (k + seeds <= 1 024)
    "p_bf16": dict(p=P_P, k=400, dtype=BF, off=GENERIC, on=(16, 1, 4, 0, 2048)),
    "p_exact": dict(p=P_P, k=400, dtype=EX, off=GENERIC, on=(16, 1, 4, 0, 2048)),
    "q_bf16": dict(p=P_Q, k=600, dtype=BF, off=GENERIC, on=(16, 1, 3, 0, 4096)),
    # fp32 and deep k: the hint leaves the plan alone
    "g_fp32": dict(p=P_C, k=500, dtype=F32, off=GENERIC, on=GENERIC),
    "h_bf16": dict(p=P_C, k=2048, dtype=BF, off=(128, 0, 1, 0, None), on=(128, 0, 1, 0, None)),
}
# the oracle ranks a problem once per arithmetic, at the largest k any of its cases asks for: a shorter list is its prefix
K_REF = {}
for _c in CASES.values():
    _key = (_c["p"], BF if _c["dtype"] == BF else F32)
    K_REF[_key] = max(K_REF.get(_key, 0), _c["k"])


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _golden():
    """tests/golden/score_plans.txt -> {name: (17 inputs, 34 plan words)} (the word order of tests/host/score_plan_main.cpp)."""
    rows = {}
    with open(GOLDEN) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            name, inputs, words = (s.strip() for s in line.split("|"))
            rows[name] = ([int(x) for x in inputs.split()], [int(x) for x in words.split()])
    return rows


def _plan_row(case, hint):
    """The case's row: its inputs are the case's shape, its branch words the ones CASES claims -> the row's last[8]."""
    c = CASES[case]
    V, lo, nt, B = c["p"][:4]
    inputs, w = _golden()["09_hint_%s_%s" % (case, "on" if hint else "off")]
    n_rg = (B + 127) // 128
    assert inputs[:5] == [(V - lo + 31) // 32, lo, V, H, 1 if c["dtype"] == F32 else 0], inputs
    assert inputs[5:8] == [128, n_rg, n_rg * 128] and inputs[11:] == [nt, c["k"], c["dtype"], 0, 1 if hint else 0, 1], inputs
    nb_rg, wave_groups, gmax, use_band, ld_g = c["on" if hint else "off"]
    assert (w[14], w[17], w[21], w[18]) == (nb_rg, wave_groups, gmax, use_band), (case, hint, w)
    assert ld_g is None or w[20] == ld_g, (case, hint, w)
    return dict(last=w[26:], ld_s=w[19], ld_g=w[20], gmax=gmax)


@functools.lru_cache(maxsize=None)
def _problem(V, lo, nt, B, hot, long_row, boost):
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=V % 97, bias="zipf", n_tracks=nt)
    if boost:
        return _boosted_problem(V, nt, B, boost, W_enc, b_enc, W_dec, b_dec)
    if hot:
        b_dec = b_dec.copy()
        last = lo + (nt - lo) // 32 * 32                  # first column of the last ranked tile, where that tile is a partial one
        b_dec[nt:lo + (nt - lo + 31) // 32 * 32 + 300] = HOT_BIAS
        # The sample is the n_samp tiles of the largest ranked bias (prepack.hip tile_order_kernel), and under the Zipf prior the
        # last ranked tile has the smallest: left alone it is never sampled and the kernels' partial-tile branch never runs.  Its
        # ranked columns take the biases of the image's most popular columns, which puts the tile second in the order.
        b_dec[last:nt] = b_dec[lo:lo + nt - last]
    pos, ones, seeds = make_playlists(B, nt, V - nt, seed=V % 97 + 1)
    rng = np.random.default_rng(V % 97 + 2)
    # row 1: 250 seeds, the image's 100 most popular columns (the row's likely winners) among them
    seeds[1] = np.unique(np.concatenate([lo + np.arange(100), rng.permutation(nt)[:150]]))[:250].tolist()
    if long_row:
        seeds[2] = np.unique(np.concatenate([np.arange(100), rng.permutation(nt)[:1500]])).tolist()
    rp, col, val = coo_to_csr(pos, ones, B, V)
    srp, sc = seeds_to_csr(seeds, B, nt)
    assert int(np.diff(srp).max()) <= 250 or long_row
    feed = tuple(_dev(a) for a in (rp, col, val, W_enc, b_enc))
    return dict(feed=feed, Wd=_dev(W_dec), bd=_dev(b_dec), srp=srp, sc=sc, d_srp=_dev(srp),
                d_sc=_dev(sc if sc.size else np.zeros(1, np.int32)), ref={})


def _block_of_row(B):
    return (np.arange(B) % 128) // 32


def _boosted_problem(V, nt, B, boost, W_enc, b_enc, W_dec, b_dec):
    """Row r holds ONE track, t_r with t_r % 4 = its row block; the encoder turns hidden unit c % 4 on for input c and every
    other unit off (sigmoid(+-12)); the decoder adds BOOST x unit u to the columns of set u and nothing else to any column.  The
    biases stay the Zipf prior's, so the tile order is the tile index.  Seeds: the row's track and r % 21 columns of its set."""
    first, count = boost
    rng = np.random.default_rng(V % 97 + 3)
    W_enc[:] = -12.0
    W_enc[np.arange(V), np.arange(V) % 4] = 12.0
    W_dec[:] = 0.0
    for u in range(4):
        W_dec[(first + count * u) * 32:(first + count * (u + 1)) * 32, u] = BOOST
    blk = _block_of_row(B)
    t = 4 * rng.integers(1500, nt // 4, B) + blk
    seeds = [[int(t[r])] + ((first + count * blk[r]) * 32 + rng.permutation(count * 32)[:r % 21]).tolist() for r in range(B)]
    rp, col, val = coo_to_csr(np.stack([np.arange(B), t], axis=1), np.ones(B, np.float32), B, V)
    srp, sc = seeds_to_csr(seeds, B, nt)
    feed = tuple(_dev(a) for a in (rp, col, val, W_enc, b_enc))
    return dict(feed=feed, Wd=_dev(W_dec), bd=_dev(b_dec), srp=srp, sc=sc, d_srp=_dev(srp), d_sc=_dev(sc), ref={})


def _reference(pkey, arith):
    """The oracle's ranking (scores, logits, indices at K_REF) of the device's dense logits of `arith` (BF or F32), decoded on a
    context of its own that never saw the hint.  Computed once per problem and arithmetic, read-only."""
    import torch
    p = _problem(*pkey)
    if arith not in p["ref"]:
        V, lo, nt, B = pkey[:4]
        c = _lib.Context(0)
        try:
            c.prepack_decoder(p["Wd"], p["bd"], lo, V, dtype=arith)
            h = torch.empty((B, H), device="cuda")
            c.encode(*p["feed"], h)
            z = torch.empty((B, V - lo), device="cuda")
            c.decode_dense(h, z, apply_sigmoid=False, dtype=arith)
            z = z.cpu().numpy()
        finally:
            c.close()
        K = K_REF[(pkey, arith)]
        # Columns below the row's (K + most seeds of a row)-th largest ranked logit cannot be among its K best non-seeds: they go
        # to the oracle as -inf, which it leaves out before its sort of the whole row (ties with that value stay in).
        zr, m = z[:, :nt - lo], K + int(np.diff(p["srp"]).max())
        assert m < zr.shape[1]
        floor = np.partition(zr, zr.shape[1] - m, axis=1)[:, zr.shape[1] - m]
        zr = np.where(zr >= floor[:, None], zr, np.float32(-np.inf))
        score, idx = oracle.topk(zr, K, p["srp"], p["sc"], col_base=lo)
        # the logit behind every list entry (-inf behind the padding of a short list)
        logit = np.where(idx >= 0, z[np.arange(B)[:, None], np.maximum(idx - lo, 0)], np.float32(-np.inf)).astype(np.float32)
        for a in (score, idx, logit):
            a.setflags(write=False)
        p["ref"][arith] = dict(score=score, idx=idx, logit=logit)
    return p["ref"][arith]


def _out(B, k):
    import torch
    return torch.full((B, k), 7.0, device="cuda"), torch.full((B, k), -7, dtype=torch.int32, device="cuda")


def _lists(c, p, nt, B, k, dtype):
    s, i = _out(B, k)
    c.score_topk(*p["feed"], nt, p["d_srp"], p["d_sc"], k, s, i, dtype=dtype)
    return s, i, c.last_plan()


def _same(got, want_score, want_idx):
    s, i = got[0].cpu().numpy(), got[1].cpu().numpy()
    return np.array_equal(i, want_idx) and np.array_equal(s.view(U32), np.ascontiguousarray(want_score, np.float32).view(U32))


def _check_call(c, case, hint, want):
    """One score_topk of the case on context c, hint as given: its lists are `want`, its plan the golden row's."""
    cs = CASES[case]
    V, lo, nt, B = cs["p"][:4]
    row = _plan_row(case, hint)
    c.set_overlap_hint(4 if hint else 0)
    s, i, plan = _lists(c, _problem(*cs["p"]), nt, B, cs["k"], cs["dtype"])
    assert list(plan.values()) == row["last"], (case, hint, plan, row["last"])
    assert _same((s, i), *want), (case, hint, plan)
    return s, i, row


@pytest.mark.parametrize("case", sorted(CASES))
def test_hinted_lists_thresholds_and_plan(case):
    import torch
    cs = CASES[case]
    pkey, k, dtype = cs["p"], cs["k"], cs["dtype"]
    V, lo, nt, B, _hot, long_row, boost = pkey
    p = _problem(*pkey)
    ref = _reference(pkey, BF if dtype == BF else F32)
    want = (ref["score"][:, :k], ref["idx"][:, :k])
    kth = ref["logit"][:, k - 1]                        # -inf where fewer than k ranked non-seed columns exist
    assert (want[1][:, k - 1] >= 0).all() and np.isfinite(kth).all()      # (no case here pads)
    if boost:                                           # every row's k winners are columns of its row block's set
        assert ((want[1] // 32 - boost[0]) // boost[1] == _block_of_row(B)[:, None]).all()
        assert (k + np.diff(p["srp"]) <= boost[1] * 32).all()
    c = _lib.Context(0)
    try:
        if dtype == EX:
            # the fp32 path without the hint: the lists the exact mode has to reproduce, themselves the oracle's
            c.prepack_decoder(p["Wd"], p["bd"], lo, V, dtype=F32)
            s32, i32, _plan = _lists(c, p, nt, B, k, F32)
            assert _same((s32, i32), *want)
            want = (s32.cpu().numpy(), i32.cpu().numpy())
            c.set_exact_audit(1, 16)
        c.prepack_decoder(p["Wd"], p["bd"], lo, V, dtype=dtype)
        if dtype == EX:
            c.exact_stats_read()
        stats = {}
        for hint in (0, 1):
            s, i, row = _check_call(c, case, hint, want)
            if dtype == EX:
                stats[hint] = c.exact_stats_read()
                assert stats[hint]["rows"] > 0                           # the refine launch ran
        if dtype == F32:
            assert _golden()["09_hint_%s_on" % case][1] == _golden()["09_hint_%s_off" % case][1]      # every plan word
        print("overlap hint case %s: plan words on %s off %s%s" % (
            case, _golden()["09_hint_%s_on" % case][1], _golden()["09_hint_%s_off" % case][1],
            "; exact stats on %s off %s" % (stats[1], stats[0]) if stats else ""))

        # the threshold itself, under the hint (still set)
        tau = torch.full((B,), 7.0, device="cuda")
        c.score_topk_begin(*p["feed"], nt, p["d_srp"], k, tau, dtype=dtype)
        s2, i2 = _out(B, k)
        c.score_topk_finish(tau, p["d_srp"], p["d_sc"], s2, i2)
        tau = tau.cpu().numpy()
        assert not np.isnan(tau).any() and (tau <= kth).all(), (case, np.flatnonzero(~(tau <= kth))[:8])
        # finite maxima of a row: all ld_g (every group holds a whole ranked tile), or -- gmax_per_wave 1: one slot per wave slot
        # and position -- the sample's elements
        n_fin = row["ld_g"] if row["gmax"] != 1 else min(row["ld_g"], row["ld_s"])
        rank = k + np.diff(p["srp"])
        assert np.isfinite(tau[rank <= n_fin]).all(), (case, np.flatnonzero(~np.isfinite(tau) & (rank <= n_fin))[:8])
        if long_row:
            assert rank[2] > n_fin and tau[2] == -np.inf                  # the case reaches the row without a threshold
        assert _same((s2, i2), *want), case
        if dtype == EX:
            assert c.exact_guard_read() == (0, -1)
            a = c.exact_audit_read()
            assert a["violations"] == 0 and a["audits"] >= 3, a
    finally:
        c.close()


def test_toggling_the_hint_on_one_context():
    """off -> on -> off -> on on ONE context, case e (without the hint the band-dealt list, with it none) and then case a, and e
    again without the hint after a's image took the slot: the band list cache (band_gen, band_nbrg, band_nsamp) and the tile
    order are keyed by what the hint and the image change, so stale reuse shows in the lists."""
    c = _lib.Context(0)
    try:
        for case in ("e_bf16", "a_bf16", "e_bf16"):
            cs = CASES[case]
            V, lo, nt, B = cs["p"][:4]
            p = _problem(*cs["p"])
            ref = _reference(cs["p"], BF)
            want = (ref["score"][:, :cs["k"]], ref["idx"][:, :cs["k"]])
            c.prepack_decoder(p["Wd"], p["bd"], lo, V, dtype=BF)
            for hint in (0, 1, 0, 1):
                _check_call(c, case, hint, want)
            _check_call(c, case, 0, want)
    finally:
        c.close()
