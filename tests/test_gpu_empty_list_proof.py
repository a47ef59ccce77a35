"""GPU (-m gpu): the threshold launch proves the filter launch's live list empty from the sample launch's {dq, tau_safe} pairs and
the envelope of the filter list, and then runs no arrival tail (tau_select.hip, csrc/empty_proof.h; DESIGN.md sections 2 and 4).

Lists, scores, thresholds, live counts and the three counters of dae_filter_skip_read cannot tell which path ran: they are
compared, bit for bit, with the skip off, with the halves (dae_score_topk_begin / _finish: the standalone live_tiles_kernel) and
with the C oracle.  dae_live_proof_read can: the row groups whose list was proved empty.

Shapes: those of tests/test_gpu_live_in_tau.py -- 30 000 tracks + 6 000 artists at hidden 256, k = 500, 469 filter tiles; the
popularity model (nothing live: every group proves) and b_dec = 0 (most tiles live: none does); 256 rows = two full groups, 130
= a second group of 2 rows whose second half group holds no row, 65 = one group with one row in its second half group."""
import numpy as np
import pytest

import oracle
from spotify_recsys_challenge_2018_amd import _lib
from test_gpu_live_in_tau import K, N_FILTER, NA, NT, _counters, _dev, _feed, _hidden, _model, _oracle_lists, _same_bits
from test_gpu_live_in_tau import _Scorer as _BaseScorer

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class _Scorer(_BaseScorer):
    """... and every call leaves the row groups proved empty in self.proved and the thresholds its filter launch took in self.tau."""

    def _result(self, s, i):
        r = super()._result(s, i)
        self.proved = self.ctx.live_proof_read()
        return r

    def score(self, feed, skip=True):
        r = super().score(feed, skip)
        self.tau = self.ctx.last_tau(feed[0].size - 1)
        return r

    def decode(self, h, srp, sc, skip=True, n_tracks=None):
        r = super().decode(h, srp, sc, skip, n_tracks)
        self.tau = self.ctx.last_tau(h.shape[0])
        return r

    def prepack(self, W_dec, b_dec):
        self.Wd, self.bd = _dev(W_dec), _dev(b_dec)
        self.ctx.prepack_decoder(self.Wd, self.bd, 0, self.V, dtype=self.dtype)


def _n_rg(B):
    return (B + 127) // 128


def _check_feed(sc, B, feed, h, ref, want_proved, what):
    """score, decode (h given) and the halves with the skip on, score with it off: lists and scores against `ref` and each other,
    the thresholds of every call against begin's, the live counts and counters against the halves' (the standalone kernel), and
    the groups proved: want_proved for the calls whose threshold launch builds the lists, 0 for the halves and the skip off."""
    n_rg = _n_rg(B)
    s_h, i_h, live_h, cnt_h, tau_h = sc.halves(feed)
    assert sc.proved == 0, "the halves proved a group"
    s_f, i_f, live_f, cnt_f = sc.score(feed)
    proved_f, tau_f = sc.proved, sc.tau
    on = [(s_f, i_f, live_f, cnt_f, proved_f, tau_f)]
    if h is not None:
        s_d, i_d, live_d, cnt_d = sc.decode(h, feed[3], feed[4])
        on.append((s_d, i_d, live_d, cnt_d, sc.proved, sc.tau))
    s_0, i_0, live_0, cnt_0 = sc.score(feed, skip=False)
    print("%s, B = %d: groups proved %s of %d, live %s (halves %s) of %d" % (what, B, [r[4] for r in on], n_rg, live_f, live_h, N_FILTER))
    assert sc.proved == 0 and live_0 == [] and cnt_0["launches"] == 0
    assert np.array_equal(_bits(sc.tau), _bits(tau_h)), "the skip moves the thresholds"
    assert _same_bits(s_0, i_0, *ref) and _same_bits(s_h, i_h, *ref)
    assert len(live_h) == n_rg and cnt_h == _counters(n_rg, N_FILTER, live_h), (live_h, cnt_h)
    for s, i, live, cnt, proved, tau in on:
        assert _same_bits(s, i, *ref) and _same_bits(s, i, s_0, i_0)
        assert np.array_equal(_bits(tau), _bits(tau_h)), "thresholds moved"
        assert live == live_h and cnt == cnt_h, (live, live_h, cnt, cnt_h)
        assert proved == want_proved, (proved, want_proved)
    return live_h


def _check_decode(sc, h, srp, scol, ref, what):
    """Hidden rows given by the caller: against the skip off (and `ref`, where the oracle has an answer) -> (live, groups proved)."""
    n_rg = _n_rg(h.shape[0])
    s1, i1, live, cnt = sc.decode(h, srp, scol)
    proved, tau1 = sc.proved, sc.tau
    s0, i0, live0, cnt0 = sc.decode(h, srp, scol, skip=False)
    print("%s: groups proved %d of %d, live %s of %d" % (what, proved, n_rg, live, N_FILTER))
    assert sc.proved == 0 and live0 == [] and cnt0["launches"] == 0
    assert np.array_equal(_bits(tau1), _bits(sc.tau)), "thresholds moved"
    assert _same_bits(s1, i1, s0, i0)
    if ref is not None:
        assert _same_bits(s1, i1, *ref)
    assert len(live) == n_rg and cnt == _counters(n_rg, N_FILTER, live), (live, cnt)
    return live, proved


# ---- 1. the popularity model: every group with a real row proves ------------------------------------------------------------------
@pytest.mark.parametrize("Hh", [256, 252])
@pytest.mark.parametrize("B", [256, 130, 65])
def test_popularity_model_every_group_proved(B, Hh):
    sc = _Scorer(NT, NA, *_model(NT, NA, "zipf", Hh))
    live = _check_feed(sc, B, _feed(B, NT, NA), _hidden(B, NT, NA, "zipf", Hh), _oracle_lists(B, NT, NA, "zipf", Hh), _n_rg(B),
                       "popularity model, hidden %d" % Hh)
    sc.close()
    assert live == [0] * _n_rg(B)


# ---- 2. b_dec = 0: no group proves, the arrival tail builds the lists ----------------------------------------------------------------
@pytest.mark.parametrize("B", [256, 130])
def test_bias_zeros_nothing_proved(B):
    sc = _Scorer(NT, NA, *_model(NT, NA, "zeros"))
    live = _check_feed(sc, B, _feed(B, NT, NA), _hidden(B, NT, NA, "zeros"), _oracle_lists(B, NT, NA, "zeros"), 0, "b_dec = 0")
    sc.close()
    assert all(0 < n < N_FILTER for n in live), live


# ---- 3. d = 0.5: the grid's last point -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", ["zipf", "zeros"])
@pytest.mark.parametrize("B", [256, 130])
def test_hidden_rows_at_zero_and_one(B, bias):
    _, _, W_dec, b_dec = _model(NT, NA, bias)
    h = (np.random.default_rng(3).random((256, 256)) < 0.5).astype(np.float32)[:B]
    _, _, _, srp, scol = _feed(B, NT, NA)
    sc = _Scorer(NT, NA, *_model(NT, NA, bias))
    live, proved = _check_decode(sc, h, srp, scol, oracle.topk(oracle.decode(h, W_dec, b_dec, 0, NT), K, srp, scol),
                                 "hidden rows in {0, 1}, bias %s" % bias)
    sc.close()
    if bias == "zipf":
        assert proved == _n_rg(B) and live == [0] * _n_rg(B), (proved, live)
    else:
        assert proved == 0 and live == [N_FILTER] * _n_rg(B), (proved, live)


# ---- 4. one launch with both paths ------------------------------------------------------------------------------------------------
def test_one_launch_with_a_proved_group_and_an_arriving_one():
    """The encoder of test_gpu_live_in_tau.py's "one live tile for one row": rows at 0.5 except the last, which sits at 1 on the
    positive weights of column c*.  Group 0 (d = 0) proves; group 1 (two rows, d = 0.5) keeps the tile of c* and must take the
    arrival tail."""
    B, c_star = 130, NT - 10
    _, b_enc, W_dec, b_dec = _model(NT, NA, "zipf")
    W_dec = W_dec.copy()
    w = W_dec[c_star].astype(np.float64)
    s_all, s_pos = w.sum(), w[w > 0].sum()
    alpha = 2.0 * (3.0 - float(b_dec[c_star])) / (s_all + s_pos)
    W_dec[c_star] = (W_dec[c_star] * np.float32(alpha)).astype(np.float32)
    assert float(b_dec[c_star]) + 0.5 * alpha * s_all < -6.0
    feed = _feed(B, NT, NA)
    rp, col, val, srp, scol = feed
    c_feed = max(set(col[rp[B - 1]:rp[B]].tolist()) - set(col[:rp[B - 1]].tolist()))
    W_enc = np.zeros((NT + NA, 256), np.float32)
    W_enc[c_feed, W_dec[c_star] > 0] = 1.0e4
    h = oracle.encode(rp, col, val, W_enc, b_enc)
    assert (h[:B - 1] == 0.5).all() and set(np.unique(h[B - 1]).tolist()) == {0.5, 1.0}
    ref = oracle.topk(oracle.decode(h, W_dec, b_dec, 0, NT), K, srp, scol)
    sc = _Scorer(NT, NA, W_enc, b_enc, W_dec, b_dec)
    live = _check_feed(sc, B, feed, h, ref, 1, "one live tile for one row")
    sc.close()
    assert live[0] == 0 and 1 <= live[1] < N_FILTER, live


def test_the_envelope_entry_is_the_grid_point_at_or_above_d():
    """One tile whose bound crosses the thresholds between two neighbouring grid points.  Column c* gets weights +5 on half the
    units and -5 on the others (sum 0, M_t about 1 280: the bound rises by 2.5 per grid step) and keeps its bias of about -8.5; every
    row sits at 0.5 except the last, which sits at 0.5 +- 2/512 with the signs of c*'s weights: d = d_2 exactly, c*'s logit about
    -3.5 against thresholds about -4.6.  Group 0 (d = 0) proves from G[0], about -7.7.  Group 1 must take G[2], about -3.5, and
    not prove; G[1], about -6, would prove it and lose the tile of c*."""
    B, c_star = 130, 29970
    W_enc, b_enc, W_dec, b_dec = _model(NT, NA, "zipf")
    W_dec = W_dec.copy()
    sign = np.where(np.arange(256) % 2 == 0, 1.0, -1.0).astype(np.float32)
    W_dec[c_star] = 5.0 * sign
    assert -9.0 < float(b_dec[c_star]) < -7.5
    h = np.full((B, 256), 0.5, np.float32)
    h[B - 1] = 0.5 + sign * np.float32(2.0 / 512.0)
    _, _, _, srp, scol = _feed(B, NT, NA)
    ref = oracle.topk(oracle.decode(h, W_dec, b_dec, 0, NT), K, srp, scol)
    assert c_star in ref[1][B - 1] and not (ref[1][:B - 1] == c_star).any()
    sc = _Scorer(NT, NA, W_enc, b_enc, W_dec, b_dec)
    live, proved = _check_decode(sc, h, srp, scol, ref, "a bound that crosses tau between d_1 and d_2")
    sc.close()
    assert live[0] == 0 and 1 <= live[1] < N_FILTER and proved == 1, (live, proved)


# ---- 5. no proof for rows outside [0, 1] and for a NaN ----------------------------------------------------------------------------
def test_hidden_rows_outside_the_unit_interval():
    """d > 0.5 in both groups: the grid ends at 0.5, so neither proves, whatever the tail then finds."""
    B = 130
    h = _hidden(B, NT, NA, "zipf").copy()
    h[5, 7] = 1.25
    h[129, 3] = -0.5
    _, _, W_dec, b_dec = _model(NT, NA, "zipf")
    _, _, _, srp, scol = _feed(B, NT, NA)
    sc = _Scorer(NT, NA, *_model(NT, NA, "zipf"))
    live, proved = _check_decode(sc, h, srp, scol, oracle.topk(oracle.decode(h, W_dec, b_dec, 0, NT), K, srp, scol), "d > 0.5 in both groups")
    sc.close()
    assert proved == 0, proved


def test_a_nan_in_one_hidden_row():
    """Row 70: its group has no proof (D is a NaN) and its tail keeps every tile; the other group proves."""
    B = 256
    h = _hidden(B, NT, NA, "zipf").copy()
    h[70, 17] = np.nan
    _, _, _, srp, scol = _feed(B, NT, NA)
    sc = _Scorer(NT, NA, *_model(NT, NA, "zipf"))
    live, proved = _check_decode(sc, h, srp, scol, None, "NaN in row 70")
    sc.close()
    assert live == [N_FILTER, 0] and proved == 1, (live, proved)


def test_the_pairs_are_stored_by_a_workgroup_that_decodes_nothing():
    """Workgroup 0 of a half group stores the pair, and it may be one that skips all its tiles and ends early.  The model: the
    popularity model with the weights of its most popular tile at -0.2 (logits about b - 25: the first item of workgroup 0 is
    skipped as its other three are).  Call 1 leaves NaN pairs in the context (a NaN row in every half group: nothing skips,
    nothing proves); call 2, clean rows on the same context, must store its own and prove both groups."""
    B = 130
    W_enc, b_enc, W_dec, b_dec = _model(NT, NA, "zipf")
    W_dec = W_dec.copy()
    t0 = int(np.argmax(b_dec[:NT])) // 32
    W_dec[t0 * 32:(t0 + 1) * 32] = -0.2
    h = _hidden(B, NT, NA, "zipf")
    h_nan = h.copy()
    h_nan[[0, 64, 128], 5] = np.nan
    _, _, _, srp, scol = _feed(B, NT, NA)
    sc = _Scorer(NT, NA, W_enc, b_enc, W_dec, b_dec)
    live1, proved1 = _check_decode(sc, h_nan, srp, scol, None, "a NaN row in every half group")
    live2, proved2 = _check_decode(sc, h, srp, scol, oracle.topk(oracle.decode(h, W_dec, b_dec, 0, NT), K, srp, scol),
                                   "clean rows behind them, workgroup 0 skipping every tile")
    sc.close()
    assert live1 == [N_FILTER, N_FILTER] and proved1 == 0, (live1, proved1)
    assert live2 == [0, 0] and proved2 == 2, (live2, proved2)


# ---- 6. the envelope follows the tile order -----------------------------------------------------------------------------------------
def test_one_context_prepacked_again():
    """Popularity model, b_dec = 0, popularity model on ONE context: an envelope left over from the first image would prove the
    second's groups empty (wrong live counts, wrong lists)."""
    B = 256
    feed = _feed(B, NT, NA)
    ref_sc = _Scorer(NT, NA, *_model(NT, NA, "zeros"))
    want = ref_sc.halves(feed)
    ref_sc.close()
    sc = _Scorer(NT, NA, *_model(NT, NA, "zipf"))
    seen = []
    for bias in ("zipf", "zeros", "zipf"):
        if seen:
            sc.prepack(*_model(NT, NA, bias)[2:])
        s, i, live, cnt = sc.score(feed)
        seen.append((bias, live, sc.proved))
        assert _same_bits(s, i, *_oracle_lists(B, NT, NA, bias)), bias
        assert cnt == _counters(2, N_FILTER, live)
        if bias == "zeros":
            assert live == want[2] and sc.proved == 0, (live, want[2], sc.proved)
        else:
            assert live == [0, 0] and sc.proved == 2, (live, sc.proved)
    sc.close()
    print("one context, three images: %s" % seen)


# ---- 7. changing row counts, the two models alternating ---------------------------------------------------------------------------
def test_one_context_through_changing_row_counts_and_models():
    """256 (popularity) -> 130 (b_dec = 0) -> 65 (popularity) -> 256 (b_dec = 0), nothing reset, the counters read at the end only:
    the proved path leaves the arrival counters alone, so the last call's groups fire exactly when their last row arrives."""
    ref_sc = _Scorer(NT, NA, *_model(NT, NA, "zeros"))
    want = {B: ref_sc.halves(_feed(B, NT, NA)) for B in (130, 256)}
    ref_sc.close()
    sc = _Scorer(NT, NA, *_model(NT, NA, "zipf"))
    planned = live_sum = 0
    steps = ((256, "zipf"), (130, "zeros"), (65, "zipf"), (256, "zeros"))
    for n, (B, bias) in enumerate(steps):
        if n:
            sc.prepack(*_model(NT, NA, bias)[2:])
        d = [_dev(a) for a in _feed(B, NT, NA)]
        s, i = sc._out(B)
        sc.ctx.set_filter_skip(True)
        sc.ctx.score_topk(d[0], d[1], d[2], sc.We, sc.be, NT, d[3], d[4], K, s, i)
        live = sc.ctx.filter_skip_last()
        assert _same_bits(s.cpu().numpy(), i.cpu().numpy(), *_oracle_lists(B, NT, NA, bias)), (B, bias)
        assert live == ([0] * _n_rg(B) if bias == "zipf" else want[B][2]), (B, bias, live)
        planned += _n_rg(B) * N_FILTER
        live_sum += sum(live)
    cnt, proved = sc.ctx.filter_skip_read(), sc.ctx.live_proof_read()
    sc.close()
    assert cnt == {"launches": 4, "planned": planned, "live": live_sum}, cnt
    assert proved == 2 + 0 + 1 + 0, proved


# ---- 8. two contexts, one image, two streams ------------------------------------------------------------------------------------
def test_two_contexts_on_two_streams_interleaved():
    import torch
    m = _model(NT, NA, "zipf")
    solo = _Scorer(NT, NA, *m)
    shapes = (256, 130, 65)
    want = {B: solo.score(_feed(B, NT, NA)) for B in shapes}
    feeds = {B: [_dev(a) for a in _feed(B, NT, NA)] for B in shapes}
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    guests = []
    for st in streams:
        with torch.cuda.stream(st):
            guests.append(_Scorer(NT, NA, *m, share_from=solo))        # (a context binds the stream current at its creation)
    n_calls = 18
    outs = [[], []]
    for n in range(n_calls):
        for g, (st, sc) in enumerate(zip(streams, guests)):
            B = shapes[(n + g) % 3]                                    # the two streams run different row counts side by side
            d = feeds[B]
            with torch.cuda.stream(st):
                s, i = sc._out(B)
                sc.ctx.score_topk(d[0], d[1], d[2], sc.We, sc.be, NT, d[3], d[4], K, s, i)
            outs[g].append((B, s, i))
    torch.cuda.synchronize()
    for g, sc in enumerate(guests):
        for B, s, i in outs[g]:
            assert _same_bits(s.cpu().numpy(), i.cpu().numpy(), want[B][0], want[B][1]), (g, B)
            assert _same_bits(want[B][0], want[B][1], *_oracle_lists(B, NT, NA, "zipf"))
        groups = sum(_n_rg(B) for B, _, _ in outs[g])
        with torch.cuda.stream(streams[g]):
            assert sc.ctx.filter_skip_last() == [0] * _n_rg(outs[g][-1][0])
            cnt, proved = sc.ctx.filter_skip_read(), sc.ctx.live_proof_read()
        assert cnt == {"launches": n_calls, "planned": groups * N_FILTER, "live": 0}, cnt
        assert proved == groups, (proved, groups)
        sc.close()
    solo.close()


# ---- 9. where nothing is proved because no threshold launch builds lists from a table ----------------------------------------------
def test_inactive_with_a_score_mix():
    import torch
    B = 130
    _, _, _, srp, scol = _feed(B, NT, NA)
    h = _hidden(B, NT, NA, "zipf")
    sc = _Scorer(NT, NA, *_model(NT, NA, "zipf"))
    mixT = torch.zeros(((NT + 31) // 32 * 32, B), device="cuda"); w = torch.ones(B, device="cuda")
    sc.ctx.set_score_mix(mixT, w)
    s1, i1, live, cnt = sc.decode(h, srp, scol)
    proved = sc.proved
    s0, i0, _, _ = sc.decode(h, srp, scol, skip=False)
    sc.ctx.set_score_mix()
    sc.close()
    assert proved == 0 and live == [] and cnt["launches"] == 0 and _same_bits(s1, i1, s0, i0)


@pytest.mark.parametrize("Hh,B,dtype", [(128, 256, _lib.DAE_DTYPE_F32), (256, 64, _lib.DAE_DTYPE_F32), (256, 33, _lib.DAE_DTYPE_F32),
                                        (256, 256, _lib.DAE_DTYPE_BF16), (256, 256, _lib.DAE_DTYPE_BF16_EXACT)])
def test_inactive_paths(Hh, B, dtype):
    sc = _Scorer(NT, NA, *_model(NT, NA, "zipf", Hh), dtype=dtype)
    feed = _feed(B, NT, NA)
    s1, i1, live, cnt = sc.score(feed)
    proved = sc.proved
    s0, i0, _, _ = sc.score(feed, skip=False)
    assert sc.proved == 0
    sc.close()
    assert proved == 0 and live == [] and cnt["launches"] == 0 and _same_bits(s1, i1, s0, i0)
    if dtype != _lib.DAE_DTYPE_BF16:
        assert _same_bits(s1, i1, *_oracle_lists(B, NT, NA, "zipf", Hh))
