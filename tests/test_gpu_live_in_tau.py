"""GPU (-m gpu): the threshold launch builds the live tile lists of the fp32 hidden-256 filter launch itself (tau_select.hip
tau_select_kernel's tail: DESIGN.md section 2, "who builds the lists").

Two ways lead to the lists.  dae_score_topk / dae_decode_topk compute the thresholds and hand them to their own filter launch:
the last workgroup of every 128-row group of the threshold launch builds that group's list ("fused" below).  The halves --
dae_score_topk_begin, then dae_score_topk_finish with the thresholds begin returned -- run the standalone live_tiles_kernel
on the same thresholds.  Both must give the same counts per row group, and lists and scores that are bit for bit those of
the call with the skip off and of the C oracle.

Shapes: the models of tests/test_gpu_filter_skip.py (30 000 tracks + 6 000 artists at hidden 256: sample stride 2, 469 filter
tiles -- more than one pass of 256 threads and no multiple of it), the popularity model (nothing live) and b_dec = 0 (most
tiles live); 256 rows = two full groups, 130 = a second group of 2 rows (arrival target 2), 65 = one short group."""
import functools

import numpy as np
import pytest

import oracle
from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.models.DAEs import coo_to_csr, seeds_to_csr
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights

pytestmark = pytest.mark.gpu
K = 500
NT, NA = 30000, 6000
N_FILTER = 469


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _model(nt, na, bias, Hh=256):
    return make_weights(nt + na, Hh, seed=0, bias=bias, n_tracks=nt)


@functools.lru_cache(maxsize=None)
def _feed(B, nt, na):
    pos, ones, seeds = make_playlists(B, nt, na, seed=1)
    rp, col, val = coo_to_csr(pos, ones, B, nt + na)
    srp, sc = seeds_to_csr(seeds, B, nt)
    return rp, col, val, srp, sc


@functools.lru_cache(maxsize=None)
def _hidden(B, nt, na, bias, Hh=256):
    """The fp32 hidden rows of the feed, by the oracle (bit for bit the encode kernel's: tests/test_gpu_parity.py)."""
    W_enc, b_enc, _, _ = _model(nt, na, bias, Hh)
    rp, col, val, _, _ = _feed(B, nt, na)
    h = oracle.encode(rp, col, val, W_enc, b_enc)
    return h


@functools.lru_cache(maxsize=None)
def _oracle_lists(B, nt, na, bias, Hh=256, k=K):
    _, _, W_dec, b_dec = _model(nt, na, bias, Hh)
    _, _, _, srp, sc = _feed(B, nt, na)
    return oracle.topk(oracle.decode(_hidden(B, nt, na, bias, Hh), W_dec, b_dec, 0, nt), k, srp, sc)


def _same_bits(s, i, s_ref, i_ref):
    return np.array_equal(i, i_ref) and np.array_equal(np.ascontiguousarray(s).view(np.uint32), np.ascontiguousarray(s_ref).view(np.uint32))


class _Scorer:
    """One context with the model's image; every call returns (scores, ids, live per row group, counters)."""

    def __init__(self, nt, na, W_enc, b_enc, W_dec, b_dec, share_from=None, dtype=_lib.DAE_DTYPE_F32, k=K):
        self.nt, self.V, self.dtype, self.k = nt, nt + na, dtype, k
        self.ctx = _lib.Context(0)
        self.We, self.be = _dev(W_enc), _dev(b_enc)
        if share_from is None:
            self.Wd, self.bd = _dev(W_dec), _dev(b_dec)
            self.ctx.prepack_decoder(self.Wd, self.bd, 0, self.V, dtype=dtype)
        else:
            self.ctx.share_decoder(share_from.ctx, dtype)

    def _out(self, B):
        import torch
        return torch.empty((B, self.k), device="cuda"), torch.empty((B, self.k), dtype=torch.int32, device="cuda")

    def _result(self, s, i):
        last = self.ctx.filter_skip_last()
        return s.cpu().numpy(), i.cpu().numpy(), last, self.ctx.filter_skip_read()

    def score(self, feed, skip=True):
        d = [_dev(a) for a in feed]
        s, i = self._out(feed[0].size - 1)
        self.ctx.set_filter_skip(skip)
        self.ctx.score_topk(d[0], d[1], d[2], self.We, self.be, self.nt, d[3], d[4], self.k, s, i, dtype=self.dtype)
        return self._result(s, i)

    def decode(self, h, srp, sc, skip=True, n_tracks=None):
        s, i = self._out(h.shape[0])
        self.ctx.set_filter_skip(skip)
        self.ctx.decode_topk(_dev(h), self.nt if n_tracks is None else n_tracks, _dev(srp), _dev(sc), self.k, s, i, dtype=self.dtype)
        return self._result(s, i)

    def halves(self, feed, skip=True):
        """begin, then finish with the thresholds begin returned -> (..., the thresholds)."""
        import torch
        d = [_dev(a) for a in feed]
        B = feed[0].size - 1
        s, i = self._out(B)
        tau = torch.empty(B, device="cuda")
        self.ctx.set_filter_skip(skip)
        self.ctx.score_topk_begin(d[0], d[1], d[2], self.We, self.be, self.nt, d[3], self.k, tau, dtype=self.dtype)
        self.ctx.score_topk_finish(tau, d[3], d[4], s, i)
        return self._result(s, i) + (tau.cpu().numpy(),)

    def plan(self):
        return self.ctx.last_plan()

    def close(self):
        self.ctx.close()


def _counters(n_rg, n_f, live):
    return {"launches": 1, "planned": n_rg * n_f, "live": sum(live)}


# ---- 1. both ways to the lists, every row-group shape ----------------------------------------------------------------------------
@pytest.mark.parametrize("bias", ["zipf", "zeros"])
@pytest.mark.parametrize("B", [256, 130, 65])
@pytest.mark.parametrize("Hh", [256, 252])
def test_fused_lists_equal_the_standalone_kernels(B, bias, Hh):
    """252: Hp = 256, and the four zero units of the packed image must not enter d (they would read |0 - 0.5| = 0.5)."""
    W_enc, b_enc, W_dec, b_dec = _model(NT, NA, bias, Hh)
    feed = _feed(B, NT, NA)
    n_rg = (B + 127) // 128
    sc = _Scorer(NT, NA, W_enc, b_enc, W_dec, b_dec)
    s_h, i_h, live_h, cnt_h, _ = sc.halves(feed)
    s_f, i_f, live_f, cnt_f = sc.score(feed)
    plan = sc.plan()
    s_d, i_d, live_d, cnt_d = sc.decode(_hidden(B, NT, NA, bias, Hh), feed[3], feed[4])
    s_0, i_0, live_0, cnt_0 = sc.score(feed, skip=False)
    sc.close()
    assert plan["fused"] == 1 and plan["R_TILE"] == 128 and plan["n_rg"] == n_rg and plan["S"] == 2 and plan["n_filter_tiles"] == N_FILTER, plan
    print("B = %d, bias %s, hidden %d: live %s (halves) %s (score) %s (decode) of %d" % (B, bias, Hh, live_h, live_f, live_d, N_FILTER))
    assert len(live_h) == n_rg and live_f == live_h and live_d == live_h, (live_h, live_f, live_d)
    assert cnt_h == cnt_f == cnt_d == _counters(n_rg, N_FILTER, live_h), (cnt_h, cnt_f, cnt_d)
    assert live_0 == [] and cnt_0["launches"] == 0
    s_ref, i_ref = _oracle_lists(B, NT, NA, bias, Hh)
    for s, i in ((s_f, i_f), (s_d, i_d), (s_h, i_h), (s_0, i_0)):
        assert _same_bits(s, i, s_ref, i_ref)
    if bias == "zipf":
        assert live_h == [0] * n_rg
    elif Hh == 256:
        assert all(0 < n < N_FILTER for n in live_h), live_h


@pytest.mark.parametrize("bias", ["zipf", "zeros"])
@pytest.mark.parametrize("B", [256, 130, 65])
def test_hidden_rows_at_zero_and_one(B, bias):
    """Every entry 0 or 1: d = 0.5 exactly, through dae_decode_topk (the halves take no hidden rows: the call with the skip off
    and the oracle are the references for the lists; of the counts only their consistency is checked)."""
    W_enc, b_enc, W_dec, b_dec = _model(NT, NA, bias)
    h = (np.random.default_rng(3).random((256, 256)) < 0.5).astype(np.float32)[:B]
    _, _, _, srp, scol = _feed(B, NT, NA)
    n_rg = (B + 127) // 128
    sc = _Scorer(NT, NA, W_enc, b_enc, W_dec, b_dec)
    s1, i1, live, cnt = sc.decode(h, srp, scol)
    s0, i0, _, _ = sc.decode(h, srp, scol, skip=False)
    sc.close()
    s_ref, i_ref = oracle.topk(oracle.decode(h, W_dec, b_dec, 0, NT), K, srp, scol)
    assert _same_bits(s1, i1, s_ref, i_ref) and _same_bits(s1, i1, s0, i0)
    assert len(live) == n_rg and all(0 <= n <= N_FILTER for n in live) and cnt == _counters(n_rg, N_FILTER, live), (live, cnt)
    print("hidden rows in {0, 1}, B = %d, bias %s: live %s of %d" % (B, bias, live, N_FILTER))


# ---- 2. exactly one live tile for one row -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_star", [NT - 10,         # in the tile that also holds the first artists: bounded over its ranked columns
                                    29970])          # in the last full tile of tracks: the ordinary per-tile pair
def test_one_live_tile_for_one_row(c_star):
    """Rows at 0.5 except the last, which sits at 1 on the positive weights of column c*: group 0 keeps nothing, group 1 (2 rows)
    at least the tile of c*.  The halves take a feed, not hidden rows, so the ENCODER is built to give these rows: W_enc = 0
    and b_enc = 0 (every unit sigmoid(0) = 0.5), but 1e4 on those units in the row of a column only the last playlist holds
    (the encoder divides a row by its sum, 127 here: sigmoid(39) = 1 in fp32)."""
    B = 130
    _, b_enc, W_dec, b_dec = _model(NT, NA, "zipf")
    W_dec = W_dec.copy()
    w = W_dec[c_star].astype(np.float64)
    s_all, s_pos = w.sum(), w[w > 0].sum()
    alpha = 2.0 * (3.0 - float(b_dec[c_star])) / (s_all + s_pos)
    W_dec[c_star] = (W_dec[c_star] * np.float32(alpha)).astype(np.float32)
    assert float(b_dec[c_star]) + 0.5 * alpha * s_all < -6.0           # far below every row's threshold (about -4.5)
    h_want = np.full((B, 256), 0.5, np.float32)
    h_want[B - 1, W_dec[c_star] > 0] = 1.0
    feed = _feed(B, NT, NA)
    rp, col, val, srp, scol = feed
    c_feed = max(set(col[rp[B - 1]:rp[B]].tolist()) - set(col[:rp[B - 1]].tolist()))
    W_enc = np.zeros((NT + NA, 256), np.float32)
    W_enc[c_feed, W_dec[c_star] > 0] = 1.0e4
    assert not b_enc.any()
    h = oracle.encode(rp, col, val, W_enc, b_enc)
    assert np.array_equal(h, h_want)
    sc = _Scorer(NT, NA, W_enc, b_enc, W_dec, b_dec)
    s_h, i_h, live_h, cnt_h, _ = sc.halves(feed)
    s_f, i_f, live_f, cnt_f = sc.score(feed)
    s_d, i_d, live_d, cnt_d = sc.decode(h, srp, scol)
    s_0, i_0, _, _ = sc.decode(h, srp, scol, skip=False)
    sc.close()
    s_ref, i_ref = oracle.topk(oracle.decode(h, W_dec, b_dec, 0, NT), K, srp, scol)
    for s, i in ((s_f, i_f), (s_d, i_d), (s_h, i_h), (s_0, i_0)):
        assert _same_bits(s, i, s_ref, i_ref)
    assert c_star in i_f[B - 1] and not (i_f[:B - 1] == c_star).any()
    assert live_h[0] == 0 and 1 <= live_h[1] < N_FILTER, live_h
    assert live_f == live_h and live_d == live_h and cnt_f == cnt_d == cnt_h == _counters(2, N_FILTER, live_h), (live_h, live_f, live_d)


# ---- 3. the arrival counters are left at zero ----------------------------------------------------------------------------------
def test_one_context_through_changing_row_counts():
    """256 -> 130 -> 65 -> 256 on ONE context with nothing reset between: a reducer that left its counter standing would make
    the next call's group fire early (or never) and the counts differ from the standalone kernel's."""
    import torch
    sc = _Scorer(NT, NA, *_model(NT, NA, "zeros"))
    torch.cuda.synchronize()                                           # the owner's prepack before the borrower's first launch
    ref = _Scorer(NT, NA, *_model(NT, NA, "zeros"), share_from=sc)
    want = {B: ref.halves(_feed(B, NT, NA)) for B in (256, 130, 65)}
    ref.close()
    for B in (256, 130, 65, 256):
        s, i, live, cnt = sc.score(_feed(B, NT, NA))
        s_h, i_h, live_h, cnt_h, _ = want[B]
        assert live == live_h and cnt == cnt_h == _counters((B + 127) // 128, N_FILTER, live), (B, live, live_h, cnt)
        assert _same_bits(s, i, s_h, i_h) and _same_bits(s, i, *_oracle_lists(B, NT, NA, "zeros"))
    sc.close()


# ---- 3b. WHICH builder ran ------------------------------------------------------------------------------------------------------
def test_the_threshold_launch_is_the_builder_of_the_fused_call():
    """Counts and lists are the same on both ways by design, so they cannot tell which kernel built them.  The context's scratch
    can: only a threshold launch that builds the lists reserves its arrival counters and per-row d (score.hip topk_phase_a: 64
    counters + Bpad doubles, in 256-byte units), and it does so once.  The halves and the call with the skip off never do."""
    B = 256
    want = (64 * 4 + 256 * 8 + 255) // 256 * 256
    sc = _Scorer(NT, NA, *_model(NT, NA, "zeros"))
    feed = _feed(B, NT, NA)
    size = lambda: int(sc.ctx.lib.dae_scratch_bytes(sc.ctx.h))
    sc.halves(feed)                                                    # the standalone kernel: lists, counters, no such words
    sc.score(feed, skip=False)                                         # everything a one-call scoring needs but the lists
    s0 = size()
    sc.halves(feed)
    sc.score(feed, skip=False)
    assert size() == s0
    _, _, live, cnt = sc.score(feed)                                   # the threshold launch builds the lists
    s1 = size()
    sc.score(feed)
    sc.halves(feed)
    s2 = size()
    sc.close()
    assert sum(live) > 0 and cnt["launches"] == 1
    assert s1 - s0 == want and s2 == s1, (s0, s1, s2, want)


# ---- 4. two contexts, one image, two streams ------------------------------------------------------------------------------------
def test_two_contexts_on_two_streams_interleaved():
    import torch
    m = _model(NT, NA, "zeros")
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
        total = 0
        for B, s, i in outs[g]:
            assert _same_bits(s.cpu().numpy(), i.cpu().numpy(), want[B][0], want[B][1]), (g, B)
            total += sum(want[B][2])
        last_B = outs[g][-1][0]
        with torch.cuda.stream(streams[g]):
            assert sc.ctx.filter_skip_last() == want[last_B][2]
            cnt = sc.ctx.filter_skip_read()
        assert cnt == {"launches": n_calls, "planned": sum((B + 127) // 128 * N_FILTER for B, _, _ in outs[g]), "live": total}, cnt
        sc.close()
    solo.close()


# ---- 5. a row whose threshold is -inf ----------------------------------------------------------------------------------------
def test_threshold_minus_infinity_k1024_small_model():
    """k = 1024 on the 12 000 + 6 000 model.  Whether a row's threshold is -inf there depends on the number of group maxima the
    sample leaves per row (4 096 at 130 rows against k + seeds <= 1 124): the test reads the thresholds from begin and, for
    every group that holds such a row, wants every tile kept.  Both ways to the lists must agree in any case."""
    nt, na, B, k = 12000, 6000, 130, 1024
    W_enc, b_enc, W_dec, b_dec = _model(nt, na, "zeros")
    feed = _feed(B, nt, na)
    sc = _Scorer(nt, na, W_enc, b_enc, W_dec, b_dec, k=k)
    s_h, i_h, live_h, cnt_h, tau = sc.halves(feed)
    s_f, i_f, live_f, cnt_f = sc.score(feed)
    n_f = sc.plan()["n_filter_tiles"]
    sc.close()
    neg = [bool(np.isneginf(tau[g * 128:(g + 1) * 128]).any()) for g in range(2)]
    print("k = 1024 on 12 000 + 6 000: rows at -inf per group %s, live %s of %d" % (neg, live_h, n_f))
    assert live_f == live_h and cnt_f == cnt_h == _counters(2, n_f, live_h)
    assert all(live_h[g] == n_f for g in range(2) if neg[g])
    assert _same_bits(s_f, i_f, s_h, i_h) and _same_bits(s_f, i_f, *_oracle_lists(B, nt, na, "zeros", 256, k))


def test_threshold_minus_infinity_every_row():
    """A construction that does reach -inf: 2 000 ranked tracks of the same image are 63 tiles, 32 of them the sample, one per
    workgroup -- 1 024 group maxima per row, one short of k + 1 = 1 025.  Every row's threshold is -inf and both groups keep
    all 31 filter tiles."""
    nt, na, B, k, n_rank = 12000, 6000, 130, 1024, 2000
    W_enc, b_enc, W_dec, b_dec = _model(nt, na, "zeros")
    h = _hidden(B, nt, na, "zeros")
    _, _, seeds = make_playlists(B, n_rank, 0, seed=2)
    srp, scol = seeds_to_csr(seeds, B, n_rank)
    sc = _Scorer(nt, na, W_enc, b_enc, W_dec, b_dec, k=k)
    s1, i1, live, cnt = sc.decode(h, srp, scol, n_tracks=n_rank)
    plan = sc.plan()
    s0, i0, _, _ = sc.decode(h, srp, scol, skip=False, n_tracks=n_rank)
    sc.close()
    assert plan["fused"] == 1 and plan["n_sample_tiles"] == 32 and plan["n_filter_tiles"] == 31 and plan["n_rg"] == 2, plan
    assert live == [31, 31] and cnt == _counters(2, 31, live), (live, cnt)
    s_ref, i_ref = oracle.topk(oracle.decode(h, W_dec, b_dec, 0, n_rank), k, srp, scol)
    assert _same_bits(s1, i1, s_ref, i_ref) and _same_bits(s1, i1, s0, i0)


# ---- 6. where the threshold launch builds nothing --------------------------------------------------------------------------------
def _no_skip(live, cnt):
    return live == [] and cnt == {"launches": 0, "planned": 0, "live": 0}


def test_halves_run_the_standalone_kernel_and_skip_off_builds_nothing():
    """(the halves' results equal the fused call's in test 1; here: the skip off gives no lists on either way)"""
    sc = _Scorer(NT, NA, *_model(NT, NA, "zeros"))
    feed = _feed(130, NT, NA)
    s1, i1, live1, cnt1, _ = sc.halves(feed, skip=False)
    s0, i0, live0, cnt0 = sc.score(feed, skip=False)
    sc.close()
    assert _no_skip(live1, cnt1) and _no_skip(live0, cnt0)
    assert _same_bits(s1, i1, s0, i0) and _same_bits(s1, i1, *_oracle_lists(130, NT, NA, "zeros"))


def test_inactive_with_a_score_mix():
    import torch
    B = 130
    W_enc, b_enc, W_dec, b_dec = _model(NT, NA, "zipf")
    _, _, _, srp, scol = _feed(B, NT, NA)
    h = _hidden(B, NT, NA, "zipf")
    sc = _Scorer(NT, NA, W_enc, b_enc, W_dec, b_dec)
    mixT = torch.zeros(((NT + 31) // 32 * 32, B), device="cuda"); w = torch.ones(B, device="cuda")
    sc.ctx.set_score_mix(mixT, w)
    s1, i1, live, cnt = sc.decode(h, srp, scol)
    plan = sc.plan()
    s0, i0, _, _ = sc.decode(h, srp, scol, skip=False)
    sc.ctx.set_score_mix()
    sc.close()
    assert plan["fused"] == 1 and _no_skip(live, cnt) and _same_bits(s1, i1, s0, i0)


@pytest.mark.parametrize("Hh,B,dtype", [(128, 256, _lib.DAE_DTYPE_F32), (256, 64, _lib.DAE_DTYPE_F32), (256, 256, _lib.DAE_DTYPE_BF16), (256, 256, _lib.DAE_DTYPE_BF16_EXACT)])
def test_inactive_paths(Hh, B, dtype):
    W_enc, b_enc, W_dec, b_dec = _model(NT, NA, "zipf", Hh)
    feed = _feed(B, NT, NA)
    sc = _Scorer(NT, NA, W_enc, b_enc, W_dec, b_dec, dtype=dtype)
    s1, i1, live, cnt = sc.score(feed)
    plan = sc.plan()
    s0, i0, _, _ = sc.score(feed, skip=False)
    sc.close()
    assert plan["fused"] == 1 and plan["n_filter_tiles"] > 0, plan
    assert _no_skip(live, cnt) and _same_bits(s1, i1, s0, i0)
    if dtype != _lib.DAE_DTYPE_BF16:                                  # fp32 and the exact mode return the oracle's lists
        assert _same_bits(s1, i1, *_oracle_lists(B, NT, NA, "zipf", Hh))
