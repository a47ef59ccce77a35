"""GPU (-m gpu): the half-row-group sample stores only the wave-tiles it decodes, and the threshold launch reads only those
(decode_generic.hip decode_f32_kernel's HALF, tau_select.hip tau_select_kernel's SPARSE, the decoded-tile table of
csrc/score_plan.h; DESIGN.md sections 2 and 4).

A slot the sample skips keeps whatever an earlier call left there, so every test first POISONS the context: the weights x 40
model (nothing skipped) is prepacked into it and scored, which fills the sample and maxima buffers with large finite logits;
then the model under test is prepacked into the same context.  tests/test_sample_sparse_cpu.py shows on the CPU that the poison
bites: every row then has a stale value above its threshold among its skipped dense slots and among its unstored maxima.

Every comparison is bit for bit: the lists against the C oracle; the thresholds (last_tau, and score_topk_begin's), the live
lists, the filter counters and the sample counters against the same call under dae_set_filter_skip(0)
(tests/test_gpu_sample_skip.py _check_all / _check_decode: score_topk, begin + finish, decode_topk).

Shapes: those of tests/test_gpu_sample_skip.py -- 30 000 + 6 000 columns, k = 500, 469 sample tiles, the smallest shape that takes
the half-row-group sample with four waves' worth of tiles; 256 rows = four full half groups (128 workgroups each), 130 = a half
group of 2 rows and one of pad rows only, 65 = one row group (256 workgroups per half group: the 32-key threshold kernel, whose
rows are longer than the part it preloads) with a half group of one row."""
import numpy as np
import pytest

import oracle
import test_gpu_sample_skip as base
from test_gpu_sample_skip import K, N_SAMP, NT, _bits, _check_all, _check_decode, _dev, _feed, _hidden, _model, _oracle_lists, _planned, _same_bits
from test_sample_sparse_cpu import poison_bites

pytestmark = pytest.mark.gpu


class _Scorer(base._Scorer):
    """... whose context can take another model: load() prepacks it over the one it holds, nothing else is reset."""

    def load(self, W_enc, b_enc, W_dec, b_dec):
        self.We, self.be = _dev(W_enc), _dev(b_enc)
        self.Wd, self.bd = _dev(W_dec), _dev(b_dec)
        self.ctx.prepack_decoder(self.Wd, self.bd, 0, W_dec.shape[0], dtype=self.dtype)


def _poison(sc, bias, Hh, rows):
    """Score `rows` (a tuple of row counts) on the weights x 40 model, first with the skip off -- every wave-tile is decoded and
    every slot stored, whatever the model's bounds say -- then with it on, which leaves the decoded-tile table marking what
    that model decodes (everything, on the popularity bias at hidden 256): a sample launch that forgot to store a zero word
    would leave the threshold launch reading the poison."""
    sc.load(*_model(bias, Hh, 40.0))
    for B in rows:
        sc.score(_feed(B), skip=False)
        sc.poison_counters = sc.score(_feed(B))[4]


def _poisoned(bias, Hh, B):
    """A context that last scored 256 and B rows of the weights x 40 model and now holds the (bias, Hh) model."""
    sc = _Scorer(*_model(bias, Hh, 40.0))
    _poison(sc, bias, Hh, (256,) if B == 256 else (256, B))
    sc.load(*_model(bias, Hh))
    return sc


# ---- 1. stale slots -----------------------------------------------------------------------------------------------------------------
def test_stale_slots_are_never_read():
    """256 rows of the popularity model behind 256 rows of weights x 40 in ONE context: 84 of 1 876 wave-tiles are decoded, the
    slots of the other 1 792 hold the other model's logits -- in every row one of them lies above the row's threshold (the numpy
    model of tests/test_sample_sparse_cpu.py, which also predicts the 84)."""
    B = 256
    dense, maxima, decoded = poison_bites(B)
    assert dense.all() and maxima.all() and decoded == 84
    sc = _poisoned("zipf", 256, B)
    assert sc.poison_counters["decoded"] == sc.poison_counters["planned"] == 4 * N_SAMP      # (every slot marked and stored)
    cs = _check_all(sc, B, _feed(B), _hidden(B, "zipf"), _oracle_lists(B, "zipf"), "zipf bias behind weights x 40")
    sc.close()
    for c in cs:
        assert c["decoded"] == decoded and c["planned"] == 4 * N_SAMP, c


# ---- 2. row shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [256, 130, 65])
@pytest.mark.parametrize("Hh", [256, 252])
def test_row_shapes_behind_the_poison(B, Hh):
    """A half group of 2 rows and one of pad rows only (130), one row group with 256 workgroups per half group (65), pad units
    (hidden 252); seeds come from the feed."""
    assert np.diff(_feed(B)[3]).max() > 0
    sc = _poisoned("zipf", Hh, B)
    cs = _check_all(sc, B, _feed(B), _hidden(B, "zipf", Hh), _oracle_lists(B, "zipf", Hh), "zipf bias, hidden %d, behind weights x 40" % Hh)
    sc.close()
    for c in cs:
        assert 0 < c["decoded"] <= c["planned"] // 4, c


# ---- 3. partly live workgroups --------------------------------------------------------------------------------------------------------
def test_partly_live_workgroups_zero_bias():
    """b_dec = 0: 1 624 of 1 876 wave-tiles decoded -- most workgroups hold live and skipped waves side by side."""
    B = 256
    sc = _poisoned("zeros", 256, B)
    cs = _check_all(sc, B, _feed(B), _hidden(B, "zeros"), _oracle_lists(B, "zeros"), "b_dec = 0 behind weights x 40")
    sc.close()
    for c in cs:
        assert 0 < c["decoded"] < c["planned"], c


def test_partly_live_workgroups_hidden_rows_at_zero_and_one():
    """Hidden rows forced to {0, 1} on the popularity model (d = 0.5: 516 of 1 876 decoded), through dae_decode_topk."""
    B = 256
    _, _, W_dec, b_dec = _model("zipf")
    h = (np.random.default_rng(3).random((B, 256)) < 0.5).astype(np.float32)
    _, _, _, srp, scol = _feed(B)
    ref = oracle.topk(oracle.decode(h, W_dec, b_dec, 0, NT), K, srp, scol)
    sc = _poisoned("zipf", 256, B)
    c1, _ = _check_decode(sc, h, srp, scol, ref, "hidden rows in {0, 1}, zipf bias, behind weights x 40")
    sc.close()
    assert 0 < c1["decoded"] < c1["planned"], c1


# ---- 4. one context, nothing reset; two contexts on one image ---------------------------------------------------------------------------
def test_one_context_skip_on_off_on_through_row_counts():
    """256 -> 65 -> 256 rows on ONE poisoned context: at each, three skipping calls, two with the skip off (which store every
    slot again), and a skipping call behind them.  The table follows the geometry (128 / 256 words per half group)."""
    sc = _poisoned("zipf", 256, 65)
    seen = {}
    for B in (256, 65, 256):
        ref = _oracle_lists(B, "zipf")
        cs = _check_all(sc, B, _feed(B), _hidden(B, "zipf"), ref, "zipf bias, one context")
        s, i, _, _, c = sc.score(_feed(B))                             # (_check_all ends on the calls with the skip off)
        assert _same_bits(s, i, *ref) and np.array_equal(_bits(sc.tau_last), _bits(sc.tau(_feed(B), skip=False)[5]))
        assert c == cs[0] and 0 < c["decoded"] <= c["planned"] // 4, (c, cs[0])
        assert seen.setdefault(B, c) == c
    sc.close()


def test_two_contexts_share_one_image_on_two_streams():
    """Two contexts on one image (the popularity model), two streams, interleaved calls at rotating row counts: the table is per
    context, and a context's buffers hold what its own earlier calls at OTHER row counts left there."""
    import torch
    m = _model("zipf")
    solo = _Scorer(*m)
    shapes = (256, 130, 65)
    want, tau_off = {}, {}
    for B in shapes:
        _check_all(solo, B, _feed(B), None, _oracle_lists(B, "zipf"), "zipf bias, solo")
        want[B] = solo.score(_feed(B))
        solo.score(_feed(B), skip=False)
        tau_off[B] = solo.tau_last
    feeds = {B: [_dev(a) for a in _feed(B)] for B in shapes}
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    guests = []
    for st in streams:
        with torch.cuda.stream(st):
            guests.append(_Scorer(*m, share_from=solo))                # (a context binds the stream current at its creation)
    n_calls = 9
    outs = [[], []]
    for n in range(n_calls):
        for g, (st, sc) in enumerate(zip(streams, guests)):
            B = shapes[(n + g) % 3]
            d = feeds[B]
            with torch.cuda.stream(st):
                s, i = sc._out(B)
                sc.ctx.score_topk(d[0], d[1], d[2], sc.We, sc.be, NT, d[3], d[4], K, s, i)
            outs[g].append((B, s, i))
    torch.cuda.synchronize()
    for g, sc in enumerate(guests):
        for B, s, i in outs[g]:
            assert _same_bits(s.cpu().numpy(), i.cpu().numpy(), want[B][0], want[B][1]), (g, B)
        last_B = outs[g][-1][0]
        with torch.cuda.stream(streams[g]):
            assert np.array_equal(_bits(sc.ctx.last_tau(last_B)), _bits(tau_off[last_B]))
            assert sc.ctx.filter_skip_last() == want[last_B][2]
            f = sc.ctx.filter_skip_read()
            c = sc.ctx.sample_skip_read()
        assert f == {"launches": n_calls, "planned": sum((B + 127) // 128 * base.N_FILTER for B, _, _ in outs[g]),
                     "live": sum(sum(want[B][2]) for B, _, _ in outs[g])}, f
        assert c == {"launches": n_calls, "planned": sum(_planned(B) for B, _, _ in outs[g]),
                     "decoded": sum(want[B][4]["decoded"] for B, _, _ in outs[g])}, c
        sc.close()
    solo.close()


# ---- 5. nothing skipped -------------------------------------------------------------------------------------------------------------
def test_nothing_skipped_every_slot_marked():
    """weights x 40: decoded == planned -- the table marks every wave-tile, the threshold launch reads everything."""
    B = 256
    sc = _Scorer(*_model("zipf", 256, 40.0))
    cs = _check_all(sc, B, _feed(B), _hidden(B, "zipf", 256, 40.0), _oracle_lists(B, "zipf", 256, 40.0), "weights x 40")
    sc.close()
    for c in cs:
        assert c["decoded"] == c["planned"], c
