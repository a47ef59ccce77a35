"""Several DAEs over one vocabulary answering together: `DAE_ensemble` ranks by a weighted sum of its
members' scores,

    t_m[r, c] = sigmoid(z_m[r, c]) * a_m[r]
    acc = t_0;  acc = acc + t_m  for m = 1 .. M-2                 (untitled: the last member is not in acc)
    untitled:  y = t_{M-1} + acc                                  (M = 1: y = t_0)
    titled:    acc also takes t_{M-1};  y = sigmoid(z_title) * w_title[r] + acc

every operation one fp32 rounding in this order (include/dae_hip.h: the canonical value).  `recommend` never builds a
[n_rows, n_input] matrix: the members' terms meet in one transposed buffer (dae_decode_mix_term, dae_decode_mix_term_add) and
the last scorer's threshold path ranks its own weighted sigmoid plus that buffer (dae_ensemble_topk).  `ensemble_scores` is
the readable definition: the dense y from per-member dense decodes and elementwise torch operations in the same order.
`rank_of` gives the exact rank of given tracks under y over the whole vocabulary (dae_ensemble_rank_of), and `fit_alphas`
chooses the alphas by those ranks (utils/ensemble_fit.py).

The reference trains a tied `--pretrain` and an untied `--dae` model per challenge category and can use one at a time; their
pickles are interchangeable "if both have same number of tracks & artists" -- which is all an ensemble asks of its members.
"""
import copy
import pickle
import sys

import numpy as np

from .. import _lib
from .stream_loop import SEEDS_FROM_INPUT      # noqa: F401  (recommend(seeds=SEEDS_FROM_INPUT))


class DAE_ensemble:
    """members: fitted `DAE` / `DAE_tied` objects over the same vocabulary (equal n_input and n_tracks; hidden sizes may
    differ), in the order of the sum.  alphas: M floats, or an [M, n_rows] array of per-row weights (rows behind it weigh 0);
    default float32(1 / M) each.  title_model: a fitted title scorer (models/title_models.py) -- with titles in use the mix of
    `DAE_title` joins the sum: a_m[r] = alpha_m[r] * w_playlist[r] (one fp32 product), w_title / w_playlist from
    dae_mix_weights over member 0's feed.  Without titles in use a_m[r] = alpha_m[r].

    The ensemble owns nothing of its members: it binds their contexts to the caller's stream for a call, as the members' own
    calls do, and leaves no state behind in them.  The batch of a call is member 0's `n_batch`."""

    K_MAX = _lib.DAE_MAX_K

    def __init__(self, members, alphas=None, title_model=None):
        members = list(members)
        if not members:
            raise ValueError("DAE_ensemble: at least one member is required")
        for i, m in enumerate(members):
            for attr in ("n_input", "n_tracks", "n_hidden", "n_batch", "weights", "biases"):
                if not hasattr(m, attr):
                    raise ValueError("DAE_ensemble: member %d is no DAE / DAE_tied model (it has no `%s`)" % (i, attr))
            if getattr(m, "ctx", None) is None:
                raise ValueError("DAE_ensemble: member %d is not fitted (call fit() first)" % i)
            if any(m is o for o in members[:i]):
                raise ValueError("DAE_ensemble: member %d is listed twice (every member ranks with a context of its own)" % i)
        m0 = members[0]
        for i, m in enumerate(members[1:], 1):
            if int(m.n_input) != int(m0.n_input):
                raise ValueError("DAE_ensemble: member %d has n_input = %d, member 0 has %d" % (i, m.n_input, m0.n_input))
            if int(m.n_tracks) != int(m0.n_tracks):
                raise ValueError("DAE_ensemble: member %d has n_tracks = %d, member 0 has %d" % (i, m.n_tracks, m0.n_tracks))
            if int(getattr(m, "device_index", 0)) != int(getattr(m0, "device_index", 0)):
                raise ValueError("DAE_ensemble: member %d lives on device %d, member 0 on %d"
                                 % (i, m.device_index, m0.device_index))
        if title_model is not None:
            if getattr(title_model, "ctx", None) is None:
                raise ValueError("DAE_ensemble: the title model is not fitted (call fit() first)")
            if int(title_model.output_dim) != int(m0.n_input):
                raise ValueError("DAE_ensemble: the title model scores %d columns, the members have n_input = %d"
                                 % (title_model.output_dim, m0.n_input))
        self.members, self.title_model = members, title_model
        self.n_input, self.n_tracks, self.n_batch = int(m0.n_input), int(m0.n_tracks), int(m0.n_batch)
        self.alphas = self._check_alphas(alphas, len(members))
        self._exact_said = False

    # -- arguments ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_alphas(alphas, M):
        """-> float32 [M] (one weight per member) or float32 [M, n] (per row)."""
        if alphas is None:
            return np.full(M, np.float32(1.0) / np.float32(M), np.float32)
        a = np.asarray(alphas, np.float32)
        if a.ndim not in (1, 2) or a.shape[0] != M:
            raise ValueError("DAE_ensemble: alphas must be %d floats or an array [%d, n_rows], got shape %s"
                             % (M, M, tuple(a.shape)))
        return np.ascontiguousarray(a)

    def _refuse(self, k=None, catalogue=None):
        if k is not None and not 1 <= int(k) <= self.K_MAX:
            raise ValueError("DAE_ensemble ranks 1 <= k <= %d tracks per row (got %d): the mixed threshold path keeps that limit"
                             % (self.K_MAX, k))
        if catalogue is not None:
            raise ValueError("DAE_ensemble does not rank inside a catalogue: its members rank all n_tracks = %d tracks"
                             % self.n_tracks)
        for i, m in enumerate(self.members):
            if getattr(m, "_score_shard", None) is not None:
                raise ValueError("DAE_ensemble is not vocabulary-sharded: member %d has a scoring shard (shard_scoring); every "
                                 "member must hold its whole decoder" % i)

    def _dtype(self, dtype):
        dtype = self.members[0]._dtype_of(dtype)
        if dtype == _lib.DAE_DTYPE_BF16_EXACT:
            if not self._exact_said:
                self._exact_said = True
                print("[dae] decode_dtype = exact_bf16: an ensemble has no exact bf16 path; its calls run on the fp32 kernels "
                      "(same lists, slower)", file=sys.stderr)
            return _lib.DAE_DTYPE_F32
        return dtype

    def _titles_in_use(self, titles, titles_use):
        return (self.title_model is not None and titles is not None and titles_use is not None
                and bool(np.any(np.asarray(titles_use))))

    # -- the shared front of every call: CSR, hidden rows, weights -------------------------------------------------------------
    def _alpha_rows(self, nb):
        """The alphas as M float32 vectors of nb rows on member 0's device."""
        import torch
        a = self.alphas
        rows = np.zeros((len(self.members), nb), np.float32)
        if a.ndim == 1:
            rows[:] = a[:, None]
        else:
            n = min(nb, a.shape[1])
            rows[:, :n] = a[:, :n]
        d = self.members[0]._to_dev(rows, torch.float32)
        return [d[m] for m in range(len(self.members))]

    def _begin(self, x_positions, x_ones, nb, dtype, titles, titles_use, pack=True):
        """Everything in front of the ranking, enqueued on the current stream: member 0's CSR of the feed, every member's
        hidden rows (dae_encode), the weights a_m and -- with titles in use -- the title features and w_title.
        -> (csr, hs, a, feat, w_t)."""
        import torch
        m0, tm = self.members[0], self.title_model
        titled = self._titles_in_use(titles, titles_use)
        for m in self.members:
            if pack:
                m._ensure_packed(dtype)
            else:
                m.sync_params()
            m.ctx.bind_stream()
        if titled:
            if pack:
                tm._ensure_packed(dtype)
            tm.ctx.bind_stream()
        csr = m0._upload_csr(x_positions, x_ones, n_rows=nb)
        dev = csr[0].device
        hs = []
        for m in self.members:
            h = torch.empty((nb, m.n_hidden), dtype=torch.float32, device=dev)
            m.ctx.encode(csr[0], csr[1], csr[2], m.weights["encoder_h"], m.biases["encoder_b"], h)
            hs.append(h)
        a = self._alpha_rows(nb)
        feat = w_t = None
        if titled:
            w_t, w_p = self._mix_weights(csr, titles_use, nb)
            a = [al * w_p for al in a]                            # a_m = alpha_m * w_playlist: one fp32 product
            feat = tm.features(titles, nb)
        return csr, hs, a, feat, w_t

    def _mix_weights(self, csr, titles_use, nb):
        """w_title / w_playlist of the rows as `DAE_title` computes them (dae_mix_weights over member 0's feed)."""
        import torch
        m0 = self.members[0]
        P = _lib._ptr
        u = np.zeros(nb, np.float32)
        tu = np.asarray(titles_use, np.float32).reshape(-1)
        u[:len(tu)] = tu[:nb]
        u = m0._to_dev(u, torch.float32)
        w_t = torch.empty(nb, dtype=torch.float32, device=csr[0].device)
        w_p = torch.empty(nb, dtype=torch.float32, device=csr[0].device)
        m0.ctx.check(m0.ctx.lib.dae_mix_weights(m0.ctx.h, P(csr[0]), P(csr[1]), P(csr[2]), nb, 1.0, 0, P(u), P(w_t), P(w_p)))
        return w_t, w_p

    # -- ranking ------------------------------------------------------------------------------------------------------------
    def recommend(self, x_positions, x_ones, seeds, k=500, n_rows=None, dtype=None, titles=None, titles_use=None,
                  catalogue=None):
        """The k best tracks per row by the ensemble's y (canonical order: y descending, then column ascending; seeds removed)
        -> (idx [n_rows, k] int32 with -1 padding, score [n_rows, k] float32 holding y, -inf beside a -1), like
        `DAE.recommend`.  seeds: per-row id lists or SEEDS_FROM_INPUT.  dtype: "f32" | "bf16" (member 0's decode_dtype by
        default); "exact_bf16" runs the fp32 kernels and says so once on stderr.  k > 1024, a catalogue, or a member with a
        scoring shard raise ValueError naming the limit, before anything is launched."""
        import torch
        self._refuse(k=k, catalogue=catalogue)
        dtype = self._dtype(dtype)
        nb = self.n_batch
        n_rows = nb if n_rows is None else n_rows
        m0 = self.members[0]
        csr, hs, a, feat, w_t = self._begin(x_positions, x_ones, nb, dtype, titles, titles_use)
        d_srp, d_sc = m0._seed_csr_dev(seeds, csr, n_rows=nb)
        score = torch.empty((nb, k), dtype=torch.float32, device=csr[0].device)
        idx = torch.empty((nb, k), dtype=torch.int32, device=csr[0].device)
        ctxs = [m.ctx for m in self.members]
        ranker = self.title_model.ctx if feat is not None else ctxs[-1]
        ranker.ensemble_topk(ctxs, hs, a, self.n_tracks, d_srp, d_sc, k, score, idx, dtype=dtype, feat=feat, w_title=w_t)
        res = idx[:n_rows].cpu().numpy(), score[:n_rows].cpu().numpy()
        m0._check_feed()
        return res

    def recommend_iter(self, feeds, k=500, want_scores=True, dtype=None):
        """A plain loop over `recommend` with the models' feed tuples (x_positions, x_ones, seeds, n_rows[, titles[,
        titles_use]]) -> (idx, score or None) per feed, in order.  NOT pipelined: every feed is uploaded, ranked and fetched
        before the next one is looked at.  It exists so that the drivers' `recommend_iter` branches take an ensemble as they
        take a model."""
        self._refuse(k=k)
        for f in feeds:
            kw = {"titles": f[4], "titles_use": f[5] if len(f) > 5 else None} if len(f) > 4 else {}
            idx, score = self.recommend(f[0], f[1], f[2], k=k, n_rows=f[3], dtype=dtype, **kw)
            yield idx, (score if want_scores else None)

    # -- the readable definition --------------------------------------------------------------------------------------------------
    def ensemble_scores(self, x_positions, x_ones, n_rows=None, dtype=None, titles=None, titles_use=None):
        """The dense y over the track columns, float32 [n_rows, n_tracks] (host array): per member one dense decode with the
        sigmoid (dae_decode_dense in `dtype`), then the canonical chain as separate elementwise fp32 operations.  What
        `recommend` ranks, element for element; it materialises one [n_batch, n_input] matrix at a time."""
        import torch
        self._refuse()
        dtype = self._dtype(dtype)
        nb, nt = self.n_batch, self.n_tracks
        n_rows = nb if n_rows is None else n_rows
        csr, hs, a, feat, w_t = self._begin(x_positions, x_ones, nb, dtype, titles, titles_use)
        dense = torch.empty((nb, self.n_input), dtype=torch.float32, device=csr[0].device)

        def term(ctx, h, w):
            ctx.decode_dense(h, dense, apply_sigmoid=True, dtype=dtype)
            return dense[:, :nt] * w[:, None]                     # t = sigmoid(z) * a: a fresh tensor, `dense` is reused
        M = len(self.members)
        n_acc = M if feat is not None else M - 1
        acc = None
        for m in range(n_acc):
            t = term(self.members[m].ctx, hs[m], a[m])
            acc = t if acc is None else acc + t
        last = term(self.title_model.ctx, feat, w_t) if feat is not None else term(self.members[-1].ctx, hs[-1], a[-1])
        y = last if acc is None else last + acc
        res = y[:n_rows].cpu().numpy()
        self.members[0]._check_feed()
        return res

    # -- caller-given candidate columns ------------------------------------------------------------------------------------------
    def score_candidates(self, x_positions, x_ones, candidates, n_rows=None, titles=None, titles_use=None):
        """y of THESE columns for each playlist, in the forms `DAE.score_candidates` takes and returns: per member the
        canonical fp32 sigmoid of the listed pairs (dae_encode + dae_decode_candidates, the two halves of
        dae_score_candidates), weighted and summed on the device in the canonical
        order with separate fp32 multiplies and adds; with titles in use the title scorer's own term from the title chain of
        dae_mix_candidates.  Always fp32, so `score_candidates(feed, recommend(feed)[0])` equals an fp32 `recommend(feed)[1]`
        bit for bit."""
        import torch
        self._refuse()
        m0, tm = self.members[0], self.title_model
        n_rows, rp, col, cand, status = m0._cand_begin(candidates, n_rows, unique=False)
        nb, n_cand = self.n_batch, int(col.size)
        csr, hs, a, feat, w_t = self._begin(x_positions, x_ones, nb, _lib.DAE_DTYPE_F32, titles, titles_use, pack=False)
        dev = csr[0].device
        rp_b = np.full(nb + 1, rp[-1], np.int64)
        rp_b[:len(rp)] = rp
        rows = m0._to_dev(np.repeat(np.arange(nb), np.diff(rp_b)) if n_cand else np.zeros(0, np.int64), torch.int64)

        def term(m):
            out = torch.empty(max(n_cand, 1), dtype=torch.float32, device=dev)
            mem = self.members[m]
            mem.ctx.decode_candidates(hs[m], mem.weights["decoder_h"], mem.biases["decoder_b"], cand, n_cand, out,
                                      out_kind=_lib.DAE_OUT_SCORE, status=status)
            return out[:n_cand] * a[m][rows]
        M = len(self.members)
        n_acc = M if feat is not None else M - 1
        acc = None
        for m in range(n_acc):
            t = term(m)
            acc = t if acc is None else acc + t
        if feat is not None:
            # the title scorer's term alone: dae_mix_candidates computes sigmoid(z_title) * w_title + sigmoid(z_dae) * w_playlist,
            # and with w_playlist = -0.0f the second product is a zero whose sum leaves the first as it is
            out = torch.empty(max(n_cand, 1), dtype=torch.float32, device=dev)
            neg0 = torch.full((nb,), -0.0, dtype=torch.float32, device=dev)
            mem = self.members[0]
            tm.ctx.mix_candidates(mem.ctx, hs[0], mem.weights["decoder_h"], mem.biases["decoder_b"], feat, tm.p["Output_WT"],
                                  tm.p["Output_b"], w_t, neg0, cand, n_cand, out, status=status)
            last = out[:n_cand]
        else:
            last = term(M - 1)
        y = last if acc is None else last + acc
        m0._cand_status(status)
        values = y.cpu().numpy()
        m0._check_feed()
        return m0._cand_result(values, candidates, rp)

    # -- exact ranks of given tracks under y (dae_ensemble_rank_of) --------------------------------------------------------------------
    def rank_of(self, x_positions, x_ones, columns, seeds, n_rows=None, titles=None, titles_use=None, want_scores=False,
                catalogue=None):
        """Where THESE tracks stand for each playlist under the ensemble's y: per listed (row, column) the number of non-seed
        track columns that precede it (y descending, ties by column ascending), 0-based, so
        `rank_of(feed, recommend(feed, seeds)[0], seeds)` is `arange(k)` per row -- below position 1 024 too, where the lists
        end.  columns, seeds (SEEDS_FROM_INPUT included), n_rows, the return forms and the -1 results (padding, an artist, a
        seed) are `DAE_title.mixed_rank_of`'s; want_scores -> (ranks, y), -inf beside a rank of -1: `recommend`'s fp32 score
        column bit for bit.  The dispatch on titles in use is `recommend`'s.  Always fp32 (every scorer's fp32 image is packed
        for the call); no k applies.  A member with a scoring shard and catalogue= raise ValueError before anything is launched."""
        import torch
        if catalogue is not None:
            raise ValueError("DAE_ensemble.rank_of: ranks inside a catalogue are not built; the ranks are over all n_tracks = %d "
                             "track columns (call it without catalogue=)" % self.n_tracks)
        self._refuse()
        m0, tm = self.members[0], self.title_model
        n_rows, rp, col, ans, status = m0._cand_begin(columns, n_rows, unique=False)
        nb, n = self.n_batch, int(col.size)
        csr, hs, a, feat, w_t = self._begin(x_positions, x_ones, nb, _lib.DAE_DTYPE_F32, titles, titles_use)
        dev = csr[0].device
        d_srp, d_sc = m0._seed_csr_dev(seeds, csr, n_rows=nb)
        rank = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        score = torch.empty(max(n, 1), dtype=torch.float32, device=dev) if want_scores else None
        ctxs = [m.ctx for m in self.members]
        title_kw = {} if feat is None else {"feat": feat, "OutW_T": tm.p["Output_WT"], "Out_b": tm.p["Output_b"], "w_title": w_t}
        ranker = tm.ctx if feat is not None else ctxs[-1]
        ranker.ensemble_rank_of(ctxs, hs, a, [m.weights["decoder_h"] for m in self.members],
                                [m.biases["decoder_b"] for m in self.members], self.n_tracks, d_srp, d_sc, ans, n, rank,
                                out_score=score, status=status, **title_kw)
        m0._cand_status(status)
        ranks = rank.cpu().numpy()[:n]
        scores = score.cpu().numpy()[:n] if want_scores else None
        m0._check_feed()
        if want_scores:
            return m0._rank_result(ranks, columns, rp, n_rows, -1), m0._rank_result(scores, columns, rp, n_rows, -np.inf)
        return m0._rank_result(ranks, columns, rp, n_rows, -1)

    def _ranks_of_feeds(self, feeds):
        """`rank_of` feed by feed over (x_positions, x_ones, answers, seeds, n_rows[, titles, titles_use]) -> every listed
        answer's rank, concatenated in order (int32; -1 for what cannot be ranked)."""
        out = []
        for f in feeds:
            kw = {"titles": f[5], "titles_use": f[6] if len(f) > 6 else None} if len(f) > 5 else {}
            out.extend(np.asarray(r, np.int32).reshape(-1) for r in self.rank_of(f[0], f[1], f[2], f[3], n_rows=f[4], **kw))
        return np.concatenate(out) if out else np.zeros(0, np.int32)

    def fit_alphas(self, feeds, metric="mrr", steps=10, rounds=4):
        """Choose the alphas by the exact ranks of held-out tracks: the grid search of utils/ensemble_fit.py `search_simplex` over
        alphas = i / steps, each point evaluated as `metric` ("mrr" or "recall@N"; utils/metrics.py, a -1 rank a miss that counts
        in the denominator) of the concatenated `rank_of` ranks of all feeds.  feeds: a re-iterable sequence of
        (x_positions, x_ones, answers, seeds, n_rows[, titles, titles_use]).  Sets self.alphas to the best point and returns
        (alphas, value, trace).  Between evaluations only the alphas change.  An ensemble with per-row alphas ([M, n_rows])
        raises ValueError: the search is over one weight per member."""
        from ..utils.ensemble_fit import parse_metric, search_simplex
        if self.alphas.ndim != 1:
            raise ValueError("DAE_ensemble.fit_alphas: per-row alphas (an array [M, n_rows]) cannot be fitted; the search is over one "
                             "weight per member")
        score = parse_metric(metric)
        kept = self.alphas

        def evaluate(alphas):
            self.alphas = self._check_alphas(alphas, len(self.members))
            return score(self._ranks_of_feeds(feeds))
        try:
            alphas, value, trace = search_simplex(evaluate, len(self.members), steps=steps, rounds=rounds)
        except BaseException:
            self.alphas = kept
            raise
        self.alphas = self._check_alphas(alphas, len(self.members))
        return self.alphas.copy(), value, trace


# -- the drivers' keys: [BASE] ensemble = <pickle>[, <pickle> ...], ensemble_alpha = a0, a1, ..., ensemble_fit = <seed>[, <metric>] ------
def load_member(conf, path):
    """A further member from a pickle of the four arrays a `--pretrain` / `--dae` run saves ([enc_W, dec_W, enc_b, dec_b];
    a tied model's pickle holds its one matrix twice): an untied `DAE` over the run's vocabulary whose hidden size is the
    pickle's.  Arrays of another vocabulary raise ValueError naming the file."""
    from .DAEs import DAE
    with open(path, "rb") as f:
        emb = pickle.load(f)
    arrs = [np.asarray(x, np.float32) for x in emb[:4]]
    if arrs[0].ndim != 2 or arrs[0].shape != arrs[1].shape or arrs[0].shape[0] != int(conf.n_input):
        raise ValueError("[BASE] ensemble: %s holds matrices of shape %s / %s, the run's vocabulary has %d items"
                         % (path, arrs[0].shape, arrs[1].shape, int(conf.n_input)))
    c = copy.copy(conf)
    c.initval, c.hidden = path, int(arrs[0].shape[1])
    model = DAE(c)
    model._host_init = lambda: arrs
    model.fit()
    return model


def from_conf(conf, model):
    """The ensemble the keys of `conf` ask for around the driver's own fitted `model` (listed first): one more member per
    pickle of conf.ensemble, conf.ensemble_alpha (or uniform weights), titled when `model` carries a title model."""
    members = [model] + [load_member(conf, p) for p in conf.ensemble]
    return DAE_ensemble(members, alphas=getattr(conf, "ensemble_alpha", None), title_model=getattr(model, "title_model", None))


def split_feeds(reader_test, titled, strmaxlen=None):
    """One test split as `rank_of` feeds, batch by batch as the drivers' evaluations read it: (x_positions, x_ones, the held-out
    answers, SEEDS_FROM_INPUT, n_rows) and, `titled`, the titles and titles_use as the title evaluation feeds them (a row
    without a title takes titles_use = 0 and an all-padding title)."""
    pad = [-1] * int(strmaxlen) if titled else None
    while True:
        x_positions, test_seed, test_answer, titles, x_ones = reader_test.next_batch_test()
        feed = (x_positions, x_ones, [list(a) for a in test_answer], SEEDS_FROM_INPUT, len(test_seed))
        if titled:
            use = np.array([0.0 if t is None else 1.0 for t in titles], np.float32)
            feed += ([t if t is not None else pad for t in titles], use)
        yield feed
        if reader_test.test_idx == 0:
            break


def fit_from_conf(conf, ens, titled):
    """[BASE] ensemble_fit = <seed>[, <metric>]: fit `ens.alphas` on that test split (`DAE_ensemble.fit_alphas` over
    `split_feeds`) -> the line the drivers log, or None without the key."""
    if not getattr(conf, "ensemble_fit", None):
        return None
    from ..utils.data_reader import data_reader_test
    split, metric = conf.ensemble_fit
    reader = data_reader_test(data_dir=conf.data_dir, filename=split, batch_size=ens.n_batch, test_num=conf.testsize)
    feeds = list(split_feeds(reader, titled, getattr(conf, "strmaxlen", None)))
    alphas, value, trace = ens.fit_alphas(feeds, metric=metric)
    return "ensemble: fitted alphas %s (%s %f on %s, %d points evaluated)" % (", ".join("%g" % a for a in alphas), metric, value,
                                                                              split, len(trace))
