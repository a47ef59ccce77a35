"""Ranking metrics of the reference's utils/metrics.py, kept as the drop-in contract
(north_star: "utils/metrics.py r-precision").  Citations relative to /root/reference.

Differences from the snapshot: `get_metrics`/`single_eval` there unpack three
values from a scalar and always raise; here they return the r-precision, which is what the
training driver accumulates (main_train.py:89-100).  The ranking inside `single_eval` is NOT done
on the host: dense scores are ranked by the HIP top-k kernel (dae_topk_dense) with the canonical
tie rule, and the drivers of this repo never build dense scores at all (they call
`model.recommend`).
"""
import math

import numpy as np


def get_r_precision(answer, cand, answer_cls=None, class_divpnt=None):
    """metrics.py:20-27: |set(answer) & set(cand[:len(answer)])| / len(answer).
    `answer` may contain -1 (tracks outside the vocabulary, spotify_reader.py:271-273): they can
    never be hit but do count in the denominator.  The two class arguments are accepted and
    ignored, as in the reference."""
    n = len(answer)
    if n == 0:
        raise ZeroDivisionError("empty answer list")
    return len(set(answer) & set(cand[:n])) / n


def get_ndcg(answer, cand):
    """metrics.py:29-42 (NB: the reference's IDCG grows with the number of HITS, not with
    len(answer); kept as is)."""
    dcg = 1.0 if cand[0] in answer else 0.0
    idcg, next_ideal = 1.0, 2
    for pos in range(1, len(cand)):
        if cand[pos] in answer:
            dcg += 1.0 / math.log(pos + 1, 2)
            idcg += 1.0 / math.log(next_ideal, 2)
            next_ideal += 1
    return dcg / idcg


def get_rsc(answer, cand):
    """metrics.py:44-49: recommended-songs clicks = index of the first hit // 10, 51 if none."""
    for pos, c in enumerate(cand):
        if c in answer:
            return pos // 10
    return 51


def get_metrics(answer, cand, answer_cls=None, num_cls=None):
    """metrics.py:51-56, repaired: r-precision only (ndcg / rsc are commented out upstream)."""
    return get_r_precision(answer, cand, answer_cls, num_cls)


_ctx = None


def _rank_dense_on_gpu(scores, seed, k):
    """metrics.py:59-68 ranking (argsort desc, remove seeds, first 500) on the GPU."""
    import torch

    from .. import _lib
    global _ctx
    if _ctx is None:
        _ctx = _lib.Context(0)
    _ctx.bind_stream()
    s = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32).reshape(1, -1)).cuda()
    n = s.shape[1]
    sd = np.unique(np.asarray([x for x in seed if 0 <= x < n], dtype=np.int32))
    srp = torch.tensor([0, sd.size], dtype=torch.int32, device="cuda")
    sc = torch.from_numpy(sd if sd.size else np.zeros(1, np.int32)).cuda()
    out_s = torch.empty((1, k), dtype=torch.float32, device="cuda")
    out_i = torch.empty((1, k), dtype=torch.int32, device="cuda")
    # scores are already sigmoid outputs: rank them as they are (DAE_OUT_LOGIT = raw values)
    _ctx.topk_dense(s, n, 0, srp, sc, k, out_s, out_i, out_kind=_lib.DAE_OUT_LOGIT)
    idx = out_i.cpu().numpy()[0]
    return [int(i) for i in idx if i >= 0]


def single_eval(scores, seed, answer, answer_cls=None, num_cls=None, k=500):
    """metrics.py:58-70, repaired: rank one row of track scores, drop the seeds, keep 500, return
    the r-precision."""
    cand = _rank_dense_on_gpu(np.asarray(scores), seed, k)
    return get_metrics(answer, cand, answer_cls, num_cls)


def eval_topk(cand_idx, answer):
    """r-precision of an already ranked candidate row (output of model.recommend)."""
    cand = [int(i) for i in cand_idx if i >= 0]
    return get_r_precision(answer, cand)


# ---- the three metrics as a per-row RECORD (what dae_rank_metrics leaves on the device, include/dae_hip.h) ----------------
#
# {hits_r, first, m, n_answer, dcg}: counts and one float64 sum of additions; the divisions are done here, in Python, so the
# floats are the functions' above bit for bit (tests/test_metrics_cpu.py, tests/test_gpu_metrics.py).

RECORD_DTYPE = np.dtype([("hits_r", np.int32), ("first", np.int32), ("m", np.int32), ("n_answer", np.int32),
                         ("dcg", np.float64)])
_disc, _idcg = [0.0], [1.0]          # disc[p] = 1 / math.log(p + 1, 2) (disc[0] is never used); idcg[m] = 1 + disc[1] + ... + disc[m]


def discount_table(k):
    """The first k discounts of get_ndcg, from Python's own math.log (the table the device kernel adds from)."""
    while len(_disc) < max(int(k), 1):
        p = len(_disc)
        _disc.append(1.0 / math.log(p + 1, 2))
        _idcg.append(_idcg[-1] + _disc[-1])
    return np.array(_disc[:int(k)], np.float64)


def rank_records(idx, answers):
    """The records of the rows of `idx` [n, k] (ids, -1 = no candidate) against `answers` (n id lists) on the host: the
    restatement of csrc/metrics.hip that `evaluate_iter` uses for the feeds the native loop does not take."""
    idx = np.asarray(idx)
    out = np.zeros(len(answers), RECORD_DTYPE)
    discount_table(idx.shape[1] if idx.ndim == 2 and idx.shape[1] else 1)
    for r, answer in enumerate(answers):
        row = idx[r]
        cand = row[row >= 0]
        n = len(answer)
        pos = np.flatnonzero(np.isin(cand, np.asarray(answer, np.int64))) if n else np.zeros(0, np.int64)
        dcg = 0.0
        for p in pos.tolist():                   # (float64 additions in ascending position, as get_ndcg adds them)
            dcg = 1.0 if p == 0 else dcg + _disc[p]
        out[r] = (int(np.count_nonzero(pos < n)), int(pos[0]) if pos.size else -1, int(np.count_nonzero(pos >= 1)), n, dcg)
    return out


def finish_r_precision(rec):
    """get_r_precision of one record (an empty answer list raises, as it does there)."""
    n = int(rec["n_answer"])
    if n == 0:
        raise ZeroDivisionError("empty answer list")
    return int(rec["hits_r"]) / n


def finish_ndcg(rec):
    """get_ndcg of one record; 0.0 for a row without candidates (get_ndcg raises IndexError there)."""
    m = int(rec["m"])
    discount_table(m + 1)
    return float(rec["dcg"]) / _idcg[m]


def finish_rsc(rec):
    """get_rsc of one record."""
    first = int(rec["first"])
    return first // 10 if first >= 0 else 51


def finish_record(rec):
    """-> (r-precision, NDCG, clicks) of one record."""
    return finish_r_precision(rec), finish_ndcg(rec), finish_rsc(rec)


def finish_r_precision_rows(rec):
    """finish_r_precision of every record of an array, as a list of Python floats (the same int / int divisions)."""
    return [h / n for h, n in zip(rec["hits_r"].tolist(), rec["n_answer"].tolist())]      # (n = 0: ZeroDivisionError)


def finish_ndcg_rows(rec):
    ms = rec["m"].tolist()
    discount_table(max(ms, default=0) + 1)
    return [d / _idcg[m] for d, m in zip(rec["dcg"].tolist(), ms)]


def finish_rsc_rows(rec):
    return [f // 10 if f >= 0 else 51 for f in rec["first"].tolist()]


# ---- metrics over EXACT ranks (models/DAEs.py rank_of): pure host helpers over a rank array -------------------------------------
# `ranks`: any int array of 0-based ranks, -1 for an answer that could not be ranked (a track outside the vocabulary, padding).
# Such an answer is a miss: it can never be hit but counts in every denominator, as a -1 answer counts in get_r_precision.
def _rank_array(ranks):
    r = np.asarray(ranks, dtype=np.int64).reshape(-1)
    if r.size and r.min() < -1:
        raise ValueError("ranks: 0-based ranks or -1, got %d" % r.min())
    return r


def reciprocal_rank(ranks):
    """Per answer 1 / (rank + 1), 0.0 for a rank of -1 -> float64 array of the input's shape."""
    r = np.asarray(ranks, dtype=np.int64)
    _rank_array(r)
    out = np.zeros(r.shape, np.float64)
    ok = r >= 0
    out[ok] = 1.0 / (r[ok] + 1.0)
    return out


def mean_reciprocal_rank(ranks):
    """MRR over all answers, the unranked ones counting 0 (0.0 for no answers)."""
    rr = reciprocal_rank(ranks).reshape(-1)
    return float(rr.mean()) if rr.size else 0.0


def mean_rank(ranks):
    """Mean of the ranks of the RANKED answers (nan when there is none): a miss has no rank to average."""
    r = _rank_array(ranks)
    r = r[r >= 0]
    return float(r.mean()) if r.size else float("nan")


def median_rank(ranks):
    """Median of the ranks of the ranked answers (nan when there is none)."""
    r = _rank_array(ranks)
    r = r[r >= 0]
    return float(np.median(r)) if r.size else float("nan")


def recall_at(ranks, ks):
    """The recall curve at every cut-off at once: for each k of `ks` the share of the answers with 0 <= rank < k, among ALL
    answers (-1 included in the denominator) -> float64 array [len(ks)] (zeros for no answers)."""
    r = _rank_array(ranks)
    ks = np.asarray(ks, dtype=np.int64).reshape(-1)
    if r.size == 0:
        return np.zeros(ks.size, np.float64)
    hit = np.sort(r[r >= 0])
    return np.searchsorted(hit, ks, side="left") / float(r.size)


def auc_row(ranks, n_rankable):
    """AUC of one row from the ranks of its answers among n_rankable columns:

        AUC = 1 - rank_mean_corrected / (n_rankable - 1),
        rank_mean_corrected = mean over the row's distinct ranked answers, sorted ascending r_(0) < r_(1) < ..., of r_(i) - i

    r_(i) - i is the number of NON-answer columns ranked before answer i (the i answers before it taken out), so for a single
    answer this is 1 - rank / (n_rankable - 1): 1.0 at rank 0, 0.0 at the last rank.  With P answers the non-answers number
    n_rankable - P, so the value is the pairwise AUC times (n_rankable - P) / (n_rankable - 1): off by P / n_rankable at most.
    Unranked answers (-1) take no part; nan for a row without a ranked answer or with n_rankable < 2."""
    r = _rank_array(ranks)
    r = np.unique(r[r >= 0])
    if r.size == 0 or n_rankable < 2:
        return float("nan")
    if r[-1] >= n_rankable:
        raise ValueError("rank %d among %d rankable columns" % (r[-1], n_rankable))
    corrected = r - np.arange(r.size)
    return 1.0 - float(corrected.mean()) / (n_rankable - 1.0)
