"""GPU (-m gpu): dae_rank_metrics (csrc/metrics.hip) through the C ABI against utils/metrics.py get_r_precision / get_ndcg /
get_rsc -- every field of every record bit for bit (the DCG as float64 bits), and the three finished metrics with ==.  No
tolerance anywhere: an approximate compare would hide a reassociated sum."""
import numpy as np
import pytest

from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.utils import metrics as met
from test_metrics_cpu import KINDS, make_case, reference

pytestmark = pytest.mark.gpu

CAP = 1024          # answers the kernel holds in LDS at a time (csrc/metrics.hip MET_CAP)


def run(ctx, rows, answers, k, ld=None, disc=None):
    import torch
    B = len(rows)
    ld = ld or k
    idx = np.full((B, ld), 12345, np.int32)              # (columns past k are never read: a hit there would show)
    idx[:, :k] = np.stack(rows)
    rp = np.zeros(B + 1, np.int32)
    rp[1:] = np.cumsum([len(a) for a in answers])
    col = np.asarray([x for a in answers for x in a] or [0], np.int32)
    d_idx = torch.from_numpy(idx).cuda()
    out = ctx.rank_metrics(d_idx[:, :k] if ld != k else d_idx, k, torch.from_numpy(rp).cuda(), torch.from_numpy(col).cuda(),
                           disc=None if disc is None else torch.from_numpy(disc).cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(-1).view(met.RECORD_DTYPE)


def check(rec, rows, answers):
    want = met.rank_records(np.stack(rows), answers)
    for f in ("hits_r", "first", "m", "n_answer"):
        assert np.array_equal(rec[f], want[f]), f
    assert np.array_equal(rec["dcg"].view(np.uint64), want["dcg"].view(np.uint64))
    for r in range(0, len(rows), max(1, len(rows) // 256)):          # (the reference functions are O(k n) per row in Python)
        if len(answers[r]):
            assert met.finish_record(rec[r]) == reference(rows[r], answers[r]), r


@pytest.mark.parametrize("B", [1, 250, 2048])
@pytest.mark.parametrize("k", [1, 10, 500, 1024])
def test_rank_metrics_equals_the_python_functions(B, k):
    ctx = _lib.Context(0)
    rng = np.random.default_rng(1000 * k + B)
    rows, answers = [], []
    for i in range(B):
        row, answer = make_case(rng, k, KINDS[(i + 5 * (B == 1)) % len(KINDS)])       # (B = 1: a list without candidates)
        rows.append(row); answers.append(answer)
    check(run(ctx, rows, answers, k), rows, answers)
    if B == 250:
        check(run(ctx, rows, answers, k, ld=k + 7), rows, answers)                   # ld > k
    ctx.close()


@pytest.mark.parametrize("k", [10, 500, 1024])
def test_long_answer_rows_around_and_past_the_lds_pass(k):
    """Answer rows of CAP - 1, CAP, CAP + 1, 2 CAP, 2 CAP + 1 and a few thousand ids: the hits sit in every pass, the last id
    of a row included; one list is all -1; one answer row is empty (the record is marked invalid, nothing is divided)."""
    ctx = _lib.Context(0)
    rng = np.random.default_rng(7 + k)
    rows, answers = [], []
    for n in (1, CAP - 1, CAP, CAP + 1, 2 * CAP, 2 * CAP + 1, 3000, 5000, 4097, 0, 333):
        cand = rng.choice(3000, size=k, replace=False)
        row = cand.astype(np.int64)
        if n == 4097:
            row[:] = -1
        if n == 333:
            row[k // 2:] = -1
        answer = (10000 + rng.choice(20000, size=n, replace=False)).tolist()
        if n:
            where = sorted(set([0, n - 1, n // 2] + rng.integers(0, n, size=min(n, 40)).tolist()))
            picks = rng.choice(cand, size=min(len(where), k), replace=False)
            for w, c in zip(where, picks):
                answer[w] = int(c)
            if n > 8:
                answer[3] = -1; answer[5] = answer[where[-1]]
        rows.append(row); answers.append(answer)
    rec = run(ctx, rows, answers, k)
    check(rec, rows, answers)
    assert rec["n_answer"][9] == 0 and rec["hits_r"][9] == 0
    with pytest.raises(ZeroDivisionError):
        met.finish_r_precision(rec[9])
    assert met.finish_record(rec[8]) == (0.0, 0.0, 51)                               # no candidates: NDCG defined as 0.0
    assert rec["m"].max() > 0
    ctx.close()


def test_the_sum_follows_the_callers_table_in_position_order():
    """A table whose sum depends on the order of its additions (1e16, then ones) comes back as the ascending-position sum."""
    ctx = _lib.Context(0)
    k = 500
    disc = np.ones(k, np.float64)
    disc[1] = 1e16
    row = np.arange(k, dtype=np.int64)
    answer = list(range(0, 400))
    rec = run(ctx, [row], [answer], k, disc=disc)
    want = 1.0
    for p in range(1, 400):
        want += disc[p]
    other = 0.0
    for p in range(399, 0, -1):
        other += disc[p]
    assert rec["dcg"][0] == want and want != other + 1.0
    assert rec["hits_r"][0] == 400 and rec["m"][0] == 399 and rec["first"][0] == 0
    ctx.close()


def test_bad_arguments_are_errors():
    import torch
    ctx = _lib.Context(0)
    idx = torch.zeros((2, 8), dtype=torch.int32, device="cuda")
    rp = torch.zeros(3, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.DaeError):
        ctx.rank_metrics(idx, 2000, rp, rp)
    with pytest.raises(_lib.DaeError):
        ctx.rank_metrics(idx, 0, rp, rp)
    ctx.close()
