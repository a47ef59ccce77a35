"""Choosing an ensemble's alphas (models/ensemble.py `DAE_ensemble.fit_alphas`; DESIGN.md section 4e "Ranks under the
ensemble"): a deterministic, device-free search over the simplex grid

    { (i_0, ..., i_{M-1}) / steps : i_m integers >= 0, sum i_m = steps }

for the point where `evaluate(alphas) -> float` (higher is better) is largest.  `evaluate` is a black box -- in `fit_alphas`
one pass of `rank_of` over a split and a metric of the ranks -- so the search spends evaluations sparingly and never twice
on one point.
"""
import numpy as np

from . import metrics as met


def grid_alphas(point, steps):
    """A grid point (integers summing to `steps`) -> the float32 alphas an ensemble takes: float32(i) / float32(steps)."""
    return (np.asarray(point, np.float32) / np.float32(steps)).astype(np.float32)


def search_simplex(evaluate, M, steps=10, rounds=4):
    """-> (alphas float32 [M], value, trace).  trace: [(alphas float32 [M], value)] of every evaluated point, each once, in the
    order of evaluation.

    M = 1: [1], one evaluation.
    M = 2: all steps + 1 points, alpha_0 ascending; the best wins, ties to the earlier point.
    M > 2: start from the best of the M corners (member 0's first) and the centre (steps split evenly, the remainder to the
      first members), ties to the earlier candidate; then up to `rounds` sweeps over the ordered pairs (i, j), i != j, in
      lexicographic order: where alpha_j > 0 one grid step moves from j to i, and the move is kept only if the value is
      STRICTLY larger.  A sweep that keeps nothing ends the search."""
    M, steps, rounds = int(M), int(steps), int(rounds)
    if M < 1 or steps < 1 or rounds < 0:
        raise ValueError("search_simplex: M >= 1, steps >= 1 and rounds >= 0 are required (got %d, %d, %d)" % (M, steps, rounds))
    memo, trace = {}, []

    def value(point):
        point = tuple(int(i) for i in point)
        if point not in memo:
            a = grid_alphas(point, steps)
            memo[point] = float(evaluate(a))
            trace.append((a, memo[point]))
        return memo[point]

    def best_of(points):
        best = None
        for pt in points:
            v = value(pt)
            if best is None or v > best[1]:
                best = (tuple(pt), v)
        return best

    if M == 1:
        cur, cur_v = best_of([(steps,)])
    elif M == 2:
        cur, cur_v = best_of([(i, steps - i) for i in range(steps + 1)])
    else:
        corners = [tuple(steps if m == c else 0 for m in range(M)) for c in range(M)]
        centre = tuple(steps // M + (1 if m < steps % M else 0) for m in range(M))
        cur, cur_v = best_of(corners + [centre])
        for _ in range(rounds):
            moved = False
            for i in range(M):
                for j in range(M):
                    if i == j or cur[j] == 0:
                        continue
                    cand = list(cur)
                    cand[i] += 1
                    cand[j] -= 1
                    v = value(cand)
                    if v > cur_v:
                        cur, cur_v, moved = tuple(cand), v, True
            if not moved:
                break
    return grid_alphas(cur, steps), cur_v, trace


def parse_metric(metric):
    """"mrr" or "recall@N" -> a function of a rank array (-1 = a miss that counts in the denominator), higher is better."""
    if metric == "mrr":
        return met.mean_reciprocal_rank
    if isinstance(metric, str) and metric.startswith("recall@"):
        try:
            n = int(metric[len("recall@"):])
        except ValueError:
            n = 0
        if n >= 1:
            return lambda ranks: float(met.recall_at(ranks, [n])[0])
    raise ValueError("metric %r: \"mrr\" or \"recall@N\" with an integer N >= 1" % (metric,))
