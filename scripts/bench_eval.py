#!/usr/bin/env python
"""The evaluation of a test split (main_train.py eval) at the bench's size, as playlists/s through
  (a) recommend_iter + utils/metrics.py eval_topk per row -- the loop the driver ran before the metrics moved to the device --
  (b) evaluate_iter (the pipeline's evaluation mode: dae_rank_metrics behind the scoring call, 24 bytes a row come back)
for f32, bf16 and exact_bf16, (a) and (b) alternating in ONE process.  Both must arrive at the same r-precision float or the
run is void (exit status 1).  usage: bench_eval.py [--reps 3] [--modes f32,bf16,exact_bf16] [--feeds-a 100] [--scale-b 1.0]
One JSON line per mode, then a summary line."""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spotify_recsys_challenge_2018_amd.models.DAEs import DAE, SEEDS_FROM_INPUT          # noqa: E402
from spotify_recsys_challenge_2018_amd.utils import metrics as met                         # noqa: E402
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights   # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", default="f32,bf16,exact_bf16")
    ap.add_argument("--feeds-a", type=int, default=100, help="feeds of the timed region of (a): ~25 000 rows/s of eval_topk -> 1 s")
    ap.add_argument("--scale-b", type=float, default=1.0, help="factor on the feeds of the timed region of (b)")
    ap.add_argument("--small", action="store_true", help="a vocabulary of 24 000 (rehearsal)")
    a = ap.parse_args()
    nt, na, H, B, k = (20000, 4000, 256, 250, 500) if a.small else (140000, 30000, 256, 250, 500)
    V = nt + na
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=0, bias="zipf", n_tracks=nt)
    tmp = tempfile.mkdtemp(prefix="bench_eval_")
    path = os.path.join(tmp, "init.pkl")
    with open(path, "wb") as f:
        pickle.dump([W_enc, W_dec, b_enc, b_dec], f)

    class C:
        save = os.path.join(tmp, "unused"); batch = B; n_input = V; hidden = H; lr = 0.005; reg_lambda = 0.0
        n_tracks = nt; initval = path
    # one model per loop: a model keeps ONE pipeline at a time, alternating the loops on one model would time its re-creation
    m = DAE(C()); m.fit()
    m_b = DAE(C()); m_b.fit()
    # the generated split: 16 distinct feeds of 250 playlists; a playlist's answers are tracks the fp32 model lists for it
    # (drawn from anywhere in its top 500) among tracks it does not, 10 - 100 ids, as a held-out half of a playlist would be
    rng = np.random.default_rng(5)
    batches = [make_playlists(B, nt, na, seed=200 + s)[:2] for s in range(16)]
    feeds = [(p, o, SEEDS_FROM_INPUT, B) for p, o in batches]
    answers = []
    for idx, _s in m.recommend_iter(feeds, k=k, want_scores=False, dtype="f32"):
        ans = []
        for row in idx:
            n = int(rng.integers(10, 101))
            hit = rng.choice(row[row >= 0], size=int(rng.integers(0, n // 3 + 1)), replace=False).tolist()
            ans.append([int(x) for x in rng.permutation(hit + rng.choice(nt, size=n - len(hit), replace=False).tolist())])
        answers.append(ans)

    def loop_a(mode, n_feeds):
        total, rows = 0.0, 0
        fs = (feeds[i % len(feeds)] for i in range(n_feeds))
        for b_no, (idx, _s) in enumerate(m.recommend_iter(fs, k=k, want_scores=False, dtype=mode)):
            ans = answers[b_no % len(feeds)]
            for i in range(len(idx)):
                total += met.eval_topk(idx[i], ans[i])
            rows += len(idx)
        return total, rows

    def loop_b(mode, n_feeds):
        total, rows = 0.0, 0
        fs = ((feeds[i % len(feeds)], answers[i % len(feeds)]) for i in range(n_feeds))
        for rec in m_b.evaluate_iter(fs, k=k, dtype=mode):
            for r in met.finish_r_precision_rows(rec):
                total += r
            rows += len(rec)
        return total, rows

    def times_of(model):
        """The host side of the model's pipeline so far (dae_pipeline_times, ms) and its launch counts."""
        for _key, (_g, p) in model.__dict__.get("_pipes", {}).items():
            return dict(p.times(), **p.stats())
        return {}

    def delta(t1, t0):
        return {key: round(v - t0.get(key, 0), 2) for key, v in t1.items()}

    ok = True
    summary = {}
    for mode in a.modes.split(","):
        n_b = int({"f32": 4000, "bf16": 16000, "exact_bf16": 16000}[mode] * a.scale_b)
        loop_a(mode, 32); loop_b(mode, max(64, n_b // 8))                  # warm-up: both pipelines' shapes, the device's clocks
        torch.cuda.synchronize()
        ra, rb, same = [], [], True
        t_a = t_b = None
        for _ in range(a.reps):
            h0 = times_of(m)
            t0 = time.perf_counter(); tot_a, rows_a = loop_a(mode, a.feeds_a); dt_a = time.perf_counter() - t0
            t_a = delta(times_of(m), h0)
            h0 = times_of(m_b)
            t0 = time.perf_counter(); tot_b, rows_b = loop_b(mode, n_b); dt_b = time.perf_counter() - t0
            t_b = dict(delta(times_of(m_b), h0), total_ms=round(dt_b * 1e3, 1))
            # the same r-precision float: (b) over as many feeds as (a) took (the sum's order is the rows' order)
            chk_b, _n = loop_b(mode, a.feeds_a)
            same = same and chk_b / rows_a == tot_a / rows_a
            ra.append(rows_a / dt_a); rb.append(rows_b / dt_b)
            print("# %-10s (a) %9.0f playlists/s over %.2f s   (b) %9.0f playlists/s over %.2f s   rprecision %.6f %s"
                  % (mode, ra[-1], dt_a, rb[-1], dt_b, tot_a / rows_a, "same" if same else "DIFFERENT"), flush=True)
        ok = ok and same
        row = {"mode": mode, "a_playlists_per_s": [round(x) for x in ra], "b_playlists_per_s": [round(x) for x in rb],
               "a_spread": round((max(ra) - min(ra)) / max(ra), 4), "b_over_a_median": round(float(np.median(rb) / np.median(ra)), 2),
               "same_rprecision": same, "pipeline_a": t_a, "pipeline_b": t_b}
        summary[mode] = row["b_over_a_median"]
        print(json.dumps(row), flush=True)
    print(json.dumps({"bench_eval": "b_over_a_median", **summary, "valid": ok}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
