#!/usr/bin/env python
"""Exact ranks under an ensemble's y through the fused call against the route a caller had before it, on the same device in the
same session: V = 170 000, 140 000 tracks, hidden 256 (every member), title feature rows of 448, 256 rows; M = 2 and 3 members,
untitled and titled; 10, 100 and 250 answers per row.  Inputs are resident (hidden rows, feature rows, weights, lists, outputs).

  fused   dae_ensemble_rank_of(answers)
  dense   per scorer dae_decode_dense with the sigmoid into a [B, V] matrix, the weighted sum in torch in the canonical order, the
          seeds set to -inf, torch.sort of the track columns + torch.searchsorted of the answers' own scores -- none of it is
          code of the fused call

and, per case, the launches in front of the counting launch timed alone -- the term launches (dae_decode_mix_term / _add for the
members in acc), dae_ensemble_candidates over the answers and over the seed CSR -- so that what is left, the sort, the count and
the finish, can be read off: fused - terms - candidates.

Device time per call, `--iters` calls between two events, the median of `--runs` alternating runs (fused, dense, ...), all values
printed.  The two routes' ranks are compared before anything is timed: the dense route gives tied scores one shared rank and
knows no column order, so "answers that differ" is reported, not required to be 0; a tie can only add to the canonical rank, and
the differences that is not true of are counted too (0 expected).  Prints one line per case and a final JSON line; `--out FILE`
also writes the JSON there.

`--fit`: the wall time of one DAE_ensemble.fit_alphas (M = 2, steps = 10, 11 evaluations) over a split of `--playlists` (1 000)
playlists with `--fit-answers` (25) held-out tracks each, in feeds of `--rows` rows, models of the same shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spotify_recsys_challenge_2018_amd import _lib                                                # noqa: E402
from spotify_recsys_challenge_2018_amd.models.DAEs import DAE, SEEDS_FROM_INPUT, coo_to_csr, seeds_to_csr   # noqa: E402
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights        # noqa: E402


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters          # ms per call


def fit(a):
    from spotify_recsys_challenge_2018_amd.models.ensemble import DAE_ensemble
    import torch
    nt, na, H, B = a.tracks, a.artists, a.hidden, a.rows
    V = nt + na

    class Conf:
        batch = B; n_input = V; n_tracks = nt; hidden = H; lr = 0.005; reg_lambda = 0.0; save = "/tmp/_bench_unused"; initval = "NULL"
    members = []
    for seed in (0, 1):
        m = DAE(Conf())
        W = make_weights(V, H, seed=seed, bias="zipf", n_tracks=nt)
        m._host_init = lambda W=W: [W[0], W[2], W[1], W[3]]
        m.fit()
        members.append(m)
    rng = np.random.default_rng(3)
    feeds = []
    for lo in range(0, a.playlists, B):
        n = min(B, a.playlists - lo)
        pos, ones, _seeds = make_playlists(n, nt, na, seed=10 + lo)
        feeds.append((pos, ones, [rng.integers(0, nt, a.fit_answers).tolist() for _ in range(n)], SEEDS_FROM_INPUT, n))
    ens = DAE_ensemble(members)
    ens.fit_alphas(feeds, steps=2)                             # the warm-up: images packed, scratch grown
    ens.alphas = ens._check_alphas(None, 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    alphas, value, trace = ens.fit_alphas(feeds, steps=10)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = {"fit": True, "V": V, "tracks": nt, "H": H, "B": B, "playlists": a.playlists, "answers_per_playlist": a.fit_answers,
           "feeds": len(feeds), "points": len(trace), "wall_s": dt, "alphas": alphas.tolist(), "mrr": value}
    print("fit_alphas(M = 2, steps = 10) over %d playlists x %d answers in %d feeds of <= %d rows: %.3f s wall, %d points, %.1f ms per "
          "point" % (a.playlists, a.fit_answers, len(feeds), B, dt, len(trace), 1e3 * dt / len(trace)))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=140000)
    ap.add_argument("--artists", type=int, default=30000)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--ld-feat", type=int, default=448, help="width of the title feature rows")
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--members", type=int, nargs="*", default=[2, 3])
    ap.add_argument("--answers", type=int, nargs="*", default=[10, 100, 250])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fit", action="store_true", help="the wall time of one fit_alphas instead")
    ap.add_argument("--playlists", type=int, default=1000)
    ap.add_argument("--fit-answers", type=int, default=25)
    a = ap.parse_args()
    if a.fit:
        return fit(a)
    nt, na, H, B, F = a.tracks, a.artists, a.hidden, a.rows, a.ld_feat
    V = nt + na
    M_max = max(a.members)
    pos, ones, seeds = make_playlists(B, nt, na, seed=1)
    rp, col, val = coo_to_csr(pos, ones, B, V)
    srp, sc = seeds_to_csr(seeds, B, nt)
    rng = np.random.default_rng(2)

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_rp, d_col, d_val, d_srp, d_sc = dev(rp), dev(col), dev(val), dev(srp), dev(sc)
    seed_rows = dev(np.repeat(np.arange(B, dtype=np.int64), np.diff(srp)))
    seed_cols = dev(sc.astype(np.int64))
    ctxs, hs, Wd, bd = [], [], [], []
    for m in range(M_max):
        W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=m, bias="zipf", n_tracks=nt)
        c = _lib.Context(0)
        Wd.append(dev(W_dec)); bd.append(dev(b_dec))
        c.prepack_decoder(Wd[-1], bd[-1], dtype=_lib.DAE_DTYPE_F32)
        h = torch.empty((B, H), device="cuda")
        c.encode(d_rp, d_col, d_val, dev(W_enc), dev(b_enc), h)
        ctxs.append(c); hs.append(h)
    OutW_T = (rng.standard_normal((V, F)) * 0.05).astype(np.float32)
    Out_b = (b_dec + rng.standard_normal(V).astype(np.float32)).astype(np.float32)        # a popularity prior of its own
    d_Wt, d_bt = dev(OutW_T), dev(Out_b)
    tc = _lib.Context(0)
    tc.prepack_decoder(d_Wt, d_bt, dtype=_lib.DAE_DTYPE_F32)
    d_feat = dev((np.abs(rng.standard_normal((B, F))) * 0.5).astype(np.float32))
    x_count = np.bincount(np.repeat(np.arange(B), np.diff(rp)), weights=val.astype(np.float64), minlength=B).astype(np.float32)
    deno = np.float32(1.0) + x_count + np.float32(1e-10)                                  # titles_use = 1 on every row
    w_t, w_p = (np.float32(1.0) / deno).astype(np.float32), (x_count / deno).astype(np.float32)
    d_wt = dev(w_t)
    dense_m = torch.empty((B, V), device="cuda")
    nt32 = min((nt + 31) // 32 * 32, V)
    accT = torch.empty((nt32, B), device="cuda")
    neg_inf = torch.tensor(float("-inf"), device="cuda")
    res = {"V": V, "tracks": nt, "H": H, "ld_feat": F, "B": B, "iters": a.iters, "runs": a.runs, "cases": []}
    print("V = %d, tracks = %d, hidden = %d, ld_feat = %d, rows = %d; ms per call (device), median of %d alternating runs of %d calls"
          % (V, nt, H, F, B, a.runs, a.iters))
    for titled in (False, True):
        for M in a.members:
            alpha = (rng.random((M, B)) * 0.9 + 0.1).astype(np.float32)
            a_m = [dev(alpha[m] * w_p if titled else alpha[m]) for m in range(M)]
            mem, h_m, W_m, b_m = ctxs[:M], hs[:M], Wd[:M], bd[:M]
            ranker = tc if titled else mem[-1]
            kw = dict(feat=d_feat, OutW_T=d_Wt, Out_b=d_bt, w_title=d_wt) if titled else {}
            n_acc = M if titled else M - 1
            for A in a.answers:
                cols = rng.integers(0, nt, (B, A))
                d_ans = (dev(np.arange(B + 1, dtype=np.int32) * A), dev(cols.reshape(-1).astype(np.int32)))
                d_cols64 = dev(cols.astype(np.int64))
                rank = torch.empty(B * A, dtype=torch.int32, device="cuda")
                ya = torch.empty(max(B * A, int(d_sc.numel())), dtype=torch.float32, device="cuda")
                status = torch.zeros(1, dtype=torch.int32, device="cuda")

                def fused():
                    ranker.ensemble_rank_of(mem, h_m, a_m, W_m, b_m, nt, d_srp, d_sc, d_ans, B * A, rank, status=status, **kw)

                def dense():
                    def term(ctx, h, w):
                        ctx.decode_dense(h, dense_m, apply_sigmoid=True)
                        return dense_m[:, :nt] * w[:, None]
                    acc = None
                    for m in range(n_acc):
                        t = term(mem[m], h_m[m], a_m[m])
                        acc = t if acc is None else acc + t
                    last = term(tc, d_feat, d_wt) if titled else term(mem[-1], h_m[-1], a_m[-1])
                    y = last if acc is None else last + acc
                    y.index_put_((seed_rows, seed_cols), neg_inf)
                    mine = torch.gather(y, 1, d_cols64)
                    srt = torch.sort(-y, dim=1).values                 # ascending of -y = scores descending
                    r = torch.searchsorted(srt, -mine)                 # how many scores are strictly larger
                    return torch.where(torch.isneginf(mine), torch.full_like(r, -1), r)

                def terms():
                    for m in range(n_acc):
                        (mem[m].decode_mix_term if m == 0 else mem[m].decode_mix_term_add)(h_m[m], a_m[m], nt, accT)

                def cands_answers():
                    ranker.ensemble_candidates(mem, h_m, a_m, W_m, b_m, d_ans, B * A, ya, **kw)

                def cands_seeds():
                    ranker.ensemble_candidates(mem, h_m, a_m, W_m, b_m, (d_srp, d_sc), int(d_sc.numel()), ya, **kw)

                fused(); want = dense(); terms(); cands_answers(); cands_seeds()           # (also the warm-up of every route)
                got = rank.view(B, A).to(torch.int64)
                differ = int((got != want).sum().item())
                # a tie can only ADD the tied smaller columns to the canonical rank: anything else would be an error of one route
                unexplained = int((((got < 0) != (want < 0)) | (got < want)).sum().item())
                plan = _lib.rank_of_plan(B, F if titled else H, B * A)
                passes = -(-A // plan["capacity"])
                routes = (fused, dense, terms, cands_answers, cands_seeds)
                t = [[] for _ in routes]
                for _ in range(a.runs):
                    for i, fn in enumerate(routes):
                        t[i].append(timed(fn, a.iters))
                mf, md, mt, mca, mcs = (float(np.median(x)) for x in t)
                spread = max(max(t[0]) - min(t[0]), max(t[1]) - min(t[1]))
                case = {"titled": titled, "members": M, "answers_per_row": A, "answers_that_differ": differ,
                        "differences_no_tie_explains": unexplained, "fused_ms": t[0], "dense_ms": t[1], "terms_ms": t[2],
                        "candidates_answers_ms": t[3], "candidates_seeds_ms": t[4], "fused_median_ms": mf, "dense_median_ms": md,
                        "terms_median_ms": mt, "candidates_answers_median_ms": mca, "candidates_seeds_median_ms": mcs,
                        "sort_count_finish_ms": mf - mt - mca - mcs,
                        "fused_ahead_in_every_pair": all(x < y_ for x, y_ in zip(t[0], t[1])),
                        "medians_apart_by_3_spreads": bool(abs(md - mf) >= 3 * spread), "rows_per_group": plan["rows"],
                        "answers_per_pass": plan["capacity"], "passes": passes}
                res["cases"].append(case)
                print("%-8s M = %d %3d answers/row: fused %8.3f ms (%s)  dense route %8.3f ms (%s)  ratio %.2fx  every pair ahead: %s  "
                      "3 x spread: %s  %d-row groups, %d answers/pass, %d pass(es)  terms %.3f ms  candidates: answers %.3f ms, seeds "
                      "%.3f ms  the rest (sort, count, finish) %.3f ms  %d of %d answers differ (%d not by ties)"
                      % ("titled" if titled else "untitled", M, A, mf, " ".join("%.3f" % x for x in t[0]), md,
                         " ".join("%.3f" % x for x in t[1]), md / mf, case["fused_ahead_in_every_pair"],
                         case["medians_apart_by_3_spreads"], plan["rows"], plan["capacity"], passes, mt, mca, mcs,
                         case["sort_count_finish_ms"], differ, B * A, unexplained))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for c in ctxs + [tc]:
        c.close()


if __name__ == "__main__":
    main()
