#!/usr/bin/env python
"""Exact ranks of given tracks through the fused call against the route a caller had before it, on the same device in the same
session: V = 170 000, 140 000 tracks, hidden 256, 256 rows.

  fused   dae_score_rank_of(answers)
  dense   dae_encode + dae_decode_dense (logits) into [B, V] + the seeds set to -inf + torch.sort of the track columns +
          torch.searchsorted of the answers' own logits -- none of it is code of rank_of

per (model, answers per row) for the zipf bench model and the same weights with b_dec = 0, and 10, 100 and 250 answers per row.
Everything is resident on the device (the CSR, the seed CSR, the seeds' flat index, the answers, the outputs): the figures are
device time per call, `--iters` calls between two events, the median of `--runs` alternating runs (fused, dense, fused, dense,
...), all values printed.  The two routes' ranks are compared before anything is timed: the dense route gives tied logits one
shared rank and knows no column order, so "answers that differ" is reported, not required to be 0; a tie can only add to the
canonical rank, and the differences that is not true of are counted too (0 expected).  Each case also reports the
plan (rows per row group, answers per pass, passes of the GEMM).  Prints one line per case and a final JSON line; `--out FILE`
also writes the JSON there.

`--titled`: the same for the ranks under the title mix at title feature rows of `--ld-feat` (448), inputs resident (hidden rows,
feature rows, mixing weights):

  fused   dae_mix_rank_of(answers)
  dense   mixed_scores' launches (dae_decode_dense with the sigmoid on both contexts into two [B, V] matrices + dae_mix_scores) +
          the seeds masked + torch.sort of the track columns + torch.searchsorted of the answers' own scores

and, per case, the two launches in front of the counting launch timed alone (dae_decode_mix_term: the transposed DAE term;
dae_mix_candidates over the answers), so that the pass cost can be read off: fused - term - candidates."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spotify_recsys_challenge_2018_amd import _lib                                                # noqa: E402
from spotify_recsys_challenge_2018_amd.models.DAEs import coo_to_csr, seeds_to_csr               # noqa: E402
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


def titled(a):
    import torch
    nt, na, H, B, F = a.tracks, a.artists, a.hidden, a.rows, a.ld_feat
    V = nt + na
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=0, bias="zipf", n_tracks=nt)
    pos, ones, seeds = make_playlists(B, nt, na, seed=1)
    rp, col, val = coo_to_csr(pos, ones, B, V)
    srp, sc = seeds_to_csr(seeds, B, nt)
    rng = np.random.default_rng(2)
    OutW_T = (rng.standard_normal((V, F)) * 0.05).astype(np.float32)
    Out_b = (b_dec + rng.standard_normal(V).astype(np.float32)).astype(np.float32)        # a popularity prior of its own
    feat = (np.abs(rng.standard_normal((B, F))) * 0.5).astype(np.float32)
    x_count = np.bincount(np.repeat(np.arange(B), np.diff(rp)), weights=val.astype(np.float64), minlength=B).astype(np.float32)
    deno = np.float32(1.0) + x_count + np.float32(1e-10)                                  # titles_use = 1 on every row
    w_t, w_p = (np.float32(1.0) / deno).astype(np.float32), (x_count / deno).astype(np.float32)

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_rp, d_col, d_val, d_srp, d_sc = dev(rp), dev(col), dev(val), dev(srp), dev(sc)
    d_We, d_be, d_Wd, d_bd, d_Wt, d_bt = dev(W_enc), dev(b_enc), dev(W_dec), dev(b_dec), dev(OutW_T), dev(Out_b)
    d_feat, d_wt, d_wp = dev(feat), dev(w_t), dev(w_p)
    seed_rows = dev(np.repeat(np.arange(B, dtype=np.int64), np.diff(srp)))
    seed_cols = dev(sc.astype(np.int64))
    tc, dc = _lib.Context(0), _lib.Context(0)
    dc.prepack_decoder(d_Wd, d_bd, dtype=_lib.DAE_DTYPE_F32)
    tc.prepack_decoder(d_Wt, d_bt, dtype=_lib.DAE_DTYPE_F32)
    h = torch.empty((B, H), device="cuda")
    dc.encode(d_rp, d_col, d_val, d_We, d_be, h)
    y = torch.empty((B, V), device="cuda")
    ts = torch.empty((B, V), device="cuda")
    nt32 = min((nt + 31) // 32 * 32, V)
    termT = torch.empty((nt32, B), device="cuda")
    neg_inf = torch.tensor(float("-inf"), device="cuda")
    P = _lib._ptr
    res = {"titled": True, "V": V, "tracks": nt, "H": H, "ld_feat": F, "B": B, "iters": a.iters, "runs": a.runs, "cases": []}
    print("titled: V = %d, tracks = %d, hidden = %d, ld_feat = %d, rows = %d; ms per call (device), median of %d alternating runs of "
          "%d calls" % (V, nt, H, F, B, a.runs, a.iters))
    for A in a.answers:
        cols = rng.integers(0, nt, (B, A))
        d_ans = (dev(np.arange(B + 1, dtype=np.int32) * A), dev(cols.reshape(-1).astype(np.int32)))
        d_cols64 = dev(cols.astype(np.int64))
        rank = torch.empty(B * A, dtype=torch.int32, device="cuda")
        ya = torch.empty(B * A, dtype=torch.float32, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")

        def fused():
            tc.mix_rank_of(dc, h, d_Wd, d_bd, d_feat, d_Wt, d_bt, d_wt, d_wp, nt, d_srp, d_sc, d_ans, B * A, rank, status=status)

        def dense():
            dc.decode_dense(h, y, apply_sigmoid=True)
            tc.decode_dense(d_feat, ts, apply_sigmoid=True)
            dc.check(dc.lib.dae_mix_scores(dc.h, P(ts), int(ts.stride(0)), P(y), int(y.stride(0)), P(d_wt), P(d_wp), B, V))
            y.index_put_((seed_rows, seed_cols), neg_inf)
            yt = y[:, :nt]
            mine = torch.gather(yt, 1, d_cols64)
            srt = torch.sort(-yt, dim=1).values                # ascending of -y = scores descending
            r = torch.searchsorted(srt, -mine)                 # how many scores are strictly larger
            return torch.where(torch.isneginf(mine), torch.full_like(r, -1), r)

        def term():
            dc.decode_mix_term(h, d_wp, nt, termT)

        def cands():
            tc.mix_candidates(dc, h, d_Wd, d_bd, d_feat, d_Wt, d_bt, d_wt, d_wp, d_ans, B * A, ya)

        fused(); want = dense(); term(); cands()                # (also the warm-up of every route)
        got = rank.view(B, A).to(torch.int64)
        differ = int((got != want).sum().item())
        # a tie can only ADD the tied smaller columns to the canonical rank: anything else would be an error of one route
        unexplained = int((((got < 0) != (want < 0)) | (got < want)).sum().item())
        plan = _lib.rank_of_plan(B, F, B * A)
        passes = -(-A // plan["capacity"])
        t_f, t_d, t_t, t_c = [], [], [], []
        for _ in range(a.runs):
            t_f.append(timed(fused, a.iters))
            t_d.append(timed(dense, a.iters))
            t_t.append(timed(term, a.iters))
            t_c.append(timed(cands, a.iters))
        mf, md, mt, mc = (float(np.median(t)) for t in (t_f, t_d, t_t, t_c))
        spread = max(max(t_f) - min(t_f), max(t_d) - min(t_d))
        case = {"answers_per_row": A, "answers_that_differ": differ, "differences_no_tie_explains": unexplained,
                "fused_ms": t_f, "dense_ms": t_d, "term_ms": t_t, "candidates_ms": t_c,
                "fused_median_ms": mf, "dense_median_ms": md, "term_median_ms": mt, "candidates_median_ms": mc,
                "fused_ahead_in_every_pair": all(x < y_ for x, y_ in zip(t_f, t_d)),
                "medians_apart_by_3_spreads": bool(abs(md - mf) >= 3 * spread), "rows_per_group": plan["rows"],
                "answers_per_pass": plan["capacity"], "passes": passes}
        res["cases"].append(case)
        print("titled %3d answers/row: fused %8.3f ms (%s)  dense x 2 + mix + mask + sort + searchsorted %8.3f ms (%s)  ratio %.2fx  "
              "every pair ahead: %s  3 x spread: %s  %d-row groups, %d answers/pass, %d pass(es)  term %.3f ms  candidates %.3f ms  "
              "%d of %d answers differ (%d not by ties)"
              % (A, mf, " ".join("%.3f" % x for x in t_f), md, " ".join("%.3f" % x for x in t_d), md / mf,
                 case["fused_ahead_in_every_pair"], case["medians_apart_by_3_spreads"], plan["rows"], plan["capacity"], passes, mt, mc,
                 differ, B * A, unexplained))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    tc.close()
    dc.close()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=140000)
    ap.add_argument("--artists", type=int, default=30000)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--answers", type=int, nargs="*", default=[10, 100, 250])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--titled", action="store_true", help="the ranks under the title mix (dae_mix_rank_of)")
    ap.add_argument("--ld-feat", type=int, default=448, help="--titled: width of the title feature rows")
    a = ap.parse_args()
    if a.titled:
        return titled(a)
    nt, na, H, B = a.tracks, a.artists, a.hidden, a.rows
    V = nt + na
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=0, bias="zipf", n_tracks=nt)
    pos, ones, seeds = make_playlists(B, nt, na, seed=1)
    rp, col, val = coo_to_csr(pos, ones, B, V)
    srp, sc = seeds_to_csr(seeds, B, nt)

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_rp, d_col, d_val, d_srp, d_sc = dev(rp), dev(col), dev(val), dev(srp), dev(sc)
    d_We, d_be, d_Wd = dev(W_enc), dev(b_enc), dev(W_dec)
    seed_rows = dev(np.repeat(np.arange(B, dtype=np.int64), np.diff(srp)))
    seed_cols = dev(sc.astype(np.int64))
    ctx = _lib.Context(0)
    h = torch.empty((B, H), device="cuda")
    z = torch.empty((B, V), device="cuda")
    neg_inf = torch.tensor(float("-inf"), device="cuda")
    res = {"V": V, "tracks": nt, "H": H, "B": B, "iters": a.iters, "runs": a.runs, "cases": []}
    print("V = %d, tracks = %d, hidden = %d, rows = %d; ms per call (device), median of %d alternating runs of %d calls"
          % (V, nt, H, B, a.runs, a.iters))
    rng = np.random.default_rng(2)
    for model, bias in (("zipf", b_dec), ("b_dec=0", np.zeros_like(b_dec))):
        d_bd = dev(bias)
        ctx.prepack_decoder(d_Wd, d_bd, dtype=_lib.DAE_DTYPE_F32)
        for A in a.answers:
            cols = rng.integers(0, nt, (B, A))
            d_ans = (dev(np.arange(B + 1, dtype=np.int32) * A), dev(cols.reshape(-1).astype(np.int32)))
            d_cols64 = dev(cols.astype(np.int64))
            rank = torch.empty(B * A, dtype=torch.int32, device="cuda")
            status = torch.zeros(1, dtype=torch.int32, device="cuda")

            def fused():
                ctx.score_rank_of(d_rp, d_col, d_val, d_We, d_be, d_Wd, d_bd, nt, d_srp, d_sc, d_ans, B * A, rank, status=status)

            def dense():
                ctx.encode(d_rp, d_col, d_val, d_We, d_be, h)
                ctx.decode_dense(h, z, apply_sigmoid=False)
                z.index_put_((seed_rows, seed_cols), neg_inf)
                zt = z[:, :nt]
                mine = torch.gather(zt, 1, d_cols64)
                srt = torch.sort(-zt, dim=1).values                # ascending of -z = logits descending
                r = torch.searchsorted(srt, -mine)                 # how many logits are strictly larger
                return torch.where(torch.isneginf(mine), torch.full_like(r, -1), r)

            fused(); want = dense()                                 # (also the warm-up of both routes)
            got = rank.view(B, A).to(torch.int64)
            differ = int((got != want).sum().item())
            # a tie can only ADD the tied smaller columns to the canonical rank: anything else would be an error of one route
            unexplained = int((((got < 0) != (want < 0)) | (got < want)).sum().item())
            plan = _lib.rank_of_plan(B, H, B * A)
            passes = -(-A // plan["capacity"])
            t_f, t_d = [], []
            for _ in range(a.runs):
                t_f.append(timed(fused, a.iters))
                t_d.append(timed(dense, a.iters))
            mf, md = float(np.median(t_f)), float(np.median(t_d))
            spread = max(max(t_f) - min(t_f), max(t_d) - min(t_d))
            case = {"model": model, "answers_per_row": A, "answers_that_differ": differ, "differences_no_tie_explains": unexplained,
                    "fused_ms": t_f, "dense_ms": t_d,
                    "fused_median_ms": mf, "dense_median_ms": md, "fused_ahead_in_every_pair": all(x < y for x, y in zip(t_f, t_d)),
                    "medians_apart_by_3_spreads": bool(md - mf >= 3 * spread), "rows_per_group": plan["rows"],
                    "answers_per_pass": plan["capacity"], "passes": passes}
            res["cases"].append(case)
            print("%-8s %3d answers/row: fused %8.3f ms (%s)  dense + mask + sort + searchsorted %8.3f ms (%s)  ratio %.2fx  "
                  "every pair ahead: %s  3 x spread: %s  %d-row groups, %d answers/pass, %d pass(es)  %d of %d answers differ (%d not by ties)"
                  % (model, A, mf, " ".join("%.3f" % x for x in t_f), md, " ".join("%.3f" % x for x in t_d), md / mf,
                     case["fused_ahead_in_every_pair"], case["medians_apart_by_3_spreads"], plan["rows"], plan["capacity"],
                     passes, differ, B * A, unexplained))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
