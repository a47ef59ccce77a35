#!/usr/bin/env python
"""An ensemble's ranking through the fused call against the route a caller had before it, on the same device in the same session:
V = 170 000, 140 000 tracks, hidden 256, 256 rows, k = 500, M = 2, 3, 4 members, fp32 and bf16, untitled and titled.

  fused   per member dae_encode, then dae_ensemble_topk (dae_decode_mix_term for member 0, dae_decode_mix_term_add for the others
          that go into the sum, dae_set_score_mix + dae_decode_topk on the ranking context)
  dense   per member dae_encode + dae_decode_dense with the sigmoid into a [B, V] matrix, the weighted sum of the track columns
          with torch operations in the canonical order (titled: + dae_decode_dense on the title context), the seeds set to -inf,
          torch.topk(k, sorted=True) -- none of it is code of the ensemble

Everything is resident on the device (the CSR, the seed CSR, the seeds' flat index, the weights a_m, titled: the feature rows and
w_title, the outputs): the figures are device time per call, `--iters` calls between two events, the median of `--runs`
alternating runs (fused, dense, term, fused, ...), all values printed.  The two routes' lists are compared before anything is
timed; torch.topk knows no column order among tied scores, so "rows whose lists differ" is reported, not required to be 0.
Per case the term launches (dae_decode_mix_term + the dae_decode_mix_term_add calls) are also timed alone: their share of the
fused call is what a single launch decoding all members per tile could save at most.  Prints one line per case and a final JSON
line; `--out FILE` also writes the JSON there."""
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


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=140000)
    ap.add_argument("--artists", type=int, default=30000)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--k", type=int, default=500)
    ap.add_argument("--members", type=int, nargs="*", default=[2, 3, 4])
    ap.add_argument("--dtypes", nargs="*", default=["f32", "bf16"], choices=["f32", "bf16"])
    ap.add_argument("--ld-feat", type=int, default=448, help="width of the title feature rows of the titled cases")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nt, na, H, B, k, F = a.tracks, a.artists, a.hidden, a.rows, a.k, a.ld_feat
    V = nt + na
    M_max = max(a.members)

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()
    pos, ones, seeds = make_playlists(B, nt, na, seed=1)
    rp, col, val = coo_to_csr(pos, ones, B, V)
    srp, sc = seeds_to_csr(seeds, B, nt)
    d_rp, d_col, d_val, d_srp, d_sc = dev(rp), dev(col), dev(val), dev(srp), dev(sc)
    seed_rows = dev(np.repeat(np.arange(B, dtype=np.int64), np.diff(srp)))
    seed_cols = dev(sc.astype(np.int64))
    rng = np.random.default_rng(2)
    W = [make_weights(V, H, seed=10 + m, bias="zipf", n_tracks=nt) for m in range(M_max)]
    d_W = [tuple(dev(x) for x in w) for w in W]                       # (W_enc, b_enc, W_dec, b_dec)
    OutW_T = dev((rng.standard_normal((V, F)) * 0.05).astype(np.float32))
    Out_b = dev((W[0][3] + rng.standard_normal(V).astype(np.float32)).astype(np.float32))
    d_feat = dev((np.abs(rng.standard_normal((B, F))) * 0.5).astype(np.float32))
    x_count = np.bincount(np.repeat(np.arange(B), np.diff(rp)), weights=val.astype(np.float64), minlength=B).astype(np.float32)
    deno = np.float32(1.0) + x_count + np.float32(1e-10)              # titles_use = 1 on every row
    w_t, w_p = (np.float32(1.0) / deno).astype(np.float32), (x_count / deno).astype(np.float32)
    d_wt = dev(w_t)
    ctxs = [_lib.Context(0) for _ in range(M_max)]
    tc = _lib.Context(0)
    hs = [torch.empty((B, H), device="cuda") for _ in range(M_max)]
    dense_m = torch.empty((B, V), device="cuda")
    neg_inf = torch.tensor(float("-inf"), device="cuda")
    nt32 = min((nt + 31) // 32 * 32, V)
    termT = torch.empty((nt32, B), device="cuda")
    score = torch.empty((B, k), dtype=torch.float32, device="cuda")
    idx = torch.empty((B, k), dtype=torch.int32, device="cuda")
    res = {"V": V, "tracks": nt, "H": H, "B": B, "k": k, "ld_feat": F, "iters": a.iters, "runs": a.runs, "cases": []}
    print("V = %d, tracks = %d, hidden = %d, rows = %d, k = %d; ms per call (device), median of %d alternating runs of %d calls"
          % (V, nt, H, B, k, a.runs, a.iters))
    for dname in a.dtypes:
        dtype = _lib.DAE_DTYPE_F32 if dname == "f32" else _lib.DAE_DTYPE_BF16
        for m in range(M_max):
            ctxs[m].prepack_decoder(d_W[m][2], d_W[m][3], dtype=dtype)
        tc.prepack_decoder(OutW_T, Out_b, dtype=dtype)
        for is_titled in (False, True):
            for M in a.members:
                alpha = [np.full(B, np.float32(1.0) / np.float32(M), np.float32) for _ in range(M)]
                d_a = [dev(x * w_p if is_titled else x) for x in alpha]
                n_acc = M if is_titled else M - 1
                ranker = tc if is_titled else ctxs[M - 1]
                kw = dict(feat=d_feat, w_title=d_wt) if is_titled else {}

                def encode():
                    for m in range(M):
                        ctxs[m].encode(d_rp, d_col, d_val, d_W[m][0], d_W[m][1], hs[m])

                def fused():
                    encode()
                    ranker.ensemble_topk(ctxs[:M], hs[:M], d_a, nt, d_srp, d_sc, k, score, idx, dtype=dtype, **kw)

                def term():
                    for m in range(n_acc):
                        (ctxs[m].decode_mix_term_add if m else ctxs[m].decode_mix_term)(hs[m], d_a[m], nt, termT, dtype=dtype)

                def dense():
                    encode()
                    acc = None
                    for m in range(M):
                        ctxs[m].decode_dense(hs[m], dense_m, apply_sigmoid=True, dtype=dtype)
                        t = dense_m[:, :nt] * d_a[m][:, None]
                        if m == M - 1 and not is_titled:
                            acc = t if acc is None else t + acc
                        else:
                            acc = t if acc is None else acc + t
                    if is_titled:
                        tc.decode_dense(d_feat, dense_m, apply_sigmoid=True, dtype=dtype)
                        acc = dense_m[:, :nt] * d_wt[:, None] + acc
                    acc.index_put_((seed_rows, seed_cols), neg_inf)
                    return torch.topk(acc, k, dim=1, sorted=True)

                fused(); want = dense(); term()                     # (also the warm-up of every route)
                rows_differ = int((idx.to(torch.int64) != want.indices).any(dim=1).sum().item())
                scores_differ = int((score != want.values).any(dim=1).sum().item())
                t_f, t_d, t_t = [], [], []
                for _ in range(a.runs):
                    t_f.append(timed(fused, a.iters))
                    t_d.append(timed(dense, a.iters))
                    t_t.append(timed(term, a.iters))
                mf, md, mt = (float(np.median(t)) for t in (t_f, t_d, t_t))
                spread = max(max(t_f) - min(t_f), max(t_d) - min(t_d))
                case = {"dtype": dname, "titled": is_titled, "members": M, "fused_ms": t_f, "dense_ms": t_d, "term_ms": t_t,
                        "fused_median_ms": mf, "dense_median_ms": md, "term_median_ms": mt, "term_share_of_fused": mt / mf,
                        "ahead": "fused" if mf < md else "dense", "fused_ahead_in_every_pair": all(x < y for x, y in zip(t_f, t_d)),
                        "medians_apart_by_3_spreads": bool(abs(md - mf) >= 3 * spread), "rows_whose_lists_differ": rows_differ,
                        "rows_whose_scores_differ": scores_differ}
                res["cases"].append(case)
                print("%-4s %-8s M = %d: fused %7.3f ms (%s)  dense %7.3f ms (%s)  ratio %.2fx  ahead: %s  3 x spread: %s  "
                      "term launches %.3f ms = %.0f %% of fused  lists of %d / %d rows differ (scores: %d)"
                      % (dname, "titled" if is_titled else "untitled", M, mf, " ".join("%.3f" % x for x in t_f), md,
                         " ".join("%.3f" % x for x in t_d), md / mf, case["ahead"], case["medians_apart_by_3_spreads"], mt,
                         100.0 * mt / mf, rows_differ, B, scores_differ))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for c in ctxs + [tc]:
        c.close()


if __name__ == "__main__":
    main()
