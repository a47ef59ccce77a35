#!/usr/bin/env python
"""Deep top-k through the fused call against the route a caller had before it, on the same device in the same session:
V = 170 000, 140 000 tracks, hidden 256, 256 rows.

  fused   dae_score_topk(k, dtype)
  dense   dae_encode + dae_decode_dense(dtype) into [B, V] + the seeds set to -inf + torch.topk(k, sorted=True) over the track
          columns -- what `predict` + a host-side mask + torch.topk amount to; none of it is code of the deep-k selection

per (k, dtype) for k = 500, 1 024, 2 048, 4 096 and fp32 / bf16.  Everything is resident on the device (the CSR, the seed CSR, the
seeds' flat index, the outputs): the figures are device time per call, `--iters` calls between two events, the median of `--runs`
alternating runs (fused, dense, fused, dense, ...).  The two routes' index lists are compared before anything is timed (torch.topk
breaks ties in its own order, so "equal" is reported, not required).  Prints one line per case and a final JSON line; `--out FILE`
also writes the JSON there."""
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
    ap.add_argument("--ks", type=int, nargs="*", default=[500, 1024, 2048, 4096])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nt, na, H, B = a.tracks, a.artists, a.hidden, a.rows
    V = nt + na
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=0, bias="zipf", n_tracks=nt)
    pos, ones, seeds = make_playlists(B, nt, na, seed=1)
    rp, col, val = coo_to_csr(pos, ones, B, V)
    srp, sc = seeds_to_csr(seeds, B, nt)

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_rp, d_col, d_val, d_srp, d_sc = dev(rp), dev(col), dev(val), dev(srp), dev(sc)
    d_We, d_be, d_Wd, d_bd = dev(W_enc), dev(b_enc), dev(W_dec), dev(b_dec)
    seed_rows = dev(np.repeat(np.arange(B, dtype=np.int64), np.diff(srp)))
    seed_cols = dev(sc.astype(np.int64))
    ctx = _lib.Context(0)
    h = torch.empty((B, H), device="cuda")
    z = torch.empty((B, V), device="cuda")
    neg_inf = torch.tensor(float("-inf"), device="cuda")
    res = {"V": V, "tracks": nt, "H": H, "B": B, "iters": a.iters, "runs": a.runs, "cases": []}
    print("V = %d, tracks = %d, hidden = %d, rows = %d; ms per call (device), median of %d alternating runs of %d calls"
          % (V, nt, H, B, a.runs, a.iters))
    for name, dtype in (("f32", _lib.DAE_DTYPE_F32), ("bf16", _lib.DAE_DTYPE_BF16)):
        ctx.prepack_decoder(d_Wd, d_bd, dtype=dtype)
        for k in a.ks:
            s = torch.empty((B, k), device="cuda"); i = torch.empty((B, k), dtype=torch.int32, device="cuda")

            def fused():
                ctx.score_topk(d_rp, d_col, d_val, d_We, d_be, nt, d_srp, d_sc, k, s, i, out_kind=_lib.DAE_OUT_LOGIT, dtype=dtype)

            def dense():
                ctx.encode(d_rp, d_col, d_val, d_We, d_be, h)
                ctx.decode_dense(h, z, apply_sigmoid=False, dtype=dtype)
                z.index_put_((seed_rows, seed_cols), neg_inf)
                return torch.topk(z[:, :nt], k, dim=1, sorted=True)

            fused(); want = dense()                                 # (also the warm-up of both routes)
            plan = ctx.last_plan()
            same = bool(torch.equal(i.to(torch.int64), want.indices))
            t_f, t_d = [], []
            for _ in range(a.runs):
                t_f.append(timed(fused, a.iters))
                t_d.append(timed(dense, a.iters))
            mf, md = float(np.median(t_f)), float(np.median(t_d))
            case = {"dtype": name, "k": k, "lists_equal": same, "fused_ms": t_f, "dense_ms": t_d, "fused_median_ms": mf,
                    "dense_median_ms": md, "fused_ahead_in_every_pair": all(x < y for x, y in zip(t_f, t_d)), "plan": plan}
            res["cases"].append(case)
            print("%-4s k = %4d: fused %8.3f ms (%s)  dense + mask + torch.topk %8.3f ms (%s)  ratio %.2fx  every pair ahead: %s  lists %s"
                  % (name, k, mf, " ".join("%.3f" % x for x in t_f), md, " ".join("%.3f" % x for x in t_d), md / mf,
                     case["fused_ahead_in_every_pair"], "equal" if same else "differ (tie order)"))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
