#!/usr/bin/env python
"""The cost of a batch without a step through the fused call against the two routes a caller had before it, on the same device
in the same session: V = 170 000, 140 000 tracks, hidden 256; 256 and 1 024 rows; fp32 and bf16; about 100 targets a row.

  fused   dae_score_loss (row losses and the cost)
  step    dae_train_forward_backward into throw-away gradient buffers (two [V, H] tensors for the untied model), cost_out read
  dense   dae_encode + dae_decode_dense with the sigmoid into [B, V] + the weighted BCE of the reference in torch against a dense
          [B, V] target matrix (resident, built once: not timed) -- none of it is code of the fused call

Everything is resident on the device (both CSRs, the parameters, the outputs): the figures are device time per call, `--iters`
calls between two events, the median of `--runs` alternating runs (fused, step, dense, fused, ...), all values printed.  The
three routes' costs are compared before anything is timed.  Per case also dae_decode_loss_rows alone on resident hidden rows
with empty target rows (the pack, the GEMM launch with the row-loss epilogue, the finishing launch) and, from it, 2 B V H flops
per call against the fp32 / bf16 matrix peak (157.3 / 2 516 TFLOP/s).  Prints one line per case and a final JSON line; `--out
FILE` also writes the JSON there."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spotify_recsys_challenge_2018_amd import _lib                                                # noqa: E402
from spotify_recsys_challenge_2018_amd.models.DAEs import coo_to_csr                              # noqa: E402
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights        # noqa: E402

PEAK_TFLOPS = {_lib.DAE_DTYPE_F32: 157.3, _lib.DAE_DTYPE_BF16: 2516.0}
SEED = 7


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
    ap.add_argument("--rows", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nt, na, H = a.tracks, a.artists, a.hidden
    V = nt + na
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=0, bias="zipf", n_tracks=nt)

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_We, d_be, d_Wd, d_bd = dev(W_enc), dev(b_enc), dev(W_dec), dev(b_dec)
    gWe, gWd = torch.zeros((V, H), device="cuda"), torch.zeros((V, H), device="cuda")
    gbe, gbd = torch.zeros(H, device="cuda"), torch.zeros(V, device="cuda")
    P = _lib._ptr
    ctx = _lib.Context(0)
    res = {"V": V, "tracks": nt, "H": H, "iters": a.iters, "runs": a.runs, "cases": []}
    print("V = %d, tracks = %d, hidden = %d; ms per call (device), median of %d alternating runs of %d calls" % (V, nt, H, a.runs, a.iters))
    for B in a.rows:
        pos, ones, _seeds = make_playlists(B, nt, na, seed=1, seed_counts=(50,))
        xm = pos[:, 1] < nt
        x = [dev(t) for t in coo_to_csr(pos[xm], ones[xm], B, V)]
        y_host = coo_to_csr(pos, np.ones(len(pos), np.float32), B, V)
        n_tgt = float(y_host[0][-1]) / B
        y = [dev(t) for t in y_host]
        y_empty = [torch.zeros(B + 1, dtype=torch.int32, device="cuda"), y[1], y[2]]
        y_dense = torch.zeros((B, V), device="cuda")
        y_dense[dev(pos[:, 0]), dev(pos[:, 1])] = 1.0
        h = torch.empty((B, H), device="cuda")
        p = torch.empty((B, V), device="cuda")
        rows, cost, cost_s = torch.empty(B, device="cuda"), torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
        for dtype, name in ((_lib.DAE_DTYPE_F32, "fp32"), (_lib.DAE_DTYPE_BF16, "bf16")):
            ctx.set_train_dtype(dtype)
            ctx.prepack_decoder(d_Wd, d_bd, dtype=dtype)

            def fused():
                ctx.score_loss(x, y, d_We, d_be, d_Wd, d_bd, B, False, seed=SEED, row_loss=rows, cost_out=cost)

            def step():
                ctx.check(ctx.lib.dae_train_forward_backward(
                    ctx.h, P(x[0]), P(x[1]), P(x[2]), P(y[0]), P(y[1]), P(y[2]), P(d_We), P(d_be), P(d_Wd), P(d_bd), V, H, B, B, 0,
                    1.0, 1.0, SEED, 0.0, P(gWe), P(gbe), P(gWd), P(gbd), P(cost_s)))

            def dense():
                ctx.encode(x[0], x[1], x[2], d_We, d_be, h)
                ctx.decode_dense(h, p, apply_sigmoid=True, dtype=dtype)
                L = -(y_dense * torch.log(p + 1e-10) + 0.55 * (1.0 - y_dense) * torch.log(1.0 - p + 1e-10)).sum(dim=1)
                return L.sum() / B

            def gemm():
                ctx.decode_loss_rows(h, y_empty, d_Wd, d_bd, rows, dtype=dtype)

            step(); c_dense = float(dense().item())                 # (also the warm-up of every route; the step re-tiles its own image)
            ctx.prepack_decoder(d_Wd, d_bd, dtype=dtype)
            fused(); gemm(); fused()
            c_fused, c_step = float(cost.item()), float(cost_s.item())
            t_f, t_s, t_d, t_g = [], [], [], []
            for _ in range(a.runs):
                t_f.append(timed(fused, a.iters))
                t_s.append(timed(step, a.iters))
                ctx.prepack_decoder(d_Wd, d_bd, dtype=dtype)        # (the step's re-tiling left an image without bounds: the same weights again)
                t_d.append(timed(dense, a.iters))
                t_g.append(timed(gemm, a.iters))
            mf, ms, md, mg = (float(np.median(t)) for t in (t_f, t_s, t_d, t_g))
            share = 2.0 * B * V * H / (mg * 1e-3) / 1e12 / PEAK_TFLOPS[dtype]
            case = {"rows": B, "dtype": name, "targets_per_row": n_tgt, "cost_fused": c_fused, "cost_step": c_step, "cost_dense": c_dense,
                    "fused_ms": t_f, "step_ms": t_s, "dense_ms": t_d, "rows_call_ms": t_g,
                    "fused_median_ms": mf, "step_median_ms": ms, "dense_median_ms": md, "rows_call_median_ms": mg,
                    "fused_ahead_of_step_in_every_pair": all(f < s for f, s in zip(t_f, t_s)),
                    "fused_ahead_of_dense_in_every_pair": all(f < d for f, d in zip(t_f, t_d)),
                    "spread_ms": {"fused": max(t_f) - min(t_f), "step": max(t_s) - min(t_s), "dense": max(t_d) - min(t_d)},
                    "rows_call_share_of_matrix_peak": share}
            res["cases"].append(case)
            print("%4d rows %s (%.0f targets/row): fused %7.3f ms (%s)  step %7.3f ms (%s)  dense + BCE %7.3f ms (%s)  ahead of step in "
                  "every pair: %s  of dense: %s  rows call alone %7.3f ms = %.1f%% of the %s matrix peak  costs %.6f / %.6f / %.6f"
                  % (B, name, n_tgt, mf, " ".join("%.3f" % t for t in t_f), ms, " ".join("%.3f" % t for t in t_s), md,
                     " ".join("%.3f" % t for t in t_d), case["fused_ahead_of_step_in_every_pair"],
                     case["fused_ahead_of_dense_in_every_pair"], mg, 100.0 * share, name, c_fused, c_step, c_dense))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
