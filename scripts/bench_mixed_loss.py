#!/usr/bin/env python
"""The loss of the title mix without a step through the fused call against the two routes a caller had before it, on the same
device in the same session: V = 170 000, DAE hidden 256, ld_feat 448, 88 targets a row; 150, 256 and 1 024 rows (four panels).

  fused   dae_mix_loss_rows (row losses and the cost)
  step    dae_decode_dense on both contexts into two [B, V] matrices + dae_title_loss_backward into throw-away gradients, its
          cost read (the loss half of the title step; at most 256 rows a call, so 1 024 rows are four calls over row slices)
  dense   dae_decode_dense on both contexts + dae_mix_scores + the weighted BCE of the reference in torch against a dense [B, V]
          target matrix (resident, built once: not timed) -- none of it is code of the fused call

Everything is resident on the device (hidden rows, feature rows, weights, the target CSR, the outputs): the figures are device
time per call, `--iters` calls between two events, the median of `--runs` alternating runs (fused, step, dense, fused, ...), all
values printed.  The three routes' costs are compared before anything is timed.  Per case also the pieces of the fused call that
can run alone: dae_decode_mix_term over all V columns (the DAE's GEMM, transposed stores) and the title context's plain dense
decode (the same GEMM as the loss launch, with a store instead of the loss epilogue), each over the whole batch; what the fused
call takes beyond the term launch is its title GEMM with the loss epilogue plus the finishing launches.  Prints one line per case
and a final JSON line; `--out FILE` also writes the JSON there."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spotify_recsys_challenge_2018_amd import _lib                                                # noqa: E402
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_weights                        # noqa: E402


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
    ap.add_argument("--columns", type=int, default=170000)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--ld-feat", type=int, default=448)
    ap.add_argument("--targets", type=int, default=88)
    ap.add_argument("--rows", type=int, nargs="*", default=[150, 256, 1024])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    V, H, Fd, nt = a.columns, a.hidden, a.ld_feat, a.targets
    rng = np.random.default_rng(0)
    _W_enc, _b_enc, W_dec, b_dec = make_weights(V, H, seed=0, bias="zipf", n_tracks=V)
    OutW_T = (rng.standard_normal((V, Fd)) * 0.05).astype(np.float32)
    Out_b = (rng.standard_normal(V) - 4.0).astype(np.float32)

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()
    Wd, bd, Wt, bt = dev(W_dec), dev(b_dec), dev(OutW_T), dev(Out_b)
    gW, gb = torch.zeros((V, Fd), device="cuda"), torch.zeros(V, device="cuda")
    P = _lib._ptr
    tc, dc = _lib.Context(0), _lib.Context(0)
    dc.prepack_decoder(Wd, bd, dtype=_lib.DAE_DTYPE_F32)
    tc.prepack_decoder(Wt, bt, dtype=_lib.DAE_DTYPE_F32)
    res = {"V": V, "H": H, "ld_feat": Fd, "targets_per_row": nt, "iters": a.iters, "runs": a.runs, "cases": []}
    print("V = %d, hidden = %d, ld_feat = %d, %d targets a row; ms per call (device), median of %d alternating runs of %d calls"
          % (V, H, Fd, nt, a.runs, a.iters))
    for B in a.rows:
        h = dev(rng.uniform(0.0, 1.0, (B, H)).astype(np.float32))
        feat = dev(np.abs(rng.standard_normal((B, Fd)) * 0.5).astype(np.float32))
        x = rng.integers(1, 60, B).astype(np.float32)
        w_t, w_p = dev((1.0 / (1.0 + x)).astype(np.float32)), dev((x / (1.0 + x)).astype(np.float32))
        cols = np.stack([np.sort(rng.choice(V, nt, replace=False)) for _ in range(B)]).astype(np.int32)
        rp = (np.arange(B + 1) * nt).astype(np.int32)
        y = (dev(rp), dev(cols.reshape(-1)), torch.ones(B * nt, device="cuda"))
        y_dense = torch.zeros((B, V), device="cuda")
        y_dense[dev(np.repeat(np.arange(B), nt)), dev(cols.reshape(-1).astype(np.int64))] = 1.0
        z, dae, termT = torch.empty((B, V), device="cuda"), torch.empty((B, V), device="cuda"), torch.empty((V, B), device="cuda")
        slabs = [(r0, min(256, B - r0)) for r0 in range(0, B, 256)]
        rows, cost, cost_s = torch.empty(B, device="cuda"), torch.empty(1, device="cuda"), torch.empty(len(slabs), device="cuda")
        dfeat = torch.empty((B, Fd), device="cuda")
        y_slab = [(dev((rp[r0:r0 + nb + 1] - rp[r0]).astype(np.int32)), y[1][int(rp[r0]):], y[2][int(rp[r0]):]) for r0, nb in slabs]

        def fused():
            tc.mix_loss_rows(dc, h, Wd, bd, feat, Wt, bt, w_t, w_p, B, y, row_loss=rows, cost_out=cost)

        def step():
            dc.decode_dense(h, dae, apply_sigmoid=True)
            tc.decode_dense(feat, z, apply_sigmoid=False)
            for i, (r0, nb) in enumerate(slabs):
                ys = y_slab[i]
                tc.check(tc.lib.dae_title_loss_backward(
                    tc.h, P(z[r0:]), V, P(dae[r0:]), V, P(ys[0]), P(ys[1]), P(ys[2]), P(w_t[r0:]), P(w_p[r0:]), nb, V, B,
                    P(feat[r0:]), Fd, P(Wt), P(gW), P(gb), P(dfeat[r0:]), P(cost_s[i:])))
            return cost_s[:len(slabs)].sum()

        def dense():
            dc.decode_dense(h, dae, apply_sigmoid=True)
            tc.decode_dense(feat, z, apply_sigmoid=True)
            dc.check(dc.lib.dae_mix_scores(dc.h, P(z), V, P(dae), V, P(w_t), P(w_p), B, V))        # dae <- the mixed score
            L = -(y_dense * torch.log(dae + 1e-10) + 0.55 * (1.0 - y_dense) * torch.log(1.0 - dae + 1e-10)).sum(dim=1)
            return L.sum() / B

        def term():
            dc.check(dc.lib.dae_decode_mix_term(dc.h, P(h), B, H, _lib.DAE_DTYPE_F32, P(w_p), V, P(termT), B))

        def title_gemm():
            tc.decode_dense(feat, z, apply_sigmoid=False)

        c_step, c_dense = float(step().item()), float(dense().item())         # (also the warm-up of every route)
        fused(); term(); title_gemm(); fused()
        c_fused = float(cost.item())
        t_f, t_s, t_d, t_t, t_g = [], [], [], [], []
        for _ in range(a.runs):
            t_f.append(timed(fused, a.iters))
            t_s.append(timed(step, a.iters))
            t_d.append(timed(dense, a.iters))
            t_t.append(timed(term, a.iters))
            t_g.append(timed(title_gemm, a.iters))
        mf, ms, md, mt, mg = (float(np.median(t)) for t in (t_f, t_s, t_d, t_t, t_g))
        spread = {"fused": max(t_f) - min(t_f), "step": max(t_s) - min(t_s), "dense": max(t_d) - min(t_d)}
        case = {"rows": B, "cost_fused": c_fused, "cost_step": c_step, "cost_dense": c_dense,
                "fused_ms": t_f, "step_ms": t_s, "dense_ms": t_d, "term_ms": t_t, "title_dense_decode_ms": t_g,
                "fused_median_ms": mf, "step_median_ms": ms, "dense_median_ms": md, "term_median_ms": mt,
                "title_dense_decode_median_ms": mg,
                "fused_ahead_of_step_in_every_pair": all(f < s for f, s in zip(t_f, t_s)),
                "fused_ahead_of_dense_in_every_pair": all(f < d for f, d in zip(t_f, t_d)),
                "spread_ms": spread,
                "apart_by_3_spreads_from_step": abs(ms - mf) >= 3.0 * max(spread["fused"], spread["step"]),
                "apart_by_3_spreads_from_dense": abs(md - mf) >= 3.0 * max(spread["fused"], spread["dense"])}
        res["cases"].append(case)
        print("%4d rows: fused %7.3f ms (%s)  step %7.3f ms (%s)  dense + BCE %7.3f ms (%s)  ahead of step in every pair: %s  of dense: "
              "%s  3 spreads apart: %s / %s  term alone %7.3f ms  title dense decode alone %7.3f ms  costs %.6f / %.6f / %.6f"
              % (B, mf, " ".join("%.3f" % t for t in t_f), ms, " ".join("%.3f" % t for t in t_s), md, " ".join("%.3f" % t for t in t_d),
                 case["fused_ahead_of_step_in_every_pair"], case["fused_ahead_of_dense_in_every_pair"],
                 case["apart_by_3_spreads_from_step"], case["apart_by_3_spreads_from_dense"], mt, mg, c_fused, c_step, c_dense))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    tc.close()
    dc.close()


if __name__ == "__main__":
    main()
