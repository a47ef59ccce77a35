#!/usr/bin/env python
"""The catalogue call against the other routes to "the k best tracks among THESE n columns, the same for every row", on the same
device in the same session: V = 170 000 (140 000 tracks), hidden 256, 256 rows, k = 500, random ascending catalogues.

  catalogue   dae_score_topk_catalogue on an image gathered from the catalogue's decoder rows
  candidates  dae_score_candidates + dae_rank_candidates with the catalogue as every row's list (up to --cand-max columns)
  dense       dae_encode + dae_decode_dense into [B, V] + an additive catalogue mask + the seeds set to -inf + torch.topk
  plain       at n = all tracks: dae_score_topk on the full image -- what the translation launches and the map-back cost

Everything is resident on the device (the CSR of the feed, the seed lists, the candidate CSR, the mask): the figures are device
time per call, `--iters` calls between two events, the median of `--runs` alternating runs.  The catalogue call's lists are
compared with the candidate route's (indices) before anything is timed.  Also measured: the one-off cost of dae_catalogue_create +
dae_prepack_decoder_catalogue per n (wall clock, both calls synchronise).  `--bias zeros` runs the same with b_dec = 0: the zipf
bias of the default model lets the fp32 path skip most tiles, which is no property of every model.
Prints one line per case and a final JSON line; `--out FILE` also writes the JSON there.

`--loop`: playlists/s THROUGH THE LOOP instead -- feeds of 250 rows (host COO in, host lists out), k = 500, catalogues of `--sizes`
(default 7 500 and 35 000 columns), three routes alternating in one process, the median of `--runs` runs each:
  (a) recommend_iter(..., catalogue=h)       the pipeline in catalogue mode
  (b) recommend(..., catalogue=h) per feed    the per-batch call, the caller's thread driving each launch and fetching after it
  (c) recommend_iter over the full vocabulary
(a)'s lists are compared with (b)'s before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spotify_recsys_challenge_2018_amd import _lib                                                # noqa: E402
from spotify_recsys_challenge_2018_amd.models.DAEs import coo_to_csr, seeds_to_csr               # noqa: E402
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights        # noqa: E402

DTYPES = {"f32": _lib.DAE_DTYPE_F32, "bf16": _lib.DAE_DTYPE_BF16}


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters          # ms per call


def loop_bench(a):
    import pickle
    import tempfile
    import torch
    from spotify_recsys_challenge_2018_amd.models.DAEs import DAE, SEEDS_FROM_INPUT
    nt, na, H, k, B = a.tracks, a.artists, a.hidden, a.k, 250
    V = nt + na
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=0, bias=a.bias, n_tracks=nt)
    tmp = tempfile.mkdtemp(prefix="bench_catalogue_")
    path = os.path.join(tmp, "init.pkl")
    with open(path, "wb") as f:
        pickle.dump([W_enc, W_dec, b_enc, b_dec], f)

    class C:
        save = os.path.join(tmp, "unused"); batch = B; n_input = V; hidden = H; lr = 0.005; reg_lambda = 0.0
        n_tracks = nt; initval = path
    # one model per pipeline: a model keeps ONE at a time, alternating the loops on one model would time its re-creation
    m, m_full = DAE(C()), DAE(C())
    m.fit(); m_full.fit()
    feeds = [make_playlists(B, nt, na, seed=200 + s)[:2] + (SEEDS_FROM_INPUT, B) for s in range(16)]
    rng = np.random.default_rng(0)
    n_a, n_b, n_c = a.feeds
    res = {"loop": True, "V": V, "tracks": nt, "H": H, "rows_per_feed": B, "k": k, "bias": a.bias, "runs": a.runs, "feeds": a.feeds,
           "cases": []}
    print("loop: V = %d (%d tracks), hidden = %d, feeds of %d rows, k = %d; playlists/s, %d alternating runs" % (V, nt, H, B, k, a.runs))

    def run(gen, n):
        t0 = time.perf_counter()
        rows = 0
        for idx, _s in gen:
            rows += len(idx)
        dt = time.perf_counter() - t0
        assert rows == n * B
        return rows / dt

    for n in a.sizes or [7500, 35000]:
        h = m.catalogue(np.sort(rng.permutation(nt)[:n]).astype(np.int32))
        for name in a.dtypes:
            def route_a(nf):
                return m.recommend_iter((feeds[i % 16] for i in range(nf)), k=k, dtype=name, want_scores=False, catalogue=h)

            def route_b(nf):
                return (m.recommend(*feeds[i % 16][:3], k=k, n_rows=B, dtype=name, catalogue=h) for i in range(nf))

            def route_c(nf):
                return m_full.recommend_iter((feeds[i % 16] for i in range(nf)), k=k, dtype=name, want_scores=False)
            same = all(np.array_equal(x[0], y[0]) for x, y in zip(route_a(16), route_b(16)))
            run(route_a(max(64, n_a // 8)), max(64, n_a // 8)); run(route_b(16), 16); run(route_c(max(64, n_c // 8)), max(64, n_c // 8))
            torch.cuda.synchronize()
            ra, rb, rc = [], [], []
            for _ in range(a.runs):
                ra.append(run(route_a(n_a), n_a)); rb.append(run(route_b(n_b), n_b)); rc.append(run(route_c(n_c), n_c))
            case = {"dtype": name, "n": n, "lists_equal": same, "a_playlists_per_s": [round(x) for x in ra],
                    "b_playlists_per_s": [round(x) for x in rb], "c_playlists_per_s": [round(x) for x in rc],
                    "a_median": round(float(np.median(ra))), "b_median": round(float(np.median(rb))), "c_median": round(float(np.median(rc))),
                    "a_ahead_in_every_pair": all(x > y for x, y in zip(ra, rb)),
                    "a_over_b_median": round(float(np.median(ra) / np.median(rb)), 2)}
            res["cases"].append(case)
            print("%-4s n = %6d: (a) %9d (%s)  (b) %9d (%s)  (c) %9d (%s)  | a / b %.2f, ahead in every pair: %s | lists %s"
                  % (name, n, case["a_median"], " ".join(str(x) for x in case["a_playlists_per_s"]), case["b_median"],
                     " ".join(str(x) for x in case["b_playlists_per_s"]), case["c_median"],
                     " ".join(str(x) for x in case["c_playlists_per_s"]), case["a_over_b_median"], case["a_ahead_in_every_pair"],
                     "equal" if same else "DIFFER"), flush=True)
        h.close()
    m.close_pipelines(); m_full.close_pipelines()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(c["lists_equal"] for c in res["cases"]) else 1


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=140000)
    ap.add_argument("--artists", type=int, default=30000)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--k", type=int, default=500)
    ap.add_argument("--sizes", type=int, nargs="*", default=None, help="catalogue sizes (default: 1000 7500 35000 70000 tracks)")
    ap.add_argument("--dtypes", nargs="*", default=["f32", "bf16"])
    ap.add_argument("--bias", default="zipf", choices=["zipf", "zeros"])
    ap.add_argument("--cand-max", type=int, default=35000, help="largest catalogue the candidate route is run at")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loop", action="store_true", help="playlists/s through the streamed loop (see the module docstring)")
    ap.add_argument("--feeds", type=int, nargs=3, default=[20000, 2000, 20000], help="--loop: feeds of a timed run of (a), (b), (c)")
    a = ap.parse_args()
    if a.loop:
        return loop_bench(a)
    nt, na, H, B, k = a.tracks, a.artists, a.hidden, a.rows, a.k
    V = nt + na
    sizes = a.sizes or [1000, 7500, 35000, 70000, nt]
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=0, bias=a.bias, n_tracks=nt)
    dev = torch.device("cuda", 0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)                               # noqa: E731
    We, be, Wd, bd = t(W_enc), t(b_enc), t(W_dec), t(b_dec)
    pos, ones, seeds = make_playlists(B, nt, na, seed=1)
    rp, col, val = coo_to_csr(pos, ones, B, V)
    srp, sc = seeds_to_csr(seeds, B, nt)
    d_rp, d_col, d_val, d_srp, d_sc = t(rp), t(col), t(val), t(srp), t(sc if sc.size else np.zeros(1, np.int32))
    seed_rows = t(np.repeat(np.arange(B), np.diff(srp)).astype(np.int64))
    seed_cols = t(sc.astype(np.int64))
    full = _lib.Context(0)
    rng = np.random.default_rng(0)
    res = {"V": V, "tracks": nt, "H": H, "B": B, "k": k, "bias": a.bias, "iters": a.iters, "runs": a.runs, "cases": []}
    print("V = %d (%d tracks), hidden = %d, rows = %d, k = %d, b_dec = %s; ms per call (device), median of %d alternating runs of %d calls"
          % (V, nt, H, B, k, a.bias, a.runs, a.iters))
    score = torch.empty((B, k), dtype=torch.float32, device=dev)
    idx = torch.empty((B, k), dtype=torch.int32, device=dev)
    score2, idx2 = torch.empty_like(score), torch.empty_like(idx)
    h = torch.empty((B, H), dtype=torch.float32, device=dev)
    z = torch.empty((B, V), dtype=torch.float32, device=dev)
    neg_inf = torch.tensor(float("-inf"), device=dev)
    for name in a.dtypes:
        dtype = DTYPES[name]
        full.prepack_decoder(Wd, bd, dtype=dtype)
        for n in sizes:
            cols = np.sort(rng.permutation(nt)[:n]).astype(np.int32)
            d_cols = t(cols)
            c = _lib.Context(0)
            # the one-off cost: create + prepack (each synchronises), wall clock, the median of three
            setup = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                cat = _lib.Catalogue(c, d_cols, nt)
                c.prepack_decoder_catalogue(cat, Wd, bd, dtype=dtype)
                torch.cuda.synchronize()
                setup.append((time.perf_counter() - t0) * 1e3)
                if len(setup) < 3:
                    cat.close()
            mask = torch.full((nt,), float("-inf"), device=dev)
            mask[d_cols.to(torch.int64)] = 0.0

            def catalogue():
                c.score_topk_catalogue(cat, d_rp, d_col, d_val, We, be, d_srp, d_sc, k, score, idx, dtype=dtype)

            def dense():
                full.encode(d_rp, d_col, d_val, We, be, h)
                full.decode_dense(h, z, apply_sigmoid=False, dtype=dtype)
                zt = z[:, :nt] + mask
                zt.index_put_((seed_rows, seed_cols), neg_inf)
                return torch.topk(zt, k, dim=1)

            def plain():
                full.score_topk(d_rp, d_col, d_val, We, be, nt, d_srp, d_sc, k, score2, idx2, dtype=dtype)

            routes = [("catalogue", catalogue), ("dense", dense)]
            if n <= a.cand_max and dtype == _lib.DAE_DTYPE_F32:                  # (the candidate kernels are fp32 only)
                cand = (torch.arange(0, B * n + 1, n, dtype=torch.int32, device=dev), d_cols.repeat(B))
                key = torch.empty(B * n, dtype=torch.float32, device=dev)

                def candidates():
                    full.score_candidates(d_rp, d_col, d_val, We, be, Wd, bd, cand, B * n, key, out_kind=_lib.DAE_OUT_LOGIT)
                    full.rank_candidates(V, cand, key, n, d_srp, d_sc, k, score2, idx2)
                routes.append(("candidates", candidates))
            if n == nt:
                routes.append(("plain", plain))
            same = None
            for _label, fn in routes:
                fn()                                                             # (the warm-up of every shape)
            if len(routes) > 2:                                                  # the second route's lists are in idx2
                torch.cuda.synchronize()
                same = bool(torch.equal(idx, idx2))
            times = {label: [] for label, _fn in routes}
            for _ in range(a.runs):
                for label, fn in routes:
                    times[label].append(timed(fn, a.iters))
            case = {"dtype": name, "n": n, "setup_ms": setup, "setup_median_ms": float(np.median(setup)), "idx_equal": same}
            for label in times:
                case[label + "_ms"] = times[label]
                case[label + "_median_ms"] = float(np.median(times[label]))
            catalogue()
            case["plan"] = c.last_plan()
            if dtype == _lib.DAE_DTYPE_F32:
                c.filter_skip_read()
                catalogue()
                case["filter_skip"] = c.filter_skip_read()                       # {launches, planned, live} tiles of one call
            res["cases"].append(case)
            print("%-4s n = %6d: " % (name, n) + "  ".join("%s %7.3f ms (%s)" % (label, case[label + "_median_ms"],
                  " ".join("%.3f" % x for x in times[label])) for label in times)
                  + "  | create + prepack %.1f ms | lists %s | fused %d" % (case["setup_median_ms"],
                  {None: "-", True: "equal", False: "DIFFER"}[same], case["plan"]["fused"]))
            cat.close()
            c.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    sys.exit(main())
