#!/usr/bin/env python
"""Candidate scoring against the dense route, on the same device in the same session: V = 170 000, hidden 256, 256 rows,
C uniformly random candidate columns per row.

  plain   dae_decode_candidates                  vs  dae_decode_dense into [B, V] + torch.gather
  titled  dae_mix_candidates                     vs  what `mixed_scores` runs (dae_decode_dense on both contexts +
                                                     dae_mix_scores) + torch.gather

Everything is resident on the device (hidden rows, title features, mixing weights, the candidate CSR, the gather index):
the figures are device time per call, `--iters` calls between two events, the median of `--runs` alternating runs (new, dense,
new, dense, ...).  Both routes' values are compared bit for bit before anything is timed.  Prints one line per C and a final
JSON line; `--out FILE` also writes the JSON there.

`--loop`: the STREAMED candidate calls against the per-batch calls, host lists in and host results out, in one process: `--feeds`
feeds of `--rows` (250) rows, C = 100 / 1 000 / 5 000 uniformly random candidates per row as 2-D int32 arrays, plain (DAE) and
titled (DAE_title, every title in use); (a) `score_candidates_iter` against (b) `score_candidates` per feed, and the same pair
for `rank_candidates` at k = 500.  Playlists/s over the wall clock of a whole pass, `--runs` alternating passes (a, b, a, b, ...),
medians; the verdict per case is the project's bar -- every alternating pair ahead AND the medians apart by three times the larger
spread (max - min) within a set.  For (a) it also prints `dae_pipeline_times` per pass (ms: the library thread issuing / idle,
the caller inside submit / waiting in poll), which says whose thread bounds the loop."""
import argparse
import json
import os
import pickle
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spotify_recsys_challenge_2018_amd import _lib                                                # noqa: E402
from spotify_recsys_challenge_2018_amd.models.DAEs import DAE_title                               # noqa: E402
from spotify_recsys_challenge_2018_amd.models.title_models import get_model                       # noqa: E402
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


def loop_main(a):
    """--loop (see the module's docstring)."""
    import time
    import torch
    from spotify_recsys_challenge_2018_amd.models.DAEs import DAE, SEEDS_FROM_INPUT
    nt, na, H, B = a.tracks, a.artists, a.hidden, a.rows
    V = nt + na
    Cs = a.cands or [100, 1000, 5000]
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=0, bias="zipf", n_tracks=nt)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "dae.pkl")
    with open(path, "wb") as f:
        pickle.dump([W_enc, W_dec, b_enc, b_dec], f)

    class C_:
        batch = B; n_input = V; n_output = V; n_tracks = nt; hidden = H; lr = 0.001; reg_lambda = 0.0
        char_emb = 50; strmaxlen = 25; charsize = 41; char_model = 'Char_CNN'; filter_num = 100
        filter_size = [3, 5, 7, 9]; save = os.path.join(tmp, "unused"); initval = "NULL"; DAEval = path; title_lr = 0.001
    mt = get_model(C_()); mt.fit()
    titled = DAE_title(C_(), mt); titled.fit()
    plain = DAE(C_())
    plain._host_init = lambda: [W_enc, W_dec, b_enc, b_dec]
    plain.fit()
    rng = np.random.default_rng(0)
    base = []
    for i in range(a.feeds):
        pos, ones, _seeds = make_playlists(B, nt, na, seed=1 + i)
        titles = rng.integers(0, 41, (B, 25)); titles[:, 18:] = -1
        base.append((pos, ones, SEEDS_FROM_INPUT, B, titles, np.ones(B, np.float32)))
    res = {"V": V, "H": H, "rows": B, "feeds": a.feeds, "runs": a.runs, "title_ld": int(mt.ld), "cases": []}
    print("V = %d, hidden = %d, title rows of %d, %d feeds of %d rows; playlists/s over a pass, %d alternating passes"
          % (V, H, mt.ld, a.feeds, B, a.runs))

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = fn()
        torch.cuda.synchronize()
        return n * B / (time.perf_counter() - t0)

    for C in Cs:
        cands = [rng.integers(0, V, (B, C)).astype(np.int32) for _ in range(a.feeds)]
        for label, m in (("plain", plain), ("titled", titled)):
            feeds = [(f if label == "titled" else f[:4], c) for f, c in zip(base, cands)]
            kw = (lambda f: dict(titles=f[4], titles_use=f[5])) if label == "titled" else (lambda f: {})
            routes = {
                "score": (lambda: sum(1 for _r in m.score_candidates_iter(iter(feeds))),
                          lambda: sum(1 for f, c in feeds if m.score_candidates(f[0], f[1], c, **kw(f)) is not None)),
                "rank": (lambda: sum(1 for _r in m.rank_candidates_iter(iter(feeds), k=a.k)),
                         lambda: sum(1 for f, c in feeds
                                     if m.rank_candidates(f[0], f[1], c, SEEDS_FROM_INPUT, k=a.k, **kw(f)) is not None)),
            }
            for what, (stream, per_batch) in routes.items():
                stream(); per_batch()                                   # warm-up of both routes (the pipeline is created here)
                t_a, t_b, times = [], [], []
                for _ in range(a.runs):
                    pipe = next(iter(m._pipes.values()))[1]
                    before = pipe.times()
                    t_a.append(wall(stream))
                    after = pipe.times() if pipe.h is not None else before
                    times.append({k_: round(after[k_] - before[k_], 2) for k_ in after})
                    t_b.append(wall(per_batch))
                ma, mb = float(np.median(t_a)), float(np.median(t_b))
                spread = max(max(t_a) - min(t_a), max(t_b) - min(t_b))
                pairs = all(x > y for x, y in zip(t_a, t_b))
                case = {"model": label, "call": what, "C": C, "stream_pl_s": t_a, "per_batch_pl_s": t_b, "stream_median": ma,
                        "per_batch_median": mb, "ratio": ma / mb, "ahead_in_every_pair": pairs,
                        "medians_apart_3_spreads": bool(ma - mb > 3 * spread), "meets_bar": bool(pairs and ma - mb > 3 * spread),
                        "pipeline_times_ms": times}
                res["cases"].append(case)
                print("%-6s %-5s C = %5d: stream %9.0f pl/s (%s)  per batch %9.0f pl/s (%s)  ratio %.2fx  bar %s  pipeline ms %s"
                      % (label, what, C, ma, " ".join("%.0f" % x for x in t_a), mb, " ".join("%.0f" % x for x in t_b), ma / mb,
                         "met" if case["meets_bar"] else "MISSED", times[-1]), flush=True)
            m.close_pipelines()
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
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--cands", type=int, nargs="*", default=None, help="candidates per row (default: 100 1000 10000 tracks/4)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loop", action="store_true", help="the streamed candidate calls against the per-batch calls (host in, host out)")
    ap.add_argument("--feeds", type=int, default=24, help="--loop: feeds per pass")
    ap.add_argument("--k", type=int, default=500, help="--loop: k of the rank_candidates pair")
    a = ap.parse_args()
    if a.loop:
        if a.rows == 256:
            a.rows = 250
        return loop_main(a)
    nt, na, H, B = a.tracks, a.artists, a.hidden, a.rows
    V = nt + na
    Cs = a.cands or [100, 1000, 10000, nt // 4]
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=0, bias="zipf", n_tracks=nt)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "dae.pkl")
    with open(path, "wb") as f:
        pickle.dump([W_enc, W_dec, b_enc, b_dec], f)

    class C_:
        batch = B; n_input = V; n_output = V; n_tracks = nt; hidden = H; lr = 0.001; reg_lambda = 0.0
        char_emb = 50; strmaxlen = 25; charsize = 41; char_model = 'Char_CNN'; filter_num = 100
        filter_size = [3, 5, 7, 9]; save = os.path.join(tmp, "unused"); initval = "NULL"; DAEval = path; title_lr = 0.001
    mt = get_model(C_()); mt.fit()
    m = DAE_title(C_(), mt); m.fit()
    pos, ones, _seeds = make_playlists(B, nt, na, seed=1)
    rng = np.random.default_rng(0)
    titles = rng.integers(0, 41, (B, 25)); titles[:, 18:] = -1
    use = np.ones(B, np.float32)
    dev = m.weights["encoder_h"].device

    # the resident inputs of both routes
    m._ensure_packed(); mt._ensure_packed()
    m.ctx.bind_stream(); mt.ctx.bind_stream()
    csr = m._upload_csr(pos, ones)
    h = torch.empty((B, H), dtype=torch.float32, device=dev)
    m.ctx.encode(csr[0], csr[1], csr[2], m.weights["encoder_h"], m.biases["encoder_b"], h)
    w_t, w_p = m._mix_weights(csr, use)
    feat = mt.features(titles, B)
    Wd, bd, WT, bT = m.weights["decoder_h"], m.biases["decoder_b"], mt.p["Output_WT"], mt.p["Output_b"]
    y = torch.empty((B, V), dtype=torch.float32, device=dev)
    ts = torch.empty((B, V), dtype=torch.float32, device=dev)
    P = _lib._ptr
    res = {"V": V, "H": H, "B": B, "iters": a.iters, "runs": a.runs, "cases": []}
    print("V = %d, hidden = %d, rows = %d; ms per call (device), median of %d alternating runs of %d calls" % (V, H, B, a.runs, a.iters))
    for C in Cs:
        cols = torch.from_numpy(rng.integers(0, V, (B, C)).astype(np.int32)).to(dev)
        gidx = cols.to(torch.int64)
        rp = torch.arange(0, B * C + 1, C, dtype=torch.int32, device=dev)
        cand, n = (rp, cols.reshape(-1)), B * C
        out = torch.empty(n, dtype=torch.float32, device=dev)

        def plain_new():
            m.ctx.decode_candidates(h, Wd, bd, cand, n, out)

        def plain_dense():
            m.ctx.decode_dense(h, y, apply_sigmoid=True)
            return torch.gather(y, 1, gidx)

        def titled_new():
            mt.ctx.mix_candidates(m.ctx, h, Wd, bd, feat, WT, bT, w_t, w_p, cand, n, out)

        def titled_dense():
            m.ctx.decode_dense(h, y, apply_sigmoid=True)
            mt.ctx.decode_dense(feat, ts, apply_sigmoid=True)
            m.ctx.check(m.ctx.lib.dae_mix_scores(m.ctx.h, P(ts), int(ts.stride(0)), P(y), int(y.stride(0)), P(w_t), P(w_p), B, V))
            return torch.gather(y, 1, gidx)

        for label, new, dense in (("plain", plain_new, plain_dense), ("titled", titled_new, titled_dense)):
            new(); want = dense()                                   # (also the warm-up of both shapes)
            same = bool(torch.equal(out.view(torch.int32).reshape(B, C), want.view(torch.int32)))
            t_new, t_dense = [], []
            for _ in range(a.runs):
                t_new.append(timed(new, a.iters))
                t_dense.append(timed(dense, a.iters))
            mn, md = float(np.median(t_new)), float(np.median(t_dense))
            rows_bytes = n * (H + (mt.ld if label == "titled" else 0)) * 4
            case = {"route": label, "C": C, "bit_equal": same, "new_ms": t_new, "dense_ms": t_dense, "new_median_ms": mn,
                    "dense_median_ms": md, "ahead_in_every_pair": all(x < d for x, d in zip(t_new, t_dense)),
                    "gathered_TBps": rows_bytes / (mn * 1e-3) / 1e12}
            res["cases"].append(case)
            print("%-6s C = %6d: candidates %8.3f ms (%s)  dense + gather %8.3f ms (%s)  ratio %.2fx  rows gathered at %.2f TB/s  bits %s"
                  % (label, C, mn, " ".join("%.3f" % x for x in t_new), md, " ".join("%.3f" % x for x in t_dense), md / mn,
                     case["gathered_TBps"], "equal" if same else "DIFFER"))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
