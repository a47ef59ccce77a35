#!/usr/bin/env python
"""Device time of one --title training step at the shipped title shape (V = 170 000, hidden 256, 3/5/7/9 x 100 filters ->
448 feature columns, batch 150, fp32), feeds resident on the device, one variant per process:

  unsharded   DAE_title._title_step_csr as a single process runs it
  world1      the vocabulary-sharded path with one rank (shard_title_training(0, 1)): every column, no collective
  shard8      rank 0 of eight (shard_bounds(V, 8, 0)) run ALONE, the three collectives replaced by nothing: the compute
              of one shard, an upper bound of what eight ranks could gain -- not a speed-up

--tree PATH imports the package from another checkout (the parent commit's, for `unsharded`).  Prints one JSON line."""
import argparse
import json
import os
import pickle
import sys
import tempfile

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["unsharded", "world1", "shard8"], required=True)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    import torch
    from spotify_recsys_challenge_2018_amd.models.DAEs import DAE_title
    from spotify_recsys_challenge_2018_amd.models.title_models import get_model
    from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights
    nt, na, H, B = 140000, 30000, 256, 150
    V = nt + na
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=0, bias="zipf", n_tracks=nt)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "w_dae")
    with open(path, "wb") as f:
        pickle.dump([W_enc, W_dec, b_enc, b_dec], f)

    class C:
        batch = B; n_input = V; n_output = V; n_tracks = nt; hidden = H; lr = 0.001; reg_lambda = 0.0
        char_emb = 50; strmaxlen = 25; charsize = 41; char_model = 'Char_CNN'; filter_num = 100
        filter_size = [3, 5, 7, 9]; save = os.path.join(tmp, "unused"); initval = "NULL"; DAEval = path; title_lr = 0.001
    mt = get_model(C()); mt.fit()
    m = DAE_title(C(), mt); m.fit()
    cols = (0, V)
    if a.variant != "unsharded":
        world = 1 if a.variant == "world1" else 8
        m.shard_title_training(0, world)
        tr = m._title_sharded
        cols = (tr.lo, tr.hi)
        if world > 1:                                        # the shard alone: no peers, no collectives
            tr._allreduce = tr._broadcast0 = lambda t: None
    pos, _ones, _seeds = make_playlists(B, nt, na, seed=1, seed_counts=(20, 50, 100))
    yo = np.ones(len(pos), np.float32)
    rng = np.random.default_rng(0)
    titles = rng.integers(0, 41, (B, 25)); titles[:, 18:] = -1
    m.ctx.bind_stream()
    x = m._upload_csr(pos, yo)
    d_titles = mt.titles_to_device(titles, B)
    use = torch.ones(B, dtype=torch.float32, device=d_titles.device)

    def step():
        return m._title_step_csr(x, x, d_titles, use, 0.8, 0.01, 0.8, False)
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        c = step()
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"variant": a.variant, "tree": os.path.abspath(a.tree), "columns": list(cols), "steps": a.steps,
                      "ms_per_step": round(e0.elapsed_time(e1) / a.steps, 4), "last_cost": float(c)}))


if __name__ == "__main__":
    main()
