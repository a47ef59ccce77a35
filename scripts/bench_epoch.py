"""Training throughput THROUGH the host mirror (utils/data_reader.py -> models/DAEs.py:DAE.train_step),
i.e. what `main.py --dae` sustains, at BASELINE.json configs[3] shape: V = 170 000 (140 000 tracks +
30 000 artists), H = 256, batch 256, fp32.  A synthetic `train` file of N playlists (ids Zipf over popularity
ranks, 20..100 tracks per playlist) is written to a temp dir, then the loop of main_runner/main_train.py is
timed with its parts: reader.next_batch, train_step (upload + device CSR + step + cost fetch).

  python scripts/bench_epoch.py [--playlists 20000] [--steps 200] [--tied] [--firstn 0.3,0.6] [--device-feed] [--title]

--device-feed: the loop of `[BASE] train_feed = device` -- reader.next_batch_draw, then train_step_draw (12 bytes a row up,
both CSRs built on the device from the resident training set).
--title: the loop of `main.py --title` instead: a DAE_title over the same file (titles of up to 25 characters) with the shipped
title shape -- filter_num 100, filter_size 3,5,7,9, char_emb 50, batch 150 -- on a frozen DAE; the whole playlist is input and
target, no coin.  Honours --device-feed (the title rows come out of the resident set too) and --async-cost.
"""
import argparse, json, os, random, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_train(path, n_playlists, n_tracks, n_artists, seed=0, titles=False):
    rng = np.random.default_rng(seed)
    trng = np.random.default_rng(seed + 1)          # (the titles draw from a stream of their own: the playlists stay as they were)
    pls = []
    for _ in range(n_playlists):
        c = int(rng.integers(20, 101))
        u = rng.random(c)
        t = np.unique(np.minimum(n_tracks - 1, np.floor(np.exp(u * np.log(n_tracks))).astype(np.int64) - 1).clip(0))
        a = np.unique(n_tracks + rng.integers(0, n_artists, size=max(1, c // 2)))
        title = [1, 2, 3]
        if titles:                                  # right-padded rows of max_title_len entries, as spotify_reader writes them
            k = int(trng.integers(3, 26))
            title = [int(x) for x in trng.integers(0, 41, size=k)] + [-1] * (25 - k)
        pls.append([[int(x) for x in t], [int(x) for x in a], title])
    d = {"track_uri2id": {"t%d" % i: i for i in range(n_tracks)},
         "artist_uri2id": {"a%d" % i: n_tracks + i for i in range(n_artists)},
         "max_title_len": 25, "num_char": 41, "class_divpnt": [], "playlists": pls}
    with open(path, "w") as f:
        json.dump(d, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--playlists", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--tied", action="store_true")
    ap.add_argument("--async-cost", action="store_true", help="fetch the cost once at the end instead of per step")
    ap.add_argument("--bf16", action="store_true", help="train_dtype = bf16 (the three GEMMs on bf16 operands)")
    ap.add_argument("--encoder-adam", choices=["rows", "dense"], default="rows",
                    help="untied encoder: dae_adam_rows_* (default) or the dense dae_adam_step")
    ap.add_argument("--decoder-adam", choices=["fused", "dense"], default="fused",
                    help="untied decoder: Adam inside the decoder-gradient kernel (default) or dae_adam_step")
    ap.add_argument("--host-csr", action="store_true", help="device_csr = False: feed -> CSR with numpy on the host")
    ap.add_argument("--device-feed", action="store_true", help="train_feed = device: next_batch_draw + train_step_draw")
    ap.add_argument("--firstn", default=None, metavar="LO,HI", help="data_reader_firstN with this firstN_range (e.g. 0.3,0.6)")
    ap.add_argument("--title", action="store_true", help="the --title loop: DAE_title, shipped title shape, batch 150")
    ap.add_argument("--flush-every", type=int, default=32, help="rows-Adam: all rows brought up to date every N steps")
    args = ap.parse_args()
    import torch
    from spotify_recsys_challenge_2018_amd.models.DAEs import DAE, DAE_tied, DAE_title
    from spotify_recsys_challenge_2018_amd.utils.data_reader import data_reader, data_reader_firstN

    nt, na = 140000, 30000
    tmp = tempfile.mkdtemp()
    B = 150 if args.title else 256
    write_train(os.path.join(tmp, "train"), args.playlists, nt, na, titles=args.title)
    if args.firstn:
        reader = data_reader_firstN(data_dir=tmp, filename="train", batch_size=B, from_to=[float(t) for t in args.firstn.split(",")])
    else:
        reader = data_reader(data_dir=tmp, filename="train", batch_size=B)

    class C: pass
    conf = C()
    conf.n_tracks, conf.n_input, conf.n_output = nt, nt + na, nt + na
    conf.hidden, conf.batch, conf.lr, conf.reg_lambda = 256, B, 0.005, 0.0
    conf.initval, conf.save, conf.kp = "NULL", os.path.join(tmp, "w"), 0.8
    conf.device_index = 0
    conf.encoder_adam = args.encoder_adam
    conf.decoder_adam = args.decoder_adam
    conf.device_csr = not args.host_csr
    conf.rows_adam_flush_every = args.flush_every
    if args.bf16:
        conf.train_dtype = "bf16"
    if args.title:
        import pickle
        from spotify_recsys_challenge_2018_amd.models.title_models import get_model
        from spotify_recsys_challenge_2018_amd.utils.synthetic import make_weights
        W_enc, b_enc, W_dec, b_dec = make_weights(nt + na, 256, seed=1, bias="zipf", n_tracks=nt)
        conf.DAEval = os.path.join(tmp, "w_dae")                 # the frozen DAE
        with open(conf.DAEval, "wb") as f:
            pickle.dump([W_enc, W_dec, b_enc, b_dec], f)
        conf.char_model, conf.charsize, conf.strmaxlen = "Char_CNN", reader.num_char, reader.max_title_len
        conf.char_emb, conf.filter_num, conf.filter_size, conf.title_lr = 50, 100, [3, 5, 7, 9], 0.001
        title_model = get_model(conf)
        title_model.fit()
        model = DAE_title(conf, title_model)
    else:
        model = (DAE_tied if args.tied else DAE)(conf)
    model.fit()
    if args.device_feed:
        model.attach_train_set(reader)
    random.seed(0); np.random.seed(0)

    def one(fetch=True):
        t0 = time.perf_counter()
        if args.device_feed:
            draw = reader.next_batch_draw()
        else:
            trk, art, y, _t, tv, av = reader.next_batch()
        t1 = time.perf_counter()
        kp = random.uniform(0.5, 0.8)
        kw = {} if fetch else {"fetch_cost": False}
        if args.title and args.device_feed:
            draw[1:] = -1
            l = model.train_step_draw(draw, 2, 0.8, kp, title_keep_prob=0.8, **kw)
        elif args.title:
            ones = np.ones(len(y), np.float32)
            l = model.train_step(y, ones, y, ones, 0.8, kp, titles=_t, titles_use=np.ones(B, np.float32), title_keep_prob=0.8, **kw)
        elif args.device_feed:
            l = model.train_step_draw(draw, int(np.random.randint(2) != 0), 0.8, kp, **kw)
        else:
            x, xv = (trk, tv) if np.random.randint(2) == 0 else (art, av)
            l = model.train_step(x, xv, y, np.ones(len(y), np.float32), 0.8, kp, **kw)
        t2 = time.perf_counter()
        return t1 - t0, t2 - t1, l

    for _ in range(10):
        one()
    torch.cuda.synchronize()
    tr = ts = 0.0
    t0 = time.perf_counter()
    for _ in range(args.steps):
        a, b, l = one(fetch=not args.async_cost)
        tr += a; ts += b
    model.sync_params()                 # rows-Adam: every encoder row brought up to date (part of the epoch's work)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    print(json.dumps({"what": "main_train loop through the host mirror (%s)" % ("title" if args.title else "tied" if args.tied else "untied"),
                      "ms_per_step": round(wall / args.steps * 1e3, 3),
                      "playlists_per_s": round(B * args.steps / wall, 1),
                      "reader_ms": round(tr / args.steps * 1e3, 3), "train_step_call_ms": round(ts / args.steps * 1e3, 3),
                      "async_cost": bool(args.async_cost), "encoder_adam": "dense" if args.tied else args.encoder_adam,
                      "train_dtype": "bf16" if args.bf16 else "f32", "feed": "device" if args.device_feed else "host",
                      "firstn": args.firstn, "last_cost": float(l)}))


if __name__ == "__main__":
    main()
