"""--pretrain / --dae driver (reference main_runner/main_train.py, INTENDED behaviour: the
snapshot does not run; citations relative to /root/reference).

Loop (main_train.py:193-253): next_batch -> input keep-prob ~ U(input_kp range) -> fair coin:
feed tracks-only or artists-only as x, tracks+artists as y -> one Adam step.  When the reader
wraps, evaluate r-precision on every test split (seed tracks in, top-500 out, main_train.py:48-100)
and save the parameters if the summed r-precision over `update_seed` did not get worse.
"""
import datetime
import os
import random

import numpy as np

from ..models.DAEs import DAE, DAE_tied, DAE_title
from ..models.title_models import get_model
from ..utils import metrics as met
from ..utils.data_reader import data_reader, data_reader_firstN, data_reader_test


def log_write(conf, log):
    if int(os.environ.get("RANK", "0")) != 0:
        return
    with open(os.path.join(conf.dir, 'log.txt'), "a") as f:
        f.write(log)
        f.write('\n')
    if getattr(conf, 'verbose', True):
        print(log)


def eval(reader_test, conf, model, extra=None):
    """Mean r-precision over one test split (main_train.py:48-100): seed tracks only, both
    keep-probs 1.0, rank the track columns, drop the seeds, top 500.  `extra`: a dict that receives the split's mean
    'ndcg' and 'clicks' (utils/metrics.py get_ndcg / get_rsc) as well -- [BASE] eval_metrics = all."""
    total, count = 0.0, len(reader_test.playlists)
    ndcg, clicks = 0.0, 0
    answers = []

    def feeds():
        while True:
            x_positions, test_seed, test_answer, titles, x_ones = reader_test.next_batch_test()
            answers.append(test_answer)
            yield x_positions, x_ones, test_seed, titles
            if reader_test.test_idx == 0:
                break

    if hasattr(model, 'evaluate_iter'):
        # the rows' metrics on the device (models/DAEs.py evaluate_iter): 24 bytes a row come back instead of 500 indices, and
        # what this thread adds up, row by row in the reader's order, are the same Python floats eval_topk returns
        from ..models.DAEs import SEEDS_FROM_INPUT
        pad = [-1] * conf.strmaxlen if conf.mode == 'title' else None

        def pairs():
            for x_positions, x_ones, test_seed, titles in feeds():
                if conf.mode == 'title':                           # (titles_use as in results() below)
                    use = np.array([0.0 if t is None else 1.0 for t in titles], np.float32)
                    feed = (x_positions, x_ones, SEEDS_FROM_INPUT, len(test_seed), [t if t is not None else pad for t in titles], use)
                else:
                    feed = (x_positions, x_ones, SEEDS_FROM_INPUT, len(test_seed))
                yield feed, answers.pop()
        for rec in model.evaluate_iter(pairs(), k=500):
            for r in met.finish_r_precision_rows(rec):
                total += r
            if extra is not None:
                for r in met.finish_ndcg_rows(rec):
                    ndcg += r
                clicks += sum(met.finish_rsc_rows(rec))
        if extra is not None:
            extra['ndcg'], extra['clicks'] = ndcg / max(count, 1), clicks / max(count, 1)
        return total / max(count, 1)

    def results():
        if conf.mode == 'title':                                   # main_train.py:69-79: titles_use = 1 everywhere
            # ... for rows that HAVE a title (every row of a file this repo's or the reference's generator
            # writes).  A 5-field row (the snapshot reader's layout) carries none: mixing in the score of an
            # all-padding title would rank a 0-seed row on noise, so such rows take titles_use = 0.
            pad = [-1] * conf.strmaxlen
            from ..models.DAEs import SEEDS_FROM_INPUT

            def titled():
                for x_positions, x_ones, test_seed, titles in feeds():
                    use = np.array([0.0 if t is None else 1.0 for t in titles], np.float32)
                    yield (x_positions, x_ones, SEEDS_FROM_INPUT, len(test_seed),
                           [t if t is not None else pad for t in titles], use)
            for idx, _score in model.recommend_iter(titled(), k=500, want_scores=False):
                yield idx
        elif hasattr(model, 'recommend_iter'):
            # the evaluation seeds are the seed tracks the reader feeds (main_train.py:64-68): cut out of the input on
            # the device; batches streamed (upload / launch of batch n + 1 before the fetch of batch n)
            from ..models.DAEs import SEEDS_FROM_INPUT
            stream = ((xp, xo, SEEDS_FROM_INPUT, len(seed)) for xp, xo, seed, _t in feeds())
            for idx, _score in model.recommend_iter(stream, k=500, want_scores=False):
                yield idx
        else:
            for x_positions, x_ones, test_seed, _t in feeds():
                yield model.recommend(x_positions, x_ones, test_seed, k=500, n_rows=len(test_seed))[0]

    for b_no, idx in enumerate(results()):
        for i in range(len(idx)):
            total += met.eval_topk(idx[i], answers[b_no][i])
        if extra is not None:
            for rec in met.rank_records(idx, answers[b_no]):
                ndcg += met.finish_ndcg(rec)
                clicks += met.finish_rsc(rec)
    if extra is not None:
        extra['ndcg'], extra['clicks'] = ndcg / max(count, 1), clicks / max(count, 1)
    return total / max(count, 1)


def _eval_splits(readers_test, conf, model, rank, world, extras=None):
    """r-precision of every test split (`extras`: a dict that receives split -> (ndcg, clicks) as well).  Under torch.distributed.run the splits are dealt round-robin to the ranks
    (every rank holds a full, freshly synchronised replica for inference) and the values meet in one all-reduce, so
    the evaluation of an epoch costs 1/world of what every-rank-evaluates-everything did."""
    names = list(readers_test)
    if extras is None:
        vals = [eval(readers_test[n], conf, model) if i % world == rank else 0.0 for i, n in enumerate(names)]
    else:                                                            # three values per split
        vals = []
        for i, n in enumerate(names):
            ex = {'ndcg': 0.0, 'clicks': 0.0}
            vals.append([eval(readers_test[n], conf, model, ex) if i % world == rank else 0.0, ex['ndcg'], ex['clicks']])
    if world > 1 and names:
        import torch
        import torch.distributed as dist
        # (gloo, the one-device rehearsal of the flow, reduces on the host)
        t = torch.tensor(vals, dtype=torch.float64,
                         device="cpu" if dist.get_backend() == "gloo" else torch.device("cuda", conf.device_index))
        dist.all_reduce(t)
        vals = t.tolist()
    if extras is not None:
        extras.update((n, (v[1], v[2])) for n, v in zip(names, vals))
        vals = [v[0] for v in vals]
    return dict(zip(names, vals))


def _log_splits(conf, readers_test, rprecs, extras):
    """The reference's line per split; with [BASE] eval_metrics = all two more (NDCG, recommended-songs clicks)."""
    for seed_num in readers_test:
        log_write(conf, "seed num: %s rprecision: %f" % (seed_num, rprecs[seed_num]))
        if extras is not None:
            log_write(conf, "seed num: %s ndcg: %f" % (seed_num, extras[seed_num][0]))
            log_write(conf, "seed num: %s clicks: %f" % (seed_num, extras[seed_num][1]))


RANK_CUTS = (500, 1000, 5000, 10000)


def eval_ranks(reader_test, conf, model):
    """[BASE] eval_ranks = on: the EXACT ranks of one test split's held-out tracks among all rankable tracks of their rows
    (model.rank_of, feed by feed; seeds = the input's tracks, as in eval) -> (MRR, median rank, recall at RANK_CUTS).  A
    held-out track outside the vocabulary (-1) is a miss that counts in the denominators."""
    from ..models.DAEs import SEEDS_FROM_INPUT
    ranks = []
    while True:
        x_positions, test_seed, test_answer, _titles, x_ones = reader_test.next_batch_test()
        for row in model.rank_of(x_positions, x_ones, [list(a) for a in test_answer], SEEDS_FROM_INPUT, n_rows=len(test_seed)):
            ranks.append(row)
        if reader_test.test_idx == 0:
            break
    ranks = np.concatenate(ranks) if ranks else np.zeros(0, np.int32)
    return met.mean_reciprocal_rank(ranks), met.median_rank(ranks), met.recall_at(ranks, RANK_CUTS)


def _log_ranks(conf, readers_test, model):
    """One more line per split, behind the existing ones.  Every rank of a distributed run computes it (the model's calls may
    be collective); rank 0 logs."""
    if getattr(conf, 'eval_ranks', 'off') != 'on':
        return
    for seed_num in readers_test:
        mrr, med, rec = eval_ranks(readers_test[seed_num], conf, model)
        log_write(conf, "seed num: %s ranks: mrr %f median %.1f %s"
                  % (seed_num, mrr, med, ' '.join("recall@%d %f" % (k, v) for k, v in zip(RANK_CUTS, rec))))


def eval_mixed_ranks(reader_test, conf, model):
    """[BASE] eval_mixed_ranks = on (--title): `eval_ranks` under the title mix -- model.mixed_rank_of, feed by feed, with the
    split's titles and titles_use as `eval` feeds them (a row without a title takes titles_use = 0 and an all-padding title)
    -> (MRR, median rank, recall at RANK_CUTS).  A held-out track outside the vocabulary (-1) is a miss that counts in the
    denominators."""
    from ..models.DAEs import SEEDS_FROM_INPUT
    pad = [-1] * conf.strmaxlen
    ranks = []
    while True:
        x_positions, test_seed, test_answer, titles, x_ones = reader_test.next_batch_test()
        use = np.array([0.0 if t is None else 1.0 for t in titles], np.float32)
        for row in model.mixed_rank_of(x_positions, x_ones, [list(a) for a in test_answer], SEEDS_FROM_INPUT,
                                       [t if t is not None else pad for t in titles], use, n_rows=len(test_seed)):
            ranks.append(row)
        if reader_test.test_idx == 0:
            break
    ranks = np.concatenate(ranks) if ranks else np.zeros(0, np.int32)
    return met.mean_reciprocal_rank(ranks), met.median_rank(ranks), met.recall_at(ranks, RANK_CUTS)


def _log_mixed_ranks(conf, readers_test, model):
    """As `_log_ranks`, for [BASE] eval_mixed_ranks under --title: one more line per split, behind the existing ones."""
    if getattr(conf, 'eval_mixed_ranks', 'off') != 'on' or getattr(conf, 'mode', None) != 'title':
        return
    for seed_num in readers_test:
        mrr, med, rec = eval_mixed_ranks(readers_test[seed_num], conf, model)
        log_write(conf, "seed num: %s mixed ranks: mrr %f median %.1f %s"
                  % (seed_num, mrr, med, ' '.join("recall@%d %f" % (k, v) for k, v in zip(RANK_CUTS, rec))))


def eval_ensemble_ranks(reader_test, conf, model):
    """[BASE] eval_ensemble_ranks = on: `eval_ranks` under the ensemble's y -- model.rank_of (models/ensemble.py), feed by feed
    over the feeds of `eval_mixed_ranks` (titles and titles_use under --title) with the seeds cut out of the input
    -> (MRR, median rank, recall at RANK_CUTS).  A held-out track outside the vocabulary (-1) is a miss that counts in the
    denominators."""
    from ..models.ensemble import split_feeds
    titled = getattr(conf, 'mode', None) == 'title'
    ranks = []
    for f in split_feeds(reader_test, titled, getattr(conf, 'strmaxlen', None)):
        kw = {"titles": f[5], "titles_use": f[6]} if titled else {}
        for row in model.rank_of(f[0], f[1], f[2], f[3], n_rows=f[4], **kw):
            ranks.append(row)
    ranks = np.concatenate(ranks) if ranks else np.zeros(0, np.int32)
    return met.mean_reciprocal_rank(ranks), met.median_rank(ranks), met.recall_at(ranks, RANK_CUTS)


def _log_ensemble_ranks(conf, readers_test, model):
    """As `_log_ranks`, for [BASE] eval_ensemble_ranks beside [BASE] ensemble: one more line per split, behind the existing ones."""
    if getattr(conf, 'eval_ensemble_ranks', 'off') != 'on':
        return
    for seed_num in readers_test:
        mrr, med, rec = eval_ensemble_ranks(readers_test[seed_num], conf, model)
        log_write(conf, "seed num: %s ensemble ranks: mrr %f median %.1f %s"
                  % (seed_num, mrr, med, ' '.join("recall@%d %f" % (k, v) for k, v in zip(RANK_CUTS, rec))))


def heldout_targets(x_positions, test_answer, n_input):
    """The targets of a test feed's held-out loss as COO positions: the input's entries plus the held-out answers that lie in the
    vocabulary, one entry per (row, column)."""
    pos = [np.asarray(x_positions, np.int64).reshape(-1, 2)]
    for r, ans in enumerate(test_answer):
        a = np.asarray([c for c in ans if 0 <= c < n_input], np.int64)
        pos.append(np.stack([np.full(a.size, r, np.int64), a], axis=1))
    return np.unique(np.concatenate(pos), axis=0)


def eval_loss(reader_test, conf, model):
    """[BASE] eval_loss = on: the mean over one test split's playlists of the row loss (model.loss per row, feed by feed, so a
    short last feed is averaged correctly): input = the reader's test feed, targets = `heldout_targets`, all with weight 1;
    keep probabilities 1, no lambda term."""
    total, count = 0.0, 0
    while True:
        x_positions, test_seed, test_answer, _titles, x_ones = reader_test.next_batch_test()
        y_positions = heldout_targets(x_positions, test_answer, model.n_input)
        _cost, rows = model.loss(x_positions, x_ones, y_positions, np.ones(len(y_positions), np.float32), n_rows=len(test_seed),
                                 per_row=True)
        total += float(np.sum(rows, dtype=np.float64))
        count += len(test_seed)
        if reader_test.test_idx == 0:
            break
    return total / max(count, 1)


def _log_loss(conf, readers_test, model):
    """As `_log_ranks`, for [BASE] eval_loss: one more line per split, behind the existing ones; every rank computes, rank 0 logs."""
    if getattr(conf, 'eval_loss', 'off') != 'on':
        return
    for seed_num in readers_test:
        log_write(conf, "seed num: %s heldout loss: %f" % (seed_num, eval_loss(readers_test[seed_num], conf, model)))


def eval_mixed_loss(reader_test, conf, model):
    """[BASE] eval_mixed_loss = on (--title): `eval_loss` under the title mix -- the mean over one test split's playlists of the
    row loss of the MIXED score (model.mixed_loss per row, feed by feed, so a short last feed is averaged correctly): input = the
    reader's test feed, targets = `heldout_targets`, all with weight 1; titles and titles_use as `eval_mixed_ranks` feeds them (a
    row without a title takes titles_use = 0 and an all-padding title); keep probabilities 1."""
    pad = [-1] * conf.strmaxlen
    total, count = 0.0, 0
    while True:
        x_positions, test_seed, test_answer, titles, x_ones = reader_test.next_batch_test()
        use = np.array([0.0 if t is None else 1.0 for t in titles], np.float32)
        y_positions = heldout_targets(x_positions, test_answer, model.n_input)
        _cost, rows = model.mixed_loss(x_positions, x_ones, y_positions, np.ones(len(y_positions), np.float32),
                                       [t if t is not None else pad for t in titles], use, n_rows=len(test_seed), per_row=True)
        total += float(np.sum(rows, dtype=np.float64))
        count += len(test_seed)
        if reader_test.test_idx == 0:
            break
    return total / max(count, 1)


def _log_mixed_loss(conf, readers_test, model):
    """As `_log_loss`, for [BASE] eval_mixed_loss under --title: one more line per split, behind the existing ones."""
    if getattr(conf, 'eval_mixed_loss', 'off') != 'on' or getattr(conf, 'mode', None) != 'title':
        return
    for seed_num in readers_test:
        log_write(conf, "seed num: %s mixed heldout loss: %f" % (seed_num, eval_mixed_loss(readers_test[seed_num], conf, model)))


def _refuse_ranks_under_title(conf, only_testmode=True):
    if getattr(conf, 'eval_mixed_loss', 'off') == 'on':
        if getattr(conf, 'mode', None) != 'title':
            raise ValueError("[BASE] eval_mixed_loss = on is available under --title only: the other modes have no title mix "
                             "(remove the key, set eval_mixed_loss = off, or use eval_loss)")
        if getattr(conf, 'ensemble', None):
            raise ValueError("[BASE] eval_mixed_loss = on is set beside [BASE] ensemble: an ensemble has no loss "
                             "(set eval_mixed_loss = off)")
        if not only_testmode and int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise ValueError("[BASE] eval_mixed_loss = on is not available for a vocabulary-sharded title scorer (a training run "
                             "under torch.distributed.run): partial costs across ranks are not built (set eval_mixed_loss = off)")
    if getattr(conf, 'eval_loss', 'off') == 'on':
        if getattr(conf, 'mode', None) == 'title':
            raise ValueError("[BASE] eval_loss = on is not available under --title: the loss of the mixed score is another kernel, "
                             "[BASE] eval_mixed_loss = on (remove the key or set eval_loss = off)")
        if getattr(conf, 'ensemble', None):
            raise ValueError("[BASE] eval_loss = on is set beside [BASE] ensemble: an ensemble has no loss (set eval_loss = off)")
        if not only_testmode and int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise ValueError("[BASE] eval_loss = on is not available for a vocabulary-sharded model (a training run under "
                             "torch.distributed.run): partial costs across ranks are not built (set eval_loss = off)")
    if getattr(conf, 'eval_ranks', 'off') == 'on' and getattr(conf, 'mode', None) == 'title':
        raise ValueError("[BASE] eval_ranks = on is not available under --title: it ranks by the DAE's own logits; the ranks "
                         "under the title mix are [BASE] eval_mixed_ranks = on (remove the key or set eval_ranks = off)")
    if getattr(conf, 'eval_mixed_ranks', 'off') == 'on' and getattr(conf, 'mode', None) != 'title':
        raise ValueError("[BASE] eval_mixed_ranks = on is available under --title only: the other modes have no title mix "
                         "(remove the key, set eval_mixed_ranks = off, or use eval_ranks)")


def _init_distributed(conf):
    """One process per GPU under torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE in the env):
    RCCL process group, this rank's device, and the SAME host RNG streams on every rank so that all
    ranks draw the same batches, coin flips and keep-probabilities (the batch is replicated, the
    vocabulary rows are sharded).  Returns (rank, world)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return 0, 1
    import torch
    import torch.distributed as dist
    rank = int(os.environ["RANK"])
    conf.device_index = int(os.environ.get("LOCAL_RANK", rank))
    torch.cuda.set_device(conf.device_index)
    if not dist.is_initialized():
        # DAE_DIST_BACKEND=gloo: the N > 1 flow on one device (main_challenge reads the same variable)
        dist.init_process_group(os.environ.get("DAE_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
    random.seed(int(getattr(conf, "seed", 0)))
    np.random.seed(int(getattr(conf, "seed", 0)))
    conf.verbose = getattr(conf, "verbose", True) and rank == 0
    return rank, world


def _refuse_ensemble(conf, only_testmode):
    """[BASE] ensemble outside the runs that honour it (main.py refuse_ensemble says the same from the command line)."""
    if not getattr(conf, 'ensemble', None):
        if getattr(conf, 'eval_ensemble_ranks', 'off') == 'on':
            raise ValueError("[BASE] eval_ensemble_ranks = on is set without [BASE] ensemble: there is no ensemble to rank under "
                             "(remove the key, set eval_ensemble_ranks = off, or use eval_ranks)")
        return
    if not only_testmode:
        raise ValueError("[BASE] ensemble is set, and this is a training run: the key is honoured by --challenge, --dae --testmode "
                         "and --title --testmode only (remove [BASE] ensemble / ensemble_alpha to train)")
    if getattr(conf, 'mode', None) not in ('dae', 'title'):
        raise ValueError("[BASE] ensemble is set, and --%s --testmode evaluates that model alone: the key is honoured by "
                         "--challenge, --dae --testmode and --title --testmode only" % getattr(conf, 'mode', None))
    for key in ('eval_ranks', 'eval_mixed_ranks'):
        if getattr(conf, key, 'off') == 'on':
            raise ValueError("[BASE] ensemble is set with [BASE] %s = on: an ensemble has no rank_of (set %s = off)" % (key, key))
    split = getattr(conf, 'ensemble_fit', None)
    if split and not os.path.exists(os.path.join(conf.data_dir, split[0])):
        raise ValueError("[BASE] ensemble_fit = %s: the split's file %s is missing" % (split[0], os.path.join(conf.data_dir, split[0])))


def run(conf, only_testmode):
    _refuse_ranks_under_title(conf, only_testmode)
    _refuse_ensemble(conf, only_testmode)
    rank, world = _init_distributed(conf)
    # the training reader (main_train.py:129-133): whole playlists, or -- with a [DAE] firstN_range -- their first-N prefixes
    reader_args = dict(data_dir=conf.data_dir, filename='train', batch_size=conf.batch)
    reader = data_reader(**reader_args) if -1 in conf.firstN else data_reader_firstN(from_to=conf.firstN, **reader_args)
    # what the models read off `conf` (main_train.py:134-148): the vocabulary and title shapes come from the data file
    for attr, value in (("class_divpnt", reader.class_divpnt), ("n_tracks", reader.num_tracks), ("n_input", reader.num_items),
                        ("n_output", reader.num_items), ("charsize", reader.num_char), ("strmaxlen", reader.max_title_len)):
        setattr(conf, attr, value)
    kp_range = conf.input_kp

    readers_test = {}
    for seed in conf.test_seed:
        path = os.path.join(conf.data_dir, seed)
        if not os.path.exists(path):
            log_write(conf, "test split %s not found, skipped" % path)
            continue
        readers_test[seed] = data_reader_test(data_dir=conf.data_dir, filename=seed,
                                              batch_size=conf.batch, test_num=conf.testsize)
    print(conf.n_input)

    if conf.mode == 'pretrain':                                     # main_train.py:154-161
        info, model = '[pretrain mode]', DAE_tied(conf)
    elif conf.mode == 'dae':
        if only_testmode:
            conf.initval = conf.save
        info, model = '[dae mode]', DAE(conf)
    elif conf.mode == 'title':                                      # main_train.py:162-165
        model_title = get_model(conf)
        model_title.fit()
        if only_testmode:
            model_title.load(conf.save + '.pkl')
        info, model = '[title mode]', DAE_title(conf, model_title)
    else:
        raise ValueError("unknown mode %r" % conf.mode)
    log_write(conf, '*' * 10)
    log_write(conf, info + ' start at ' + str(datetime.datetime.now()))
    model.fit()
    if world > 1 and not only_testmode:
        if conf.mode == 'title':              # the output layer's columns over the ranks; the DAE is frozen
            model.shard_title_training(rank, world)
            log_write(conf, "title training sharded over %d ranks" % world)
        else:
            model.shard_training(rank, world)

    if only_testmode:                                               # main_train.py:181-191
        log_write(conf, '<<only test mode>>')
        if getattr(conf, 'ensemble', None):
            # [BASE] ensemble: the splits are ranked by the ensemble around this model (models/ensemble.py), feed by feed
            from ..models.ensemble import fit_from_conf, from_conf
            model = from_conf(conf, model)
            log_write(conf, 'ensemble: %d members, alphas %s' % (len(model.members), ', '.join('%g' % a for a in model.alphas)))
            fitted = fit_from_conf(conf, model, conf.mode == 'title')         # [BASE] ensemble_fit: before anything is evaluated
            if fitted:
                log_write(conf, fitted)
        extras = {} if getattr(conf, 'eval_metrics', 'rprecision') == 'all' else None
        out = _eval_splits(readers_test, conf, model, rank, world, extras)
        _log_splits(conf, readers_test, out, extras)
        _log_ranks(conf, readers_test, model)
        _log_mixed_ranks(conf, readers_test, model)
        _log_ensemble_ranks(conf, readers_test, model)
        _log_loss(conf, readers_test, model)
        _log_mixed_loss(conf, readers_test, model)
        return out

    # [BASE] train_feed = device: the training set lives on the device and a batch goes up as the reader's draws alone
    # (title mode: its title rows too)
    device_feed = getattr(conf, 'train_feed', 'host') == 'device'
    if device_feed:
        model.attach_train_set(reader)

    epoch, it, loss, max_eval = 0, 0, 0.0, 0.0
    history = []
    while True:
        start_idx = reader.train_idx
        if device_feed:
            draw = reader.next_batch_draw()
        else:
            trk_positions, art_positions, y_positions, _titles, trk_val, art_val = reader.next_batch()
        end_idx = reader.train_idx
        input_kp = random.uniform(kp_range[0], kp_range[-1])        # main_train.py:199
        if device_feed and conf.mode == 'title':
            # :214-221 from the draw: the whole playlist is input and target with value 1, whatever the reader's given counts
            # say, and -- like the host loop below -- no coin is drawn
            draw[1:] = -1
            l = model.train_step_draw(draw, 2, conf.kp, input_kp, fetch_cost=False, title_keep_prob=conf.title_kp)
            l = l.double()      # summed on the device as the host loop sums its Python floats: the epoch's loss keeps its bits
        elif device_feed:                                           # the same coin, after the same draws
            l = model.train_step_draw(draw, int(np.random.randint(2) != 0), conf.kp, input_kp, fetch_cost=False)
        elif conf.mode == 'title':                                    # :214-221: the whole playlist is input and target
            ones = np.ones(len(y_positions), np.float32)
            l = model.train_step(y_positions, ones, y_positions, ones, conf.kp, input_kp, titles=_titles,
                                 titles_use=np.ones(conf.batch, np.float32), title_keep_prob=conf.title_kp)
        else:
            if np.random.randint(2) == 0:                           # :202 fair coin
                x_pos, x_val = trk_positions, trk_val
            else:
                x_pos, x_val = art_positions, art_val
            # the cost stays on the device (a 0-dim tensor, summed there and fetched once per epoch) so the reader
            # builds the next batch while this step runs -- single GPU and vocabulary-sharded alike
            kw = {"fetch_cost": False}
            l = model.train_step(x_pos, x_val, y_positions, np.ones(len(y_positions), np.float32),
                                 conf.kp, input_kp, **kw)
        loss = loss + l
        it += 1
        if start_idx > end_idx or end_idx == 0:                     # :227 reader wrapped
            epoch += 1
            loss = float(loss)                                      # drains the stream
            if hasattr(model, "check_feed"):
                model.check_feed()
            log_write(conf, "epoch " + str(epoch))
            log_write(conf, "training loss: " + str(loss / it))
            cur_eval = 0.0
            model.sync_params()            # collective when sharded: every rank refreshes its replica first
            extras = {} if getattr(conf, 'eval_metrics', 'rprecision') == 'all' else None
            rprecs = _eval_splits(readers_test, conf, model, rank, world, extras)
            _log_splits(conf, readers_test, rprecs, extras)
            _log_ranks(conf, readers_test, model)
            _log_mixed_ranks(conf, readers_test, model)
            _log_loss(conf, readers_test, model)
            _log_mixed_loss(conf, readers_test, model)
            for seed_num in readers_test:
                if seed_num in conf.update_seed:
                    cur_eval += rprecs[seed_num]
            history.append((epoch, loss / it, cur_eval))
            if cur_eval >= max_eval:                                # :243-249
                if rank == 0:
                    if conf.mode == 'title':
                        model.title_model.save(conf.save + '.pkl')   # the reference: saver.save(sess, conf.save)
                    else:
                        model.save_model()
                max_eval = cur_eval
                log_write(conf, "The highest score is updated. Parameters are saved")
            loss, it = 0.0, 0
            if epoch == conf.epochs:
                break
    return history
