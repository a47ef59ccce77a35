"""Command line of the reference (main.py; citations relative to /root/reference), same flags and
the same config.ini schema:

    python -m spotify_recsys_challenge_2018_amd.main --dir D {--pretrain|--dae|--challenge} [--testmode]

    [BASE] verbose data_dir result_dir testsize   (+ optional, this build only: train_dtype = f32 | bf16, decode_dtype = f32 | bf16 | exact_bf16,
                                                  eval_metrics = rprecision | all, train_feed = host | device,
                                                  eval_ranks = off | on, eval_mixed_ranks = off | on, eval_loss = off | on,
                                                  eval_mixed_loss = off | on,
                                                  ensemble = <pickle>[, <pickle> ...], ensemble_alpha = a0, a1, ...,
                                                  eval_ensemble_ranks = off | on, ensemble_fit = <seed>[, mrr | recall@N])
    [DAE] epochs batch lr reg_lambda hidden test_seed update_seed keep_prob input_kp firstN_range initval save
    [PRETRAIN] epochs batch lr reg_lambda save
    [TITLE] ... (parsed for compatibility; the title models are outside the scoring path)
    [CHALLENGE] batch challenge_data result   (+ optional, this build only: allow_no_title, shard_exchange, shard_tau_exchange, catalogue)

Kept on purpose: `[DAE]` is always read first, so --pretrain inherits hidden / keep_prob /
input_kp / firstN_range / test_seed from it (main.py:121, load-bearing per SURVEY App. A).
Repaired: booleans are parsed ("False" is false; main.py:19 uses bool(str)).
"""
import argparse
import configparser
import os


def _csv(text, cast=str):
    return [cast(t.strip()) for t in text.split(',')]


def _truth(text):
    return str(text).strip().lower() in ("1", "true", "yes", "on")


def _seeds(text):
    return ['test-' + t for t in _csv(text)]


def _floats(text):
    return _csv(text, float)


def _ints(text):
    return _csv(text, int)


# config.ini schema (reference main.py:12-94) as data: section -> (attribute, key, cast).
# "@dir" / "@result" casts join the value onto the run directory / the result directory.
_SCHEMA = {
    'BASE': (('data_dir', 'data_dir', str), ('result_dir', 'result_dir', str), ('testsize', 'testsize', int),
             ('verbose', 'verbose', _truth)),
    'DAE': (('epochs', 'epochs', int), ('batch', 'batch', int), ('lr', 'lr', float),
            ('reg_lambda', 'reg_lambda', float), ('test_seed', 'test_seed', _seeds),
            ('update_seed', 'update_seed', _seeds), ('input_kp', 'input_kp', _floats), ('kp', 'keep_prob', float),
            ('firstN', 'firstN_range', _floats), ('initval', 'initval', '@dir'), ('save', 'save', '@dir'),
            ('hidden', 'hidden', int)),
    'PRETRAIN': (('epochs', 'epochs', int), ('batch', 'batch', int), ('lr', 'lr', float),
                 ('reg_lambda', 'reg_lambda', float), ('save', 'save', '@dir')),
    # [TITLE] OVERRIDES epochs / batch / lr / input_kp / test_seed / update_seed / save of [DAE] (main.py:59-83),
    # for --title and, as in the reference, for --challenge as well; keep_prob stays the [DAE] one
    'TITLE': (('epochs', 'epochs', int), ('batch', 'batch', int), ('lr', 'lr', float), ('title_lr', 'lr', float),
              ('input_kp', 'input_kp', _floats), ('title_kp', 'title_kp', float),
              ('test_seed', 'test_seed', _seeds), ('update_seed', 'update_seed', _seeds),
              ('char_emb', 'char_emb', int), ('char_model', 'char_model', str), ('DAEval', 'DAEval', '@dir'),
              ('save', 'save', '@dir'), ('title_save', 'save', '@dir')),
    'CHALLENGE': (('challenge_data', 'challenge_data', str), ('result', 'result', '@result'),
                  ('batch', 'batch', int)),
}


class Conf:
    """Plain attribute bag the drivers and models read."""

    def __init__(self, dir, ini):
        self.dir = dir
        self.ini = ini
        self._load('BASE')
        # six OPTIONAL [BASE] keys this build adds (absent from the reference's files, which then mean fp32 / rprecision):
        #   train_dtype  = f32 | bf16   arithmetic of the training step's three GEMMs (BASELINE.json configs[3])
        #   decode_dtype = f32 | bf16 | exact_bf16   arithmetic of the scoring decode: fp32 MFMA (bit-exact path), bf16
        #                  (configs[4]), or the bf16 GEMM as a filter with the survivors recomputed in fp32 (north_star:
        #                  the fp32 lists, bit for bit)
        #   eval_metrics = rprecision | all   what the evaluation of a test split logs: the r-precision line alone (default,
        #                  the reference's log), or NDCG and recommended-songs clicks as well (utils/metrics.py get_ndcg /
        #                  get_rsc, which the reference defines and never calls); model selection reads r-precision either way
        #   train_feed   = host | device      where the training batches of --pretrain / --dae / --title are built: by the reader on the host
        #                  (default), or on the device from a resident copy of the training set -- only the reader's draws
        #                  go over the link (models/DAEs.py train_step_draw); same batches, same random draws
        #   eval_ranks   = off | on           with `on` the evaluation of a test split logs one more line behind the others: MRR, median
        #                  rank and recall@500 / 1 000 / 5 000 / 10 000 of the held-out tracks, from their EXACT ranks among all
        #                  rankable tracks (models/DAEs.py rank_of; feed by feed).  Refused under --title (main_train.run): ranks under
        #                  the title mix are eval_mixed_ranks'
        #   eval_mixed_ranks = off | on       --title only: with `on` one more line per test split behind the others, "mixed ranks: ...",
        #                  the same figures from the EXACT ranks under the title mix (models/DAEs.py DAE_title.mixed_rank_of, with the
        #                  split's titles and titles_use as the title evaluation feeds them).  Refused outside --title (main_train.run)
        #   eval_loss    = off | on           with `on` one more line per test split behind the others, "heldout loss: ...": the mean
        #                  over the split's playlists of the loss the optimiser minimises (models/DAEs.py loss, per row, feed by
        #                  feed; input = the test feed, targets = its entries and the held-out answers in the vocabulary, keep
        #                  probabilities 1, no lambda term).  Refused under --title, beside [BASE] ensemble and for a
        #                  vocabulary-sharded training run (main_train.run)
        #   eval_mixed_loss = off | on        --title only: with `on` one more line per test split behind the others, "mixed heldout
        #                  loss: ...", the same mean under the loss the title scorer minimises, the loss of the MIXED score (models/
        #                  DAEs.py DAE_title.mixed_loss, per row, feed by feed; titles and titles_use as eval_mixed_ranks feeds them).
        #                  Refused outside --title, beside [BASE] ensemble and for a vocabulary-sharded training run
        #                  (main_train.run)
        self.eval_metrics = 'rprecision'
        self.train_feed = 'host'
        self.eval_loss = 'off'
        self.eval_mixed_loss = 'off'
        self.eval_ranks = 'off'
        self.eval_mixed_ranks = 'off'
        self.eval_ensemble_ranks = 'off'
        for key, allowed in (('train_dtype', ('f32', 'bf16')), ('decode_dtype', ('f32', 'bf16', 'exact_bf16')),
                             ('eval_metrics', ('rprecision', 'all')), ('train_feed', ('host', 'device')),
                             ('eval_ranks', ('off', 'on')), ('eval_mixed_ranks', ('off', 'on')),
                             ('eval_ensemble_ranks', ('off', 'on')), ('eval_loss', ('off', 'on')),
                             ('eval_mixed_loss', ('off', 'on'))):
            if key in self.ini['BASE']:
                val = self.ini['BASE'][key].strip().lower()
                if val not in allowed:
                    raise ValueError("[BASE] %s must be one of %s, not %r" % (key, ' | '.join(allowed), val))
                setattr(self, key, val)
        # two more OPTIONAL [BASE] keys: an ensemble around the run's own model (models/ensemble.py)
        #   ensemble       = <pickle>[, <pickle> ...]   further members: pickles of the four arrays a --pretrain / --dae run saves, over
        #                    the same vocabulary (any hidden size); paths resolve in the run directory, as [TITLE] DAEval does.
        #                    Honoured by --challenge (titled when the title pickle exists, exactly as today's choice) and by
        #                    --dae --testmode / --title --testmode; refused in every other run (`refuse_ensemble`) and where the
        #                    plain DAE would run vocabulary-sharded.  Absent: every run is what it is without the key
        #   ensemble_alpha = a0, a1, ...                one weight per member, the section's own model first; default uniform
        self.ensemble, self.ensemble_alpha = [], None
        if 'ensemble' in self.ini['BASE'] and self.ini['BASE']['ensemble'].strip():
            names = _csv(self.ini['BASE']['ensemble'])
            if not all(names):
                raise ValueError("[BASE] ensemble = %r: an empty entry in the list of pickles" % self.ini['BASE']['ensemble'])
            self.ensemble = [os.path.join(self.dir, n) for n in names]
        if 'ensemble_alpha' in self.ini['BASE'] and self.ini['BASE']['ensemble_alpha'].strip():
            if not self.ensemble:
                raise ValueError("[BASE] ensemble_alpha is set without [BASE] ensemble: there are no members to weigh")
            try:
                alpha = _floats(self.ini['BASE']['ensemble_alpha'])
            except ValueError:
                raise ValueError("[BASE] ensemble_alpha = %r: a comma-separated list of numbers is required"
                                 % self.ini['BASE']['ensemble_alpha']) from None
            if len(alpha) != len(self.ensemble) + 1:
                raise ValueError("[BASE] ensemble_alpha lists %d weights for %d members (the section's own model first, then the "
                                 "%d of [BASE] ensemble)" % (len(alpha), len(self.ensemble) + 1, len(self.ensemble)))
            self.ensemble_alpha = alpha
        # ... and two about the ranks under the ensemble (models/ensemble.py rank_of / fit_alphas):
        #   eval_ensemble_ranks = off | on              --dae --testmode / --title --testmode with [BASE] ensemble: one more line per
        #                    test split behind the others, "ensemble ranks: ...", eval_ranks' figures from the EXACT ranks under the
        #                    ensemble's y.  Refused without [BASE] ensemble and in every other run (`refuse_ensemble_keys`)
        #   ensemble_fit   = <seed>[, mrr | recall@N]   before it evaluates or writes a submission, the run fits the alphas on that
        #                    test split (written as in test_seed: 5 for test-5) by the metric (default mrr) of the held-out tracks'
        #                    exact ranks (DAE_ensemble.fit_alphas) and logs them.  Honoured where [BASE] ensemble is; refused
        #                    beside ensemble_alpha, without ensemble, or when the split's file is missing
        self.ensemble_fit = None
        if 'ensemble_fit' in self.ini['BASE'] and self.ini['BASE']['ensemble_fit'].strip():
            raw = self.ini['BASE']['ensemble_fit']
            if not self.ensemble:
                raise ValueError("[BASE] ensemble_fit is set without [BASE] ensemble: there are no alphas to fit")
            if self.ensemble_alpha is not None:
                raise ValueError("[BASE] ensemble_fit and [BASE] ensemble_alpha are both set: the alphas are either fitted or "
                                 "given -- remove one of the keys")
            parts = _csv(raw)
            if len(parts) > 2 or not parts[0]:
                raise ValueError("[BASE] ensemble_fit = %r: <seed>[, <metric>] is required, e.g. 5 or 5, recall@500" % raw)
            metric = parts[1].lower() if len(parts) > 1 else 'mrr'
            if metric != 'mrr' and not (metric.startswith('recall@') and metric[7:].isdigit() and int(metric[7:]) >= 1):
                raise ValueError("[BASE] ensemble_fit = %r: the metric must be mrr or recall@N, not %r" % (raw, metric))
            self.ensemble_fit = (_seeds(parts[0])[0], metric)

    def _load(self, section):
        sec = self.ini[section]
        for attr, key, cast in _SCHEMA[section]:
            raw = sec[key]
            if cast == '@dir':
                val = os.path.join(self.dir, raw)
            elif cast == '@result':
                val = os.path.join(self.result_dir, raw)
            else:
                val = cast(raw)
            setattr(self, attr, val)
        return sec

    def set_dae_conf(self):
        self._load('DAE')
        self._check_firstN(self.firstN)
        self.mode = 'dae'

    @staticmethod
    def _check_firstN(rng):
        """The reference's range rules (main.py:35-43): a single -1 disables firstN; fractions
        must stay below 1 on both ends; counts must be integers >= 1."""
        if len(rng) == 1:
            assert rng[0] == -1.0
            return
        lo, hi = rng[0], rng[1]
        assert lo <= hi
        if hi < 1:
            assert lo == 0 or not float(lo).is_integer()
        else:
            assert lo >= 1 and float(lo).is_integer() and float(hi).is_integer()

    def set_pretrain_conf(self):
        self._load('PRETRAIN')
        self.is_pretrain = True
        self.mode = 'pretrain'

    def set_title_conf(self):
        """[TITLE] (main.py:58-86): the character-CNN title scorer trained on top of the frozen DAE `DAEval`.
        The variables are saved as `<save>.pkl` (the reference writes a TF checkpoint at `save`)."""
        sec = self._load('TITLE')
        if self.char_model == 'Char_CNN':
            self.filter_num = int(sec['filter_num'])
            self.filter_size = _ints(sec['filter_size'])
        os.makedirs(os.path.dirname(self.save) or '.', exist_ok=True)      # main.py:80-82
        self.mode = 'title'

    def set_challenge_oonf(self):          # (sic) the reference's spelling, main.py:88
        os.makedirs(self.result_dir, exist_ok=True)
        sec = self._load('CHALLENGE')
        # four OPTIONAL [CHALLENGE] keys this build adds (absent from the reference's files):
        #   allow_no_title = True        score with the plain DAE when <[TITLE] save>.pkl is missing (default: error --
        #                                the reference fails there too; also an error while any playlist has no seeds)
        #   shard_exchange = allgather | alltoall    under torch.distributed.run: how the per-shard top-500 meet
        #   shard_tau_exchange = False   ... without the exchange of the shards' thresholds before their filter launches
        #                                (default True: one more collective of 4 bytes per row and rank, same result,
        #                                the ranks holding unpopular tracks stop keeping 10x the candidates)
        #   catalogue = <file>           rank inside a catalogue: a text file in [BASE] data_dir, one track per line
        #                                ('spotify:track:<id>' or the bare id; blank lines and '#' lines skipped) -- the
        #                                submission holds tracks of that list only (main_challenge.read_catalogue)
        if 'allow_no_title' in sec:
            self.allow_no_title = _truth(sec['allow_no_title'])
        if 'shard_tau_exchange' in sec:
            self.shard_tau_exchange = _truth(sec['shard_tau_exchange'])
        if 'shard_exchange' in sec:
            val = sec['shard_exchange'].strip().lower()
            if val not in ('allgather', 'alltoall'):
                raise ValueError("[CHALLENGE] shard_exchange must be allgather or alltoall, not %r" % val)
            self.shard_exchange = val
        if 'catalogue' in sec and sec['catalogue'].strip():
            self.catalogue = sec['catalogue'].strip()

    set_challenge_conf = set_challenge_oonf


def load_conf(dir):
    ini = configparser.ConfigParser()
    ini.read(os.path.join(dir, 'config.ini'))
    return Conf(dir, ini)


def refuse_ensemble(conf, args):
    """[BASE] ensemble is for runs that only score: --challenge, --dae --testmode, --title --testmode.  Any other run -- a
    training run, --pretrain --testmode -- refuses the key by name, before a reader or a model is built."""
    if not getattr(conf, 'ensemble', None):
        return
    if args.challenge or (args.testmode and not args.pretrain and (args.dae or args.title)):
        return
    what = ("--pretrain" if args.pretrain else "--dae" if args.dae else "--title" if args.title else "this run") + \
        (" --testmode" if args.testmode else "")
    raise ValueError("[BASE] ensemble is set, and %s %s: the key is honoured by --challenge, --dae --testmode and "
                     "--title --testmode only (remove [BASE] ensemble / ensemble_alpha to run it)"
                     % (what, "evaluates the tied model alone" if args.testmode else "is a training run"))


def refuse_ensemble_keys(conf, args):
    """[BASE] eval_ensemble_ranks = on needs an ensemble and a run that evaluates with it (--dae --testmode, --title --testmode);
    [BASE] ensemble_fit needs its split's file.  Refused by name before a reader or a model is built."""
    if getattr(conf, 'eval_ensemble_ranks', 'off') == 'on':
        if not getattr(conf, 'ensemble', None):
            raise ValueError("[BASE] eval_ensemble_ranks = on is set without [BASE] ensemble: there is no ensemble to rank under "
                             "(remove the key, set eval_ensemble_ranks = off, or use eval_ranks)")
        if not (args.testmode and not args.pretrain and (args.dae or args.title)):
            raise ValueError("[BASE] eval_ensemble_ranks = on is honoured by --dae --testmode and --title --testmode only: this run "
                             "evaluates no ensemble (remove the key or set eval_ensemble_ranks = off)")
    if getattr(conf, 'ensemble_fit', None):
        path = os.path.join(conf.data_dir, conf.ensemble_fit[0])
        if not os.path.exists(path):
            raise ValueError("[BASE] ensemble_fit = %s: the split's file %s is missing" % (conf.ensemble_fit[0], path))


def build_parser():
    ap = argparse.ArgumentParser(description="args")
    ap.add_argument('--dir', type=str, default='qwerty', help="directory name which contains config file")
    ap.add_argument('--pretrain', action='store_true', default=False, help="pretrain mode if Specified")
    ap.add_argument('--dae', action='store_true', default=False, help="DAE mode if Specified")
    ap.add_argument('--title', action='store_true', default=False, help="title mode if Specified")
    ap.add_argument('--challenge', action='store_true', default=False, help="challenge mode if Specified")
    ap.add_argument('--testmode', action='store_true', default=False,
                    help="test mode if Specified(just check the result)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    dir = os.path.join(".", args.dir)
    if not os.path.isdir(dir):
        print("ERROR: Cannot find " + dir + " ->Create directory and config.ini file first")
        return 0
    if 'config.ini' not in os.listdir(dir):
        print("ERROR: Cannot find config.ini in " + dir + " ->Create config.ini file in the directory first")
        return 0
    conf = load_conf(dir)
    conf.set_dae_conf()                                   # always first (main.py:121)
    refuse_ensemble(conf, args)
    refuse_ensemble_keys(conf, args)
    from .main_runner import main_challenge, main_train
    if args.pretrain:
        conf.set_pretrain_conf()
        main_train.run(conf, args.testmode)
    elif args.dae:
        conf.set_dae_conf()
        main_train.run(conf, args.testmode)
    elif args.title:
        conf.set_title_conf()
        main_train.run(conf, args.testmode)
    elif args.challenge:
        if conf.eval_mixed_ranks == 'on':
            raise ValueError("[BASE] eval_mixed_ranks = on is available under --title only: --challenge evaluates nothing "
                             "(remove the key or set eval_mixed_ranks = off)")
        if conf.eval_mixed_loss == 'on':
            raise ValueError("[BASE] eval_mixed_loss = on is available under --title only: --challenge evaluates nothing "
                             "(remove the key or set eval_mixed_loss = off)")
        conf.set_title_conf()
        conf.set_challenge_oonf()
        main_challenge.run(conf)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
