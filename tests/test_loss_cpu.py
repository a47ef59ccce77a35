"""CPU: what the held-out loss needs no device for -- the [BASE] eval_loss key and where main_train refuses it by name, the
driver's targets and its line on a stub model, and the agreement of include/dae_hip.h with the ctypes bindings on the two new
entry points."""
import configparser
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _conf(extra):
    from spotify_recsys_challenge_2018_amd.main import Conf
    ini = configparser.ConfigParser()
    ini.read_string("[BASE]\nverbose = False\ndata_dir = d\nresult_dir = r\ntestsize = 10\n" + extra)
    return Conf("somewhere", ini)


def test_eval_loss_key():
    assert _conf("").eval_loss == "off"
    assert _conf("eval_loss = off\n").eval_loss == "off"
    assert _conf("eval_loss = On\n").eval_loss == "on"
    with pytest.raises(ValueError, match="eval_loss"):
        _conf("eval_loss = rows\n")


def test_eval_loss_is_refused_by_name_where_it_does_not_apply(monkeypatch):
    from spotify_recsys_challenge_2018_amd.main_runner import main_train
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    conf = _conf("eval_loss = on\n")
    conf.mode = "title"                                           # --title: before anything is read
    with pytest.raises(ValueError, match="eval_loss.*--title"):
        main_train.run(conf, True)
    conf.mode = "dae"
    conf.ensemble = ["w_other"]                                   # beside an ensemble key
    with pytest.raises(ValueError, match="eval_loss.*ensemble"):
        main_train.run(conf, True)
    conf.ensemble = []
    monkeypatch.setenv("WORLD_SIZE", "2")                         # a training run over ranks: the model is vocabulary-sharded
    with pytest.raises(ValueError, match="eval_loss.*sharded"):
        main_train.run(conf, False)
    # accepted otherwise: the run goes on to its readers (nothing else of this conf is set)
    monkeypatch.delenv("WORLD_SIZE")
    for mode, testmode in (("dae", True), ("dae", False), ("pretrain", False)):
        conf.mode = mode
        with pytest.raises(AttributeError):
            main_train.run(conf, testmode)
    conf.eval_loss = "off"
    conf.mode = "title"
    with pytest.raises(AttributeError):
        main_train.run(conf, True)


def test_heldout_targets():
    from spotify_recsys_challenge_2018_amd.main_runner.main_train import heldout_targets
    got = heldout_targets([[0, 4], [1, 2], [0, 1]], [[7, -1, 4, 12], []], 10)
    assert got.tolist() == [[0, 1], [0, 4], [0, 7], [1, 2]]       # one entry per (row, column); -1 and ids past the vocabulary left out
    assert heldout_targets(np.zeros((0, 2), np.int64), [[], []], 10).shape == (0, 2)


def test_loss_line_of_the_driver(monkeypatch):
    """eval_loss() on a stub model: feed by feed from per-row values, so a short last feed is averaged correctly."""
    from spotify_recsys_challenge_2018_amd.main_runner import main_train

    class Reader:
        test_idx = 0
        batches = [([[0, 1], [1, 2]], [[1], [2]], [[5, -1], [7]]), ([[0, 3]], [[3]], [[9, 9, 11]])]

        def next_batch_test(self):
            pos, seeds, answers = self.batches[self.test_idx]
            self.test_idx = (self.test_idx + 1) % len(self.batches)
            return np.asarray(pos), seeds, answers, [None] * len(seeds), np.ones(len(pos), np.float32)

    class Model:
        n_input = 10
        calls = []

        def loss(self, x_positions, x_ones, y_positions, y_ones, n_rows=None, per_row=False):
            assert per_row and len(y_ones) == len(y_positions) and (np.asarray(y_ones) == 1).all()
            Model.calls.append(np.asarray(y_positions).tolist())
            return 99.0, np.arange(1, n_rows + 1, dtype=np.float32) * (10.0 if n_rows == 1 else 1.0)

    assert main_train.eval_loss(Reader(), None, Model()) == pytest.approx((1.0 + 2.0 + 10.0) / 3)
    assert Model.calls == [[[0, 1], [0, 5], [1, 2], [1, 7]], [[0, 3], [0, 9]]]
    del Model.calls[:]
    lines = []
    monkeypatch.setattr(main_train, "log_write", lambda conf, log: lines.append(log))
    conf = type("C", (), {"eval_loss": "on"})()
    main_train._log_loss(conf, {"test-1": Reader()}, Model())
    assert lines == ["seed num: test-1 heldout loss: %f" % (13.0 / 3)]
    conf.eval_loss = "off"
    main_train._log_loss(conf, {"test-1": Reader()}, Model())
    assert len(lines) == 1                                        # absent / off: no line, the logs stay as they were


def test_the_models_refuse_the_loss_by_name_before_any_launch():
    from spotify_recsys_challenge_2018_amd import _lib
    from spotify_recsys_challenge_2018_amd.models.DAEs import DAE, DAE_title

    class C:
        save, initval, DAEval, batch, n_input, hidden, lr, reg_lambda = "s", "NULL", "NULL", 4, 40, 32, 0.01, 0.0
    m = DAE(C())                                                  # no fit(): nothing of a device exists
    m._score_shard = {"rank": 0}
    with pytest.raises(_lib.DaeError, match="loss.*sharded"):
        m.loss([[0, 1]], [1.0], [[0, 1]], [1.0])
    m._score_shard, m._sharded = None, object()
    with pytest.raises(_lib.DaeError, match="loss.*sharded"):
        m.loss([[0, 1]], [1.0], [[0, 1]], [1.0])
    m._sharded = None
    with pytest.raises(ValueError, match="seed"):
        m.loss([[0, 1]], [1.0], [[0, 1]], [1.0], keep_prob=0.8)
    t = DAE_title(C(), None)
    with pytest.raises(_lib.DaeError, match="DAE_title.loss.*titles in use"):
        t.loss([[0, 1]], [1.0], [[0, 1]], [1.0], titles=[[1, 2]], titles_use=[1.0, 0.0, 0.0, 0.0])


def _header_args(name):
    text = open(os.path.join(ROOT, "include", "dae_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,n_args", [("dae_decode_loss_rows", 12), ("dae_score_loss", 22)])
def test_header_and_bindings_agree(name, n_args):
    import ctypes
    from spotify_recsys_challenge_2018_amd import _lib
    args = _header_args(name)
    assert len(args) == n_args and name in _lib.EXPORTS
    lib = _lib.load()
    types = getattr(lib, name).argtypes
    assert len(types) == n_args
    for a, t in zip(args, types):
        want = ctypes.c_void_p if "*" in a else {"int": ctypes.c_int, "float": ctypes.c_float, "uint32_t": ctypes.c_uint32}[a.split()[0]]
        assert t is want, (name, a, t)
